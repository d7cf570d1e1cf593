// mir_dyn_phases.inc -- the first phases of the kernels of mir_dyn.hip and mir_osc.hip, as one textual fragment both include at the top
// of the kernel body: what a lane is in its (row, tree) pair, the tables of the tree every lane can reach and an empty M block, world
// poses level by level, spatial inertias about the tree origin, motion subspaces, and (where `want_mass`) the composite-rigid-body M
// block in LDS.
// In scope at the point of inclusion: the kernel arguments `a` (tree[], n_rows, n_trees, B, env_idx, qpos, qpos_o, nq, qst, depth_max,
// nb_max; m = JointPtrs: b_pos, b_quat, b_axis, b_qadr, d_lane; mi = InertiaPtrs: b_ipos, b_inertia, b_mass, d_armature), the pair's
// LDS struct `L` (pd, sd, inv, M, xp, xq, ci, cd) and `const bool want_mass`.
// It leaves behind: lane, row, ti, env, nb, nd, valid, isbody, isdof; body, jt, par, depth, dof1 (the lane as a body); sdof, dbody,
// pdof (the lane as a dof); qrow, P, Qx, baxis, S, sub.  Its own temporaries are named ph_*.
  const PairLane ph_pair = pair_decode(a, a.n_trees);
  const int lane = ph_pair.lane, row = ph_pair.row, ti = ph_pair.item, env = ph_pair.env;
  const bool valid = ph_pair.valid;
  const int nb = a.tree[ti].nb, nd = a.tree[ti].nd;
  const bool isbody = lane < nb, isdof = lane < nd;
  const uint32_t ph_bw = isbody ? a.tree[ti].body[lane] : 0u;
  const uint32_t ph_dw = isdof ? a.tree[ti].dof[lane] : 0u;
  const int body = ph_bw & 0xff, jt = (ph_bw >> 8) & 3, par = (ph_bw >> 10) & 15, depth = (ph_bw >> 14) & 15, dof1 = isbody ? (int)((ph_bw >> 18) & 15) : DYN_NONE;
  const int sdof = ph_dw & 0xff, dbody = (ph_dw >> 8) & 15, pdof = isdof ? (int)((ph_dw >> 12) & 15) : DYN_NONE;
  const float* const qrow = a.qpos_o ? a.qpos_o + (size_t)row * a.nq : a.qpos + (size_t)env * a.qst;
  // ---- tables of the tree every lane can reach, an empty M block
  L.pd[lane] = pdof;
  L.sd[lane] = sdof;
  for (int i = lane; i < MIR_MAX_DOF; i += G) L.inv[i] = 0xff;
#pragma unroll
  for (int j = 0; j < G; j++) L.M[lane][j] = 0.0f;
  WSYNC();
  if (isdof) L.inv[sdof] = (uint8_t)lane;
  // ---- local transform of my body
  const JointLocal jl0 = joint_local(isbody, body, jt, qrow, a.m);
  const V3 baxis = jl0.baxis;
  V3 P = jl0.P;
  Q4 Qx = jl0.Qx;
  // ---- world poses, one level of the tree at a time (a free body's pose is its qpos row, as in orc_fk)
  for (int lvl = 0; lvl <= a.depth_max; lvl++) {
    if (isbody && depth == lvl) {
      if (lvl > 0 && jt != MIR_JNT_FREE) {
        const V3 pp = ld3(L.xp[par]);
        const Q4 pq = ld4(L.xq[par]);
        P = pp + qrot(pq, P);
        Qx = qmul(pq, Qx);
      }
      st3(L.xp[lane], P);
      st4(L.xq[lane], Qx);
    }
    WSYNC();
  }
  // ---- spatial inertia about the tree origin (the root body's origin), world axes; motion subspaces of my body's dofs
  const V3 ph_cref = ld3(L.xp[0]);
  {
    float c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (isbody) {
      const M3 R = q2m(Qx);
      const float* const ib = a.mi.b_inertia + body * 6;
      const V3 i0 = v3(ib[0], ib[3], ib[4]), i1 = v3(ib[3], ib[1], ib[5]), i2 = v3(ib[4], ib[5], ib[2]);
      const V3 t0 = R.r0.x * i0 + R.r0.y * i1 + R.r0.z * i2;
      const V3 t1 = R.r1.x * i0 + R.r1.y * i1 + R.r1.z * i2;
      const V3 t2 = R.r2.x * i0 + R.r2.y * i1 + R.r2.z * i2;
      const V3 r = P + mmul(R, ld3(a.mi.b_ipos + body * 3)) - ph_cref;
      const float ms = a.mi.b_mass[body], rr = dot(r, r);
      c[0] = ms; c[1] = ms * r.x; c[2] = ms * r.y; c[3] = ms * r.z;
      c[4] = dot(t0, R.r0) + ms * (rr - r.x * r.x);
      c[5] = dot(t1, R.r1) + ms * (rr - r.y * r.y);
      c[6] = dot(t2, R.r2) + ms * (rr - r.z * r.z);
      c[7] = dot(t0, R.r1) - ms * r.x * r.y;
      c[8] = dot(t0, R.r2) - ms * r.x * r.z;
      c[9] = dot(t1, R.r2) - ms * r.y * r.z;
      const V3 rc = ph_cref - P;
      if (jt == MIR_JNT_REVOLUTE || jt == MIR_JNT_PRISMATIC) {
        const V3 axw = mmul(R, baxis);
        const Sp s = jt == MIR_JNT_REVOLUTE ? Sp{axw, cross(axw, rc)} : Sp{v3(0, 0, 0), axw};
        if (dof1 != DYN_NONE) sts6(L.cd[dof1], s);
      } else if (jt == MIR_JNT_FREE && dof1 != DYN_NONE) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const V3 ek = v3(k == 0 ? 1.0f : 0.0f, k == 1 ? 1.0f : 0.0f, k == 2 ? 1.0f : 0.0f);
          sts6(L.cd[dof1 + k], Sp{v3(0, 0, 0), ek});
          sts6(L.cd[dof1 + 3 + k], Sp{ek, cross(ek, rc)});
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 10; k++) L.ci[lane][k] = c[k];
  }
  WSYNC();
  const Sp S = isdof ? lds6(L.cd[lane]) : Sp{v3(0, 0, 0), v3(0, 0, 0)};
  const int sub = a.tree[ti].sub[isdof ? dbody : 0];
  // ---- mass matrix: composite inertia of my dof's body, M[i][j] up dof_parent, armature on the diagonal
  if (want_mass) {
    float c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < a.nb_max; b++) {
      if (isdof && (sub >> b & 1)) {
#pragma unroll
        for (int k = 0; k < 10; k++) c[k] += L.ci[b][k];
      }
    }
    if (isdof) {
      const Inert I = {c[0], {c[1], c[2], c[3]}, c[4], c[5], c[6], c[7], c[8], c[9]};
      Sp f;
      imul(I, S.a, S.b, f.a, f.b);
      const float arm = a.mi.d_armature[a.m.d_lane[sdof]];
      for (int j = lane; j != DYN_NONE; j = L.pd[j]) {
        float v = dot6(lds6(L.cd[j]), f);
        if (j == lane) v += arm;
        L.M[lane][j] = v;
        L.M[j][lane] = v;
      }
    }
  }
