"""NumPy restatement of the contact force sensor's outputs (include/mirigid.h: mir_contact_forces), fed from the float64 oracle.

Not a test module: tests/test_contact_forces_cpu.py pins this arithmetic on the oracle alone (Newton's laws), and
tests/test_gpu_contact_forces.py then judges the GPU with it.

The oracle hands out, per env, after forward(): the contact positions (F_CPOS), frames (F_CFRAME: normal, t1, t2), distances
(F_CDIST), the constraint Jacobian (F_J, nefc x nv) and the row forces (F_EFCFORCE).  Joint-limit rows come first, then four
friction-pyramid rows per contact, in contact order: n + mu t1, n - mu t1, n + mu t2, n - mu t2 (orc_make_rows), of the motion of
body b relative to body a.  mu is the larger friction of the two geoms (orc_rigid.c:1016).

The oracle does not hand out WHICH bodies a contact joins.  They are read off the Jacobian: the normal row of a contact is non-zero
exactly on the dofs that move one of its two bodies (+ for b, - for a), so its support names each side's set of moving dofs.  Bodies
that share that set (a fixed child and its parent, e.g. the Panda's hand and link7) cannot be told apart this way: the per-link sums
are therefore compared per CLASS of bodies with the same moving dofs (`body_classes`); the world is the class of the empty set.
"""
import numpy as np

import orc

NDOF = {0: 0, 1: 1, 2: 1, 3: 6}  # fixed, revolute, prismatic, free


def dof_start(spec):
    out, k = [], 0
    for b in range(spec.nbody):
        out.append(k)
        k += NDOF[spec.body[b].jtype]
    return out


def body_dofs(spec):
    """per body: the frozenset of dofs that move it (its own joint's and its ancestors')"""
    st = dof_start(spec)
    out = []
    for b in range(spec.nbody):
        own = set(range(st[b], st[b] + NDOF[spec.body[b].jtype]))
        out.append(frozenset(own | (set(out[spec.body[b].parent]) if b > 0 else set())))
    return out


def body_classes(spec):
    """class index per body (bodies with the same moving dofs share one), and the class -> frozenset table"""
    sets = body_dofs(spec)
    table = []
    cls = []
    for s in sets:
        if s not in table:
            table.append(s)
        cls.append(table.index(s))
    return np.array(cls), table


def uniform_mu(spec):
    """the scene's one friction coefficient (the scenes judged here have one); None if the geoms differ"""
    fr = {spec.geom[g].friction for g in range(spec.ngeom)}
    return fr.pop() if len(fr) == 1 else None


def free_bodies(spec):
    """[(body, first dof, mass)] of the free bodies whose origin is their centre of mass and whose joint has no armature or damping"""
    st = dof_start(spec)
    out = []
    for b in range(1, spec.nbody):
        if spec.body[b].jtype == 3:
            assert all(abs(x) == 0.0 for x in spec.body[b].ipos), "free body's origin must be its centre of mass"
            assert all(spec.dof[st[b] + k].armature == 0.0 and spec.dof[st[b] + k].damping == 0.0 for k in range(6))
            out.append((b, st[b], spec.body[b].mass))
    return out


def _quat_rot(q, v):
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return R @ np.asarray(v, float)


def contact_mu(o, e, spec):
    """The friction coefficient of every contact of env e, FROM THE ORACLE'S OWN ROWS: rows 0 and 1 of a contact are J_n +- mu J_t1 and
    rows 2 and 3 J_n +- mu J_t2, so (row0 - row1) / 2 = mu J_t1, where J_t1 = +- t1 . (velocity of the contact point per unit dof
    velocity).  That point velocity is kinematics alone -- axis x (p - anchor) for a revolute dof, the axis for a prismatic one, the unit
    vector for a linear dof of a free body (world-aligned), from the oracle's link poses and the spec's joint axes -- so mu is the ratio
    of the two norms over those dofs (a free body's angular dofs are left out).  No geom index is needed."""
    ncon, nefc, _ = o.counts(e)
    nv = o.nv
    nlim = nefc - 4 * ncon
    J = o.read(orc.F_J, e).reshape(nefc, nv)[nlim:].reshape(ncon, 4, nv)
    cpos = o.read(orc.F_CPOS, e).reshape(ncon, 3)
    frm = o.read(orc.F_CFRAME, e).reshape(ncon, 3, 3)
    xpos = o.read(orc.F_XPOS, e).reshape(spec.nbody, 3)
    xquat = o.read(orc.F_XQUAT, e).reshape(spec.nbody, 4)
    st = dof_start(spec)
    mu = np.zeros(ncon)
    for c in range(ncon):
        num = den = 0.0
        for b in range(1, spec.nbody):
            jt = spec.body[b].jtype
            cols = []
            if jt in (1, 2):
                a = _quat_rot(xquat[b], list(spec.body[b].axis))
                cols = [(st[b], np.cross(a, cpos[c] - xpos[b]) if jt == 1 else a)]
            elif jt == 3:
                cols = [(st[b] + k, np.eye(3)[k]) for k in range(3)]
            for d, col in cols:
                if np.abs(J[c, :, d]).max() == 0.0:
                    continue  # (the dof moves neither side of this contact)
                num += (0.5 * (J[c, 0, d] - J[c, 1, d])) ** 2 + (0.5 * (J[c, 2, d] - J[c, 3, d])) ** 2
                den += float(frm[c, 1] @ col) ** 2 + float(frm[c, 2] @ col) ** 2
        assert den > 0.0, (c, "no dof with a tangential effect on this contact")
        mu[c] = np.sqrt(num / den)
    return mu


def pair_mu_values(spec):
    """every value max(friction_g1, friction_g2) can take in the scene"""
    fr = sorted({spec.geom[g].friction for g in range(spec.ngeom)})
    return sorted({max(a, b) for a in fr for b in fr})


def contact_forces(o, e, mu, classes=None, spec=None):
    """From env e of an oracle after forward(): dict with n, position (n,3), normal (n,3), penetration (n), force (n,3; on side b),
    rowforce (n,4), mu (n), cls_a / cls_b (n; class of each side, `classes` = body_classes(spec)) and class_force (nclass,3).
    mu: the scene's one coefficient, or None = per contact from the oracle's rows (contact_mu; needs `spec`)."""
    if mu is None:
        mu = contact_mu(o, e, spec)
    ncon, nefc, _ = o.counts(e)
    nv = o.nv
    nlim = nefc - 4 * ncon
    cpos = o.read(orc.F_CPOS, e).reshape(ncon, 3)
    frm = o.read(orc.F_CFRAME, e).reshape(ncon, 3, 3)
    dist = o.read(orc.F_CDIST, e)[:ncon]
    J = o.read(orc.F_J, e).reshape(nefc, nv)
    f = o.read(orc.F_EFCFORCE, e)[:nefc]
    fr = f[nlim:].reshape(ncon, 4)
    n, t1, t2 = frm[:, 0], frm[:, 1], frm[:, 2]
    force = (fr.sum(1))[:, None] * n + (mu * (fr[:, 0] - fr[:, 1]))[:, None] * t1 + (mu * (fr[:, 2] - fr[:, 3]))[:, None] * t2
    out = dict(n=ncon, nlim=nlim, mu=np.broadcast_to(np.asarray(mu, float), (ncon,)), position=cpos, normal=n, penetration=-dist, force=force, rowforce=fr, J=J, efcforce=f)
    if classes is not None:
        cls, table = classes
        Jn = 0.5 * (J[nlim::4] + J[nlim + 1::4]) if ncon else np.zeros((0, nv))
        Jc = J[nlim:].reshape(ncon, 4, nv)
        ca, cb = np.zeros(ncon, int), np.zeros(ncon, int)
        for c in range(ncon):
            # the support of the contact's rows splits into the moving-dof sets of its two sides (self-collision is off in the scenes
            # judged here: the two sides are different trees, or one is the world).  Which side is b: the normal row on the linear
            # dofs of a free body is +n where the body is b and -n where it is a; a jointed body against the world is b (the plane
            # comes first in a pair).
            sup = frozenset(np.nonzero(np.abs(Jc[c]).max(0) > 0)[0].tolist())
            sides = []
            for s in table:
                if s and s <= sup and not any(s < t and t <= sup for t in table):
                    sides.append(s)
            assert 1 <= len(sides) <= 2 and frozenset().union(*sides) == sup, (c, sup, sides)
            free_lin = {}
            for s in sides:
                k = max(s)  # (the last three dofs of a free body are angular, the three before linear)
                if len(s) == 6 and np.allclose(Jn[c][[k - 5, k - 4, k - 3]], n[c], atol=1e-5):
                    free_lin[s] = +1
                elif len(s) == 6 and np.allclose(Jn[c][[k - 5, k - 4, k - 3]], -n[c], atol=1e-5):
                    free_lin[s] = -1
            if len(sides) == 2:
                known = [s for s in sides if s in free_lin]
                assert known, "a contact between two jointed trees: not handled here"
                sb = known[0] if free_lin[known[0]] > 0 else [s for s in sides if s is not known[0]][0]
                sa = [s for s in sides if s is not sb][0]
            else:  # the world is the other side
                s = sides[0]
                if s in free_lin:
                    sb, sa = (s, frozenset()) if free_lin[s] > 0 else (frozenset(), s)
                else:
                    # a jointed body against the world: the plane (world) comes first in a pair, so the jointed body is side b
                    sb, sa = s, frozenset()
            ca[c], cb[c] = table.index(sa), table.index(sb)
        cf = np.zeros((len(table), 3))
        for c in range(ncon):
            cf[cb[c]] += force[c]
            cf[ca[c]] -= force[c]
        out.update(cls_a=ca, cls_b=cb, class_force=cf)
    return out


def class_sum(link_force, cls, nclass):
    """(nbody,3) per-link forces summed per class of bodies"""
    out = np.zeros((nclass, 3))
    for b in range(link_force.shape[0]):
        out[cls[b]] += link_force[b]
    return out
