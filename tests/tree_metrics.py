"""Error metrics per kinematic tree and per dof kind, for the GPU parity tests of the query kernels.  A helper, no test.

One max-abs yardstick over all dofs of a scene lets the tree with the largest numbers hide the others (a cube's rotational block of M^-1
is ~3e5, the arm's ~10; the arm's mass entries are ~1, a cube's rotational inertia 3e-6).  Here the dofs are grouped by (tree, kind),
kind = free-linear, free-angular or scalar joint; a vector over the dofs gets one metric per group, a matrix over the dofs one per
ordered pair of groups of the same tree, a per-link output one per tree of the links (split into its linear and angular halves).

Allowed per block: max(4 x the float32 port's error on that block, 2^-23 x max |reference| of that block) -- the project's rule for a
float32 kernel that sums in another order than the serial walk, with a floor of one float32 rounding of the block's largest entry
(some blocks are exact in the port, and a float32 result is not owed more than that).
"""
from __future__ import annotations

import numpy as np

import kin_ref

EPS32 = 2.0 ** -23


def tree_of_body(model) -> list:
    """root body (child of the world) of every body's tree; 0 for the world"""
    root = [0] * model.nbody
    for b in range(1, model.nbody):
        root[b] = b if model.parent[b] == 0 else root[model.parent[b]]
    return root


def dof_groups(model) -> list:
    """[(label, dof indices)] with label = (tree root body, kind), kind in "lin" / "ang" (free joint) / "joint", in dof order"""
    root = tree_of_body(model)
    groups = {}
    for b in range(1, model.nbody):
        d, jt = model.dofadr[b], model.jtype[b]
        if jt == kin_ref.FREE:
            groups.setdefault((root[b], "lin"), []).extend(range(d, d + 3))
            groups.setdefault((root[b], "ang"), []).extend(range(d + 3, d + 6))
        elif jt in (kin_ref.REVOLUTE, kin_ref.PRISMATIC):
            groups.setdefault((root[b], "joint"), []).append(d)
    return [(k, np.array(v)) for k, v in groups.items()]


def link_groups(model, links) -> list:
    """[(tree root body, positions in `links`)]: the queried links by tree"""
    root = tree_of_body(model)
    groups = {}
    for i, b in enumerate(links):
        groups.setdefault(root[int(b)], []).append(i)
    return [(k, np.array(v)) for k, v in groups.items()]


def allowed(port_err: float, ref_block) -> float:
    return max(4.0 * port_err, EPS32 * float(np.abs(ref_block).max()) if np.size(ref_block) else 0.0)


def _row(label, got, port, ref):
    e, p = float(np.abs(got - ref).max()), float(np.abs(port - ref).max())
    return (label, e, p, allowed(p, ref))


def vector_blocks(model, got, port, ref, window=None) -> list:
    """(B, nv) outputs -> [(label, gpu error, port error, allowed)], one per group; `window` = (dof0, n_dofs) of `got` (port / ref full)"""
    d0, nd = window or (0, model.nv)
    out = []
    for label, idx in dof_groups(model):
        idx = idx[(idx >= d0) & (idx < d0 + nd)]
        if idx.size:
            out.append(_row(label, got[:, idx - d0], port[:, idx], ref[:, idx]))
    return out


def matrix_blocks(model, got, port, ref, window=None) -> list:
    """(B, nv, nv) outputs -> one row per ordered pair of groups of the same tree"""
    d0, nd = window or (0, model.nv)
    groups = [(label, idx[(idx >= d0) & (idx < d0 + nd)]) for label, idx in dof_groups(model)]
    out = []
    for la, ia in groups:
        for lb, ib in groups:
            if la[0] == lb[0] and ia.size and ib.size:
                g = got[:, (ia - d0)[:, None], (ib - d0)[None, :]]
                out.append(_row((la[0], la[1], lb[1]), g, port[:, ia[:, None], ib[None, :]], ref[:, ia[:, None], ib[None, :]]))
    return out


def link_blocks(model, links, got, port, ref, halves=True) -> list:
    """(B, L, 3 | 4 | 6) per-link outputs -> one row per tree of the links (6-wide: per tree and linear / angular half)"""
    out = []
    for tree, pos in link_groups(model, links):
        g, p, r = got[:, pos], port[:, pos], ref[:, pos]
        if halves and got.shape[-1] == 6:
            out.append(_row((tree, "lin"), g[..., 0:3], p[..., 0:3], r[..., 0:3]))
            out.append(_row((tree, "ang"), g[..., 3:6], p[..., 3:6], r[..., 3:6]))
        else:
            out.append(_row((tree,), g, p, r))
    return out


def jac_blocks(model, links, got, port, ref, window=None) -> list:
    """(B, L, 6, nv) Jacobians -> one row per (tree of the links, linear / angular rows, dof group of that tree)"""
    d0, nd = window or (0, model.nv)
    out = []
    for tree, pos in link_groups(model, links):
        for label, idx in dof_groups(model):
            idx = idx[(idx >= d0) & (idx < d0 + nd)]
            if label[0] != tree or not idx.size:
                continue
            for half, rows in (("lin", slice(0, 3)), ("ang", slice(3, 6))):
                pick = lambda a, cols: a[:, pos][:, :, rows][..., cols]  # noqa: E731
                out.append(_row((tree, half, label[1]), pick(got, idx - d0), pick(port, idx), pick(ref, idx)))
    return out


def report(title: str, rows: list) -> list:
    """prints every figure; -> the rows that miss their bar"""
    for label, e, p, a in rows:
        print(f"[{title}] {str(label):>28}: GPU {e:.3e} port {p:.3e} allowed {a:.3e}" + ("" if e <= a else "   <-- MISS"))
    return [(title, label, e, p, a) for label, e, p, a in rows if not e <= a]
