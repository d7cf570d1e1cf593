"""Thin read/write views over a MirScene that mirror the slice of the Genesis object API the
reference tasks and examples call on the hot path: ``scene.step()``,
``entity.get_pos/get_quat/get_dofs_position/get_qpos/get_link``, ``link.get_pos/get_quat``,
``entity.control_dofs_position`` (/root/reference/gym_genesis/tasks/franka/cube_pick.py:96-146,
/root/reference/gym_genesis/env.py:59-60).  All tensors are float32 on the scene's device,
batch first, quaternions wxyz.
"""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np
import torch


def _rows(t: torch.Tensor, envs_idx) -> torch.Tensor:
    """The rows `envs_idx` of a batch-first tensor, as Genesis's getters return them (`envs_idx=None`: all envs).  The reference's
    SO-101 expert asks for `robot.get_qpos(envs_idx=np.arange(B))` and `get_link("gripper").get_pos(envs_idx=torch.arange(B))`
    (/root/reference/examples/so_101/collect_task_stack_cube_batch.py:73,86,90): NumPy, torch (any device) and lists are accepted."""
    if envs_idx is None:
        return t
    if not (isinstance(envs_idx, torch.Tensor) and envs_idx.is_cuda):
        host = np.asarray(envs_idx.cpu() if isinstance(envs_idx, torch.Tensor) else envs_idx).reshape(-1)
        if host.size == t.shape[0] and np.array_equal(host, np.arange(t.shape[0])):
            return t  # (the experts' arange(B): no gather, no upload)
        envs_idx = host
    return t.index_select(0, torch.as_tensor(envs_idx, device=t.device).long().reshape(-1))


# robot.inverse_kinematics as ONE launch (mir_inverse_kinematics_rows); False: the full-batch launch with torch scatter / gather around it
IK_ROWS = True
# (an index outside the batch is clamped by the kernel; checking it here would cost a device -> host synchronisation per call)
CHECK_IK_IDX = False
from ..backend.spec import IK_INIT_BY_ENV, IK_POS_BY_ENV, IK_QUAT_BY_ENV, IK_QUAT_ONE  # noqa: E402


def _env_index(mir, envs_idx):
    """`envs_idx` of a getter as the row list of MirScene.link_kinematics: None for all envs in order (also the experts' arange(B)), else
    an int64 tensor.  Indices given on the host are checked here (IndexError); a device tensor is not read back -- the kernel clamps it."""
    if envs_idx is None:
        return None
    B = mir.num_envs
    if isinstance(envs_idx, slice):
        envs_idx = np.arange(B)[envs_idx]
    if isinstance(envs_idx, torch.Tensor) and envs_idx.is_cuda:
        return envs_idx.long().reshape(-1)
    host = np.asarray(envs_idx.cpu() if isinstance(envs_idx, torch.Tensor) else envs_idx).reshape(-1)
    if host.size and not np.issubdtype(host.dtype, np.integer):
        raise IndexError(f"envs_idx must be integers, got {host.dtype}")
    host = host.astype(np.int64)
    if host.size and (host.min() < -B or host.max() >= B):
        raise IndexError(f"envs_idx outside the batch of {B} envs")
    host = np.where(host < 0, host + B, host)
    if host.size == B and np.array_equal(host, np.arange(B)):
        return None
    return torch.as_tensor(host, device=mir.device)


def _kinematics(mir, **kw) -> dict:
    fn = getattr(mir, "link_kinematics", None)
    if fn is None:
        raise NotImplementedError("this scene has no link kinematics (MirScene.link_kinematics / mir_link_kinematics)")
    return fn(**kw)


def _accelerations(mir, **kw) -> dict:
    fn = getattr(mir, "link_accelerations", None)
    if fn is None:
        raise NotImplementedError("this scene has no link accelerations (MirScene.link_accelerations / mir_link_accelerations)")
    return fn(**kw)


class LinkView:
    def __init__(self, mir, body_index: int, name: str):
        self._mir, self.idx, self.name = mir, body_index, name

    def get_acc(self, envs_idx=None) -> torch.Tensor:
        """(B, 3): classical world linear acceleration of the link's origin, for the acceleration the next step applies if the targets
        stay as they are (EntityView.get_links_acc for one link)."""
        k = _accelerations(self._mir, links=[self.idx], env_idx=_env_index(self._mir, envs_idx))
        return k["acc"][:, 0, 0:3].contiguous()

    def get_ang_acc(self, envs_idx=None) -> torch.Tensor:
        """(B, 3): world angular acceleration of the link.  This package's own name: parity with Genesis is unpinned."""
        k = _accelerations(self._mir, links=[self.idx], env_idx=_env_index(self._mir, envs_idx))
        return k["acc"][:, 0, 3:6].contiguous()

    def get_vel(self, envs_idx=None) -> torch.Tensor:
        """(B, 3): world linear velocity of the link's origin (Genesis: RigidLink.get_vel)."""
        k = _kinematics(self._mir, links=[self.idx], env_idx=_env_index(self._mir, envs_idx), pos=False, quat=False, jac=False)
        return k["vel"][:, 0, 0:3].contiguous()

    def get_ang(self, envs_idx=None) -> torch.Tensor:
        """(B, 3): world angular velocity of the link (Genesis: RigidLink.get_ang)."""
        k = _kinematics(self._mir, links=[self.idx], env_idx=_env_index(self._mir, envs_idx), pos=False, quat=False, jac=False)
        return k["vel"][:, 0, 3:6].contiguous()

    def get_pos(self, envs_idx=None) -> torch.Tensor:
        return _rows(self._mir.get_links()[0][:, self.idx, :].contiguous(), envs_idx)

    def get_quat(self, envs_idx=None) -> torch.Tensor:
        return _rows(self._mir.get_links()[1][:, self.idx, :].contiguous(), envs_idx)


class EntityView:
    """One articulated entity (robot) or free body (cube): the bodies of one kinematic tree."""

    def __init__(self, mir, builder, root: str, dof_names: Sequence[str]):
        self._mir, self._b = mir, builder
        self.root = builder.body_index(root)
        self.dof_names = tuple(dof_names)
        self.dof_idx = [builder.dof_index(n) for n in dof_names]
        # qpos column of each scalar dof (scalar joints come first in every scene built here)
        self._qcols = list(self.dof_idx)
        qc = self._qcols
        self._qcols_run = bool(qc) and qc == list(range(qc[0], qc[0] + len(qc)))   # (a run of columns: a slice serves them)
        ctrl = [i for i, d in enumerate(builder.dofs) if d["ctrl_mode"] == 1]
        self._ucols = [ctrl.index(i) for i in self.dof_idx if i in ctrl]
        # the links of this entity: its root and everything below it, in body order
        self.link_idx = [self.root]
        for i, b in enumerate(builder.bodies):
            if i > self.root and b["parent"] in self.link_idx:
                self.link_idx.append(i)

    @property
    def n_links(self) -> int:
        return len(self.link_idx)

    # ---- contact force sensing (Genesis: RigidEntity.get_links_net_contact_force / get_contacts).  The forces are those of a forward
    # evaluation at the CURRENT state with the CURRENT PD targets -- what the next scene.step() applies if the targets stay -- where
    # Genesis reports the forces of the step just taken.  One launch per state serves every getter of every entity (MirScene.contact_sensor).
    def _sensor(self) -> dict:
        sensor = getattr(self._mir, "contact_sensor", None)
        if sensor is None:
            raise NotImplementedError("this scene has no contact force sensing (MirScene.contact_sensor / mir_contact_forces)")
        return sensor()

    def _links_t(self, device) -> torch.Tensor:
        ix = self.__dict__.get("_link_idx_t")
        if ix is None or ix.device != device:
            ix = self._link_idx_t = torch.as_tensor(self.link_idx, dtype=torch.long, device=device)
        return ix

    def get_links_net_contact_force(self, envs_idx=None) -> torch.Tensor:
        """(B, n_links, 3) float32, device: the net contact force on each link of this entity, world frame."""
        lf = self._sensor()["link_force"]
        return _rows(lf.index_select(1, self._links_t(lf.device)), envs_idx)

    def get_contacts(self, with_entity=None, envs_idx=None) -> dict:
        """The contacts that involve this entity (and `with_entity`, when given), padded to 48 rows per env in the solver's contact
        order: geom_a, geom_b, link_a, link_b (B,48) int32 (-1 in the rows that are not valid), position, force_a, force_b (B,48,3),
        penetration (B,48), valid_mask (B,48) bool.  force_b is the force on link_b, force_a = -force_b the one on link_a."""
        s = self._sensor()
        ids, gp, force = s["ids"], s["pos_normal_pen"], s["force"]
        B, K = ids.shape[0], ids.shape[1]
        valid = torch.arange(K, device=ids.device)[None, :] < s["n_contacts"][:, None]

        def touches(ent):
            lk = ent._links_t(ids.device)
            return (ids[:, :, 2, None] == lk).any(-1), (ids[:, :, 3, None] == lk).any(-1)

        a_me, b_me = touches(self)
        mask = valid & (a_me | b_me)
        if with_entity is not None:
            a_ot, b_ot = touches(with_entity)
            mask = valid & ((a_me & b_ot) | (b_me & a_ot))
        neg = torch.full_like(ids[:, :, 0], -1)
        fb = torch.where(mask[:, :, None], force, torch.zeros_like(force))
        out = {"geom_a": torch.where(mask, ids[:, :, 0], neg), "geom_b": torch.where(mask, ids[:, :, 1], neg),
               "link_a": torch.where(mask, ids[:, :, 2], neg), "link_b": torch.where(mask, ids[:, :, 3], neg),
               "position": torch.where(mask[:, :, None], gp[:, :, 0:3], torch.zeros_like(force)),
               "force_a": -fb, "force_b": fb,
               "penetration": torch.where(mask, gp[:, :, 6], torch.zeros_like(gp[:, :, 6])), "valid_mask": mask}
        return {k: _rows(v, envs_idx) for k, v in out.items()}

    @property
    def n_dofs(self) -> int:
        return len(self.dof_idx)

    # ---- differential kinematics (Genesis: RigidEntity.get_jacobian / get_links_pos / get_links_quat / get_links_vel / get_links_ang).
    # One launch of mir_link_kinematics per call, for the links and envs asked for only; links_kinematics() returns several of the
    # get_links_* results from ONE launch.
    def _jac_dofs(self) -> list:
        """The scene dofs behind the Jacobian's columns, in this entity's dof order: its named dofs (the Panda's nine), or -- an entity
        built without dof names, a free cube -- the dofs of its links in body order (the cube's six)."""
        cols = self.__dict__.get("_jac_cols")
        if cols is None:
            cols = list(self.dof_idx)
            if not cols:
                first, nd = 0, {0: 0, 1: 1, 2: 1, 3: 6}
                for i, b in enumerate(self._b.bodies):
                    n = nd[b["jtype"]] if i > 0 else 0
                    if i in self.link_idx:
                        cols.extend(range(first, first + n))
                    first += n
            self._jac_cols = cols
        return cols

    def _link_body(self, link) -> int:
        """a LinkView of this entity, or a local link index -> body index of the scene"""
        if isinstance(link, LinkView):
            if link.idx not in self.link_idx:
                raise ValueError(f"link {link.name!r} does not belong to this entity")
            return link.idx
        i = int(link)
        if not -self.n_links <= i < self.n_links:
            raise IndexError(f"local link index {i} outside the entity's {self.n_links} links")
        return self.link_idx[i]

    def _link_bodies(self, links_idx_local) -> list:
        if links_idx_local is None:
            return list(self.link_idx)
        return [self._link_body(i) for i in np.asarray(links_idx_local).reshape(-1).tolist()]

    def get_jacobian(self, link, local_point=None, envs_idx=None) -> torch.Tensor:
        """``robot.get_jacobian(link)`` -> (B, 6, n): rows 0-2 map this entity's dof velocities to the world linear velocity of the link's
        origin (of `local_point`, given in the link's frame), rows 3-5 to the link's world angular velocity; the columns are the entity's
        own dofs in its dof order (9 for the Panda, 6 for a free cube)."""
        cols = self._jac_dofs()
        run = bool(cols) and cols == list(range(cols[0], cols[0] + len(cols)))
        kw = dict(dof0=cols[0], n_dofs=len(cols)) if run else {}
        k = _kinematics(self._mir, links=[self._link_body(link)], local_points=None if local_point is None else [float(v) for v in np.asarray(local_point).reshape(3)],
                        env_idx=_env_index(self._mir, envs_idx), pos=False, quat=False, vel=False, **kw)
        jac = k["jac"][:, 0]
        if not run:
            jac = jac.index_select(2, torch.as_tensor(cols, dtype=torch.long, device=jac.device))
        return jac.contiguous()

    def links_kinematics(self, links_idx_local=None, envs_idx=None, pos=True, quat=True, vel=True) -> dict:
        """pos (B,n,3), quat (B,n,4), vel (B,n,3), ang (B,n,3) of this entity's links (all, or the local indices given) from ONE launch."""
        k = _kinematics(self._mir, links=self._link_bodies(links_idx_local), env_idx=_env_index(self._mir, envs_idx), pos=pos, quat=quat, vel=vel, jac=False)
        out = {n: k[n] for n in ("pos", "quat") if n in k}
        if "vel" in k:
            out["vel"], out["ang"] = k["vel"][:, :, 0:3].contiguous(), k["vel"][:, :, 3:6].contiguous()
        return out

    def get_links_pos(self, links_idx_local=None, envs_idx=None) -> torch.Tensor:
        return self.links_kinematics(links_idx_local, envs_idx, quat=False, vel=False)["pos"]

    def get_links_quat(self, links_idx_local=None, envs_idx=None) -> torch.Tensor:
        return self.links_kinematics(links_idx_local, envs_idx, pos=False, vel=False)["quat"]

    def get_links_vel(self, links_idx_local=None, envs_idx=None) -> torch.Tensor:
        """(B, n_links, 3): world linear velocity of each link's origin"""
        return self.links_kinematics(links_idx_local, envs_idx, pos=False, quat=False)["vel"]

    def get_links_ang(self, links_idx_local=None, envs_idx=None) -> torch.Tensor:
        """(B, n_links, 3): world angular velocity of each link"""
        return self.links_kinematics(links_idx_local, envs_idx, pos=False, quat=False)["ang"]

    # ---- link accelerations (MirScene.link_accelerations / mir_link_accelerations): one launch per call, for the links and envs asked for
    # only.  The acceleration is the one the next scene.step() applies if the targets stay as they are (one forward evaluation, the
    # convention of the contact forces) -- Genesis reports that of the step just taken; parity with Genesis is unpinned.
    def links_accelerations(self, links_idx_local=None, envs_idx=None) -> dict:
        """acc (B,n,3), ang_acc (B,n,3) of this entity's links (all, or the local indices given) from ONE launch."""
        k = _accelerations(self._mir, links=self._link_bodies(links_idx_local), env_idx=_env_index(self._mir, envs_idx))
        return {"acc": k["acc"][:, :, 0:3].contiguous(), "ang_acc": k["acc"][:, :, 3:6].contiguous()}

    def get_links_acc(self, links_idx_local=None, envs_idx=None) -> torch.Tensor:
        """``entity.get_links_acc()`` (a Genesis name) -> (B, n_links, 3): classical world linear acceleration of each link's origin.
        Gravity is not added: a link at rest reads 0 (an IMU sensor reads +9.81 up: tasks/sensors.py)."""
        return self.links_accelerations(links_idx_local, envs_idx)["acc"]

    def get_links_ang_acc(self, links_idx_local=None, envs_idx=None) -> torch.Tensor:
        """(B, n_links, 3): world angular acceleration of each link.  This package's own name: parity with Genesis is unpinned."""
        return self.links_accelerations(links_idx_local, envs_idx)["ang_acc"]

    def get_jacobian_dot_qvel(self, link, local_point=None, envs_idx=None) -> torch.Tensor:
        """(B, 6): Jdot qvel of the link's origin (of `local_point`, given in the link's frame) -- the acceleration of the point and the
        angular acceleration of the link at qacc = 0, the term of a = J qacc + Jdot qvel beside get_jacobian's J.  It needs no forward
        evaluation.  This package's own name: parity with Genesis is unpinned."""
        k = _accelerations(self._mir, links=[self._link_body(link)], local_points=None if local_point is None else [float(v) for v in np.asarray(local_point).reshape(3)],
                           env_idx=_env_index(self._mir, envs_idx), acc=False, bias_acc=True)
        return k["bias_acc"][:, 0].contiguous()

    # ---- rigid-body dynamics queries (MirScene.dynamics / mir_dynamics): one launch per call, for this entity's dofs and the envs asked
    # for only.  get_mass_mat and get_dofs_control_force are Genesis names (RigidEntity); get_dofs_bias_force, get_dofs_gravity_force and
    # inverse_dynamics are this package's own, and parity with Genesis is unpinned for all of them (the reference's tasks call none).
    def _dynamics(self, envs_idx, dofs_idx_local, name: str, **kw) -> torch.Tensor:
        fn = getattr(self._mir, "dynamics", None)
        if fn is None:
            raise NotImplementedError("this scene has no dynamics queries (MirScene.dynamics / mir_dynamics)")
        cols = self._jac_dofs()
        run = bool(cols) and cols == list(range(cols[0], cols[0] + len(cols)))
        win = dict(dof0=cols[0], n_dofs=len(cols)) if run else {}
        flags = dict(mass=False, bias=False, gravity=False, tau=False, ctrl_force=False)
        flags[name] = True
        out = fn(env_idx=_env_index(self._mir, envs_idx), **win, **flags, **kw)[name]
        if not run:
            ix = torch.as_tensor(cols, dtype=torch.long, device=out.device)
            out = out.index_select(1, ix)
            if name == "mass":
                out = out.index_select(2, ix)
        if dofs_idx_local is not None:
            out = out[:, [int(i) for i in np.asarray(dofs_idx_local).ravel()]]
        return out.contiguous()

    def get_mass_mat(self, envs_idx=None, decompose: bool = False) -> torch.Tensor:
        """``entity.get_mass_mat()`` (a Genesis name) -> (B, n, n): the joint-space mass matrix of this entity's dofs in its dof order,
        by the composite-rigid-body algorithm, with the dofs' armature on the diagonal and without the integrator's dt (damping + kv)."""
        if decompose:
            raise NotImplementedError("decompose")
        return self._dynamics(envs_idx, None, "mass")

    def get_dofs_control_force(self, dofs_idx_local=None, envs_idx=None) -> torch.Tensor:
        """``entity.get_dofs_control_force()`` (a Genesis name) -> (B, n): clamp(kp (target - q) - kv qvel, force range) of the
        position-controlled dofs, 0 for the others: the PD torque the next step applies if the targets stay as they are."""
        return self._dynamics(envs_idx, dofs_idx_local, "ctrl_force")

    def get_dofs_bias_force(self, dofs_idx_local=None, envs_idx=None) -> torch.Tensor:
        """(B, n): Coriolis, centrifugal and gravity forces c(q, qvel) of M qacc + c = applied torque.  This package's own name:
        parity with Genesis is unpinned."""
        return self._dynamics(envs_idx, dofs_idx_local, "bias")

    def get_dofs_gravity_force(self, dofs_idx_local=None, envs_idx=None) -> torch.Tensor:
        """(B, n): the bias force at qvel = 0, the torque that holds the pose at rest (gravity compensation).  This package's own name:
        parity with Genesis is unpinned."""
        return self._dynamics(envs_idx, dofs_idx_local, "gravity")

    def inverse_dynamics(self, qacc, qpos=None, qvel=None, dofs_idx_local=None, envs_idx=None) -> torch.Tensor:
        """(B, n): tau = M qacc + c(q, qvel) for the acceleration `qacc` (B, n) of this entity's dofs, at `qpos` / `qvel` (B, n) over
        this entity's dofs when given (the way inverse_kinematics takes init_qpos), else at the current state.  The dofs of other
        entities are at zero acceleration and in their current state; passive damping and PD torques are not included.  `qpos` is
        taken for entities with scalar joints only (the robot): for an entity without them (a free cube, whose qpos row is seven wide
        where it has six dofs) it raises NotImplementedError; `qvel` and `qacc` work for every entity.  This package's own name: parity
        with Genesis is unpinned."""
        mir, cols = self._mir, self._jac_dofs()
        idx = _env_index(mir, envs_idx)
        R = mir.num_envs if idx is None else int(idx.numel())
        ct = torch.as_tensor(cols, dtype=torch.long, device=mir.device)

        def entity_rows(t, name):
            t = torch.as_tensor(t, device=mir.device).to(torch.float32).reshape(R, -1)
            if t.shape[1] != len(cols):
                raise ValueError(f"{name} must be ({R}, {len(cols)}) over this entity's dofs, got {tuple(t.shape)}")
            return t

        full_acc = torch.zeros((R, mir.nv), dtype=torch.float32, device=mir.device)
        full_acc[:, ct] = entity_rows(qacc, "qacc")
        kw = dict(qacc=full_acc)
        if qpos is not None or qvel is not None:
            state = mir.get_state()
            if qpos is not None:
                if not self.dof_idx:
                    raise NotImplementedError("inverse_dynamics: qpos override of an entity without scalar joints")
                assert len(self._qcols) == len(cols), "an entity with named dofs has one qpos column per dof"
                full = _rows(state[0], idx).clone()
                full[:, torch.as_tensor(self._qcols, dtype=torch.long, device=mir.device)] = entity_rows(qpos, "qpos")
                kw["qpos"] = full
            if qvel is not None:
                full = _rows(state[1], idx).clone()
                full[:, ct] = entity_rows(qvel, "qvel")
                kw["qvel"] = full
        return self._dynamics(idx, dofs_idx_local, "tau", **kw)

    # ---- operational-space dynamics (MirScene.task_dynamics / mir_task_dynamics): one launch per call, for this entity's dofs, the link
    # and the envs asked for only.  Windows and columns are over the entity's own dofs; `envs_idx` and `qpos` are handled as in
    # inverse_dynamics.  The names are this package's own: parity with Genesis is unpinned (the reference's tasks call none).
    def _entity_rows(self, t, R: int, name: str) -> torch.Tensor:
        n = len(self._jac_dofs())
        t = torch.as_tensor(t, device=self._mir.device).to(torch.float32).reshape(R, -1)
        if t.shape[1] != n:
            raise ValueError(f"{name} must be ({R}, {n}) over this entity's dofs, got {tuple(t.shape)}")
        return t

    def _full_state_rows(self, idx, R: int, qpos=None, qvel=None, who: str = "task_dynamics") -> dict:
        """the entity-wide `qpos` / `qvel` overrides as full rows of the scene state (the other entities in their current state)"""
        mir, kw = self._mir, {}
        if qpos is None and qvel is None:
            return kw
        state = mir.get_state()
        if qpos is not None:
            if not self.dof_idx:
                raise NotImplementedError(f"{who}: qpos override of an entity without scalar joints")
            full = _rows(state[0], idx).clone()
            full[:, torch.as_tensor(self._qcols, dtype=torch.long, device=mir.device)] = self._entity_rows(qpos, R, "qpos")
            kw["qpos"] = full
        if qvel is not None:
            full = _rows(state[1], idx).clone()
            full[:, torch.as_tensor(self._jac_dofs(), dtype=torch.long, device=mir.device)] = self._entity_rows(qvel, R, "qvel")
            kw["qvel"] = full
        return kw

    def _state_rows(self, envs_idx, who: str, qpos=None, qvel=None):
        """-> (the row list or None, R, _full_state_rows() of the overrides): how every query at candidate rows starts"""
        idx = _env_index(self._mir, envs_idx)
        R = self._mir.num_envs if idx is None else int(idx.numel())
        return idx, R, self._full_state_rows(idx, R, qpos=qpos, qvel=qvel, who=who)

    def _task_dynamics(self, idx, **kw) -> dict:
        fn = getattr(self._mir, "task_dynamics", None)
        if fn is None:
            raise NotImplementedError("this scene has no operational-space dynamics (MirScene.task_dynamics / mir_task_dynamics)")
        cols = self._jac_dofs()
        run = bool(cols) and cols == list(range(cols[0], cols[0] + len(cols)))
        win = dict(dof0=cols[0], n_dofs=len(cols)) if run else {}
        out = fn(env_idx=idx, **win, **kw)
        if not run:
            ix = torch.as_tensor(cols, dtype=torch.long, device=self._mir.device)
            if "minv" in out:
                out["minv"] = out["minv"].index_select(1, ix).index_select(2, ix)
            if "solve" in out:
                out["solve"] = out["solve"].index_select(1, ix)
            if "jbar" in out:
                out["jbar"] = out["jbar"].index_select(2, ix)
        return out

    def get_mass_mat_inv(self, envs_idx=None) -> torch.Tensor:
        """(B, n, n): the inverse of get_mass_mat() over this entity's dofs -- the block of M^-1 of its kinematic tree, by a Cholesky
        factorisation on the GPU in the launch that builds M.  Bitwise symmetric."""
        out = self._task_dynamics(_env_index(self._mir, envs_idx), minv=True, lambda_inv=False, lambda_=False, jbar=False)
        return out["minv"].contiguous()

    def mass_mat_solve(self, x, qpos=None, envs_idx=None) -> torch.Tensor:
        """(B, n): M^-1 x for `x` (B, n) over this entity's dofs, at `qpos` (B, n) over this entity's dofs when given, else at the
        current state."""
        mir = self._mir
        idx = _env_index(mir, envs_idx)
        R = mir.num_envs if idx is None else int(idx.numel())
        full = torch.zeros((R, mir.nv), dtype=torch.float32, device=mir.device)
        full[:, torch.as_tensor(self._jac_dofs(), dtype=torch.long, device=mir.device)] = self._entity_rows(x, R, "x")
        kw = self._full_state_rows(idx, R, qpos=qpos, who="mass_mat_solve")
        out = self._task_dynamics(idx, x=full, solve=True, lambda_inv=False, lambda_=False, jbar=False, **kw)
        return out["solve"].contiguous()

    def forward_dynamics(self, tau, qpos=None, qvel=None, envs_idx=None) -> torch.Tensor:
        """(B, n): qacc = M^-1 (tau - c(q, qvel)) for the applied torque `tau` (B, n) over this entity's dofs: the inverse of
        inverse_dynamics.  TWO launches: mir_dynamics for the bias force c, then mir_task_dynamics for the solve.  At `qpos` / `qvel`
        (B, n) over this entity's dofs when given, else at the current state; passive damping, PD torques and contact forces are not
        included (they belong in tau)."""
        idx, R, kw = self._state_rows(envs_idx, "forward_dynamics", qpos=qpos, qvel=qvel)
        bias = self._dynamics(idx, None, "bias", **kw)
        x = self._entity_rows(tau, R, "tau") - bias
        return self.mass_mat_solve(x, qpos=qpos, envs_idx=idx)

    def operational_space(self, link, local_point=None, envs_idx=None, damping: float = 0.0, qpos=None) -> dict:
        """Operational-space dynamics of `link` (a LinkView of this entity or a local link index) at `local_point` (in the link's frame;
        None: its origin), from ONE launch: lambda_inv (B, 6, 6) = J M^-1 J^T, lambda (B, 6, 6) = (J M^-1 J^T + damping^2 I)^-1 and
        jbar (B, n, 6) = M^-1 J^T lambda over this entity's dofs, with J = get_jacobian(link, local_point) (linear rows first, then
        angular).  Where the task space is singular to float32 -- a link with fewer than six dofs above it, an arm at a singularity --
        lambda and jbar of that env are NaN; damping > 0 is the remedy.  lambda_inv is always finite."""
        idx, R, kw = self._state_rows(envs_idx, "operational_space", qpos=qpos)
        lp = None if local_point is None else [float(v) for v in np.asarray(local_point).reshape(3)]
        out = self._task_dynamics(idx, links=[self._link_body(link)], local_points=lp, damping=float(damping), **kw)
        return {"lambda_inv": out["lambda_inv"][:, 0].contiguous(), "lambda": out["lambda"][:, 0].contiguous(), "jbar": out["jbar"][:, 0].contiguous()}

    def get_operational_inertia(self, link, local_point=None, envs_idx=None, damping: float = 0.0, qpos=None) -> torch.Tensor:
        """(B, 6, 6): lambda of operational_space()."""
        return self.operational_space(link, local_point, envs_idx, damping, qpos)["lambda"]

    def get_jacobian_dyn_inverse(self, link, local_point=None, envs_idx=None, damping: float = 0.0, qpos=None) -> torch.Tensor:
        """(B, n, 6): jbar of operational_space(), the dynamically consistent generalised inverse of get_jacobian(link)."""
        return self.operational_space(link, local_point, envs_idx, damping, qpos)["jbar"]

    # ---- clearance (MirScene.signed_distance / mir_signed_distance): the entity as a set of spheres that ride on its links (the
    # sphere model of cuRobo-style planners), the rest of the scene as its exact primitives.  One launch per call.  The names are this
    # package's own: parity with Genesis is unpinned.
    def _covered_links(self) -> list:
        """the links with at least one dof on their path to the world (a base bolted to the floor never moves: it is left out)"""
        bodies, out = self._b.bodies, []
        for b in self.link_idx:
            k, moves = b, False
            while k > 0:
                moves = moves or bodies[k]["jtype"] != 0
                k = bodies[k]["parent"]
            if moves:
                out.append(b)
        return out

    def collision_spheres(self, spacing=None):
        """-> (probes (N, 4) float32: centre in the link's frame and radius, probe_link (N,) int32: body index of the scene), derived
        on the host, deterministically, from the collision geoms of the links that have at least one dof on their path to the world (a
        base bolted to the floor is left out), in geom order.  The spheres of a geom together CONTAIN it:
          sphere:  itself.
          capsule: centres along the axis from end point to end point, both included, at most `spacing` apart (default: half the
                   radius); the radius is sqrt(r^2 + (gap / 2)^2), gap = the distance between neighbouring centres -- the capsule's own
                   radius would leave the surface between two centres uncovered.
          box:     a regular grid of n_x x n_y x n_z equal cells, n_i = ceil(2 h_i / min(2 min(h), spacing)), and one sphere about every
                   cell: its circumscribed sphere, radius = |cell half extents|.
          hull:    the same grid over the bounding box of its vertices in the geom frame; a grid of one cell takes the smaller of
                   that sphere and the bounding sphere of the vertices about the box's centre.
        No radius exceeds the geom's own bounding radius (but for float32 rounding, which every radius is padded for).
        set_collision_spheres() replaces the model."""
        custom = self.__dict__.get("_spheres")
        if custom is not None and spacing is None:
            return custom[0].copy(), custom[1].copy()
        return self._derive_spheres(spacing)[:2]

    def _derive_spheres(self, spacing=None, on_links=None):
        """collision_spheres() from the geoms -> (probes, probe_link, the geom each sphere belongs to); `on_links`: the bodies whose
        geoms are taken instead of the covered links'"""
        from ..backend import spec as S

        covered, probes, links, geoms = set(self._covered_links() if on_links is None else on_links), [], [], []

        def rot(q, v):
            w, u = q[0], np.asarray(q[1:], float)
            t = 2.0 * np.cross(u, v)
            return v + w * t + np.cross(u, t)

        def grid(centre, half, q, cap=np.inf):
            half = np.asarray(half, float)
            edge = 2.0 * half.min() if spacing is None else min(2.0 * half.min(), float(spacing))
            n = np.maximum(1, np.ceil(2.0 * half / edge - 1e-9)).astype(int)
            cell = half / n
            r = float(np.linalg.norm(cell)) if n.max() > 1 else min(float(np.linalg.norm(cell)), cap)
            for i in range(n[0]):
                for j in range(n[1]):
                    for k in range(n[2]):
                        local = -half + cell * (2.0 * np.array([i, j, k]) + 1.0)
                        yield np.append(np.asarray(centre, float) + rot(q, local), r)

        for gi, g in enumerate(self._b.geoms):
            if g["body"] not in covered:
                continue
            pos, q, size, t = np.asarray(g["pos"], float), g["quat"], g["size"], g["type"]
            if t == S.GEOM_SPHERE:
                rows = [np.append(pos, size[0])]
            elif t == S.GEOM_CAPSULE:
                r, hl = float(size[0]), float(size[1])
                gap_max = 0.5 * r if spacing is None else float(spacing)
                n = 1 if hl <= 0.0 else int(np.ceil(2.0 * hl / gap_max - 1e-9)) + 1
                gap = 0.0 if n == 1 else 2.0 * hl / (n - 1)
                rad = float(np.hypot(r, 0.5 * gap))
                rows = [np.append(pos + rot(q, np.array([0.0, 0.0, -hl + gap * i])), rad) for i in range(n)]
            elif t == S.GEOM_BOX:
                rows = list(grid(pos, size, q))
            elif t == S.GEOM_HULL:
                v = np.asarray(self._b.verts[int(size[0]):int(size[0]) + int(size[1])], float)
                lo, hi = v.min(0), v.max(0)
                rows = list(grid(pos + rot(q, 0.5 * (lo + hi)), 0.5 * (hi - lo), q, cap=float(np.linalg.norm(v - 0.5 * (lo + hi), axis=1).max())))
            else:
                continue   # (a plane has no sphere model)
            probes.extend(rows)
            links.extend([g["body"]] * len(rows))
            geoms.extend([gi] * len(rows))
        out = np.asarray(probes, dtype=np.float64).reshape(-1, 4)
        # (the model is float32: every radius grows by what rounding the centre and the radius can take away, 2^-22 relative)
        out[:, 3] += 2.0 ** -22 * (np.abs(out[:, :3]).max(1) + out[:, 3])
        return out.astype(np.float32), np.asarray(links, dtype=np.int32), np.asarray(geoms, dtype=np.int32)

    def set_collision_spheres(self, probes, links) -> None:
        """Replace the sphere model: probes (N, 4) centre in the link's frame and radius, links (N,) body indices of the scene (or
        LinkViews of this entity)."""
        p = np.ascontiguousarray(probes, dtype=np.float32).reshape(-1, 4)
        lk = np.asarray([l.idx if isinstance(l, LinkView) else int(l) for l in links], dtype=np.int32)
        if lk.shape[0] != p.shape[0] or p.shape[0] < 1:
            raise ValueError(f"probes (N, 4) and links (N,) must have the same N >= 1, got {p.shape} and {lk.shape}")
        if any(int(b) not in self.link_idx for b in lk):
            raise ValueError("a sphere rides on a link that does not belong to this entity")
        if not (np.isfinite(p).all() and (p[:, 3] >= 0).all()):
            raise ValueError("sphere centres must be finite and radii >= 0")
        self._spheres = (p, lk)
        self.__dict__.pop("_sphere_model", None)
        self.__dict__.pop("_self_model", None)

    def _own_geoms(self) -> int:
        """bit mask of the geoms on this entity's links (the way sensors.Lidar computes skip_geoms)"""
        mask = 0
        for g, geom in enumerate(self._b.geoms):
            if geom["body"] in self.link_idx:
                mask |= 1 << g
        return mask

    def _skip_mask(self, with_entity=None, ignore_entities=()) -> int:
        """bit mask of the geoms a clearance query leaves out besides the entity's own: all but `with_entity`'s, and `ignore_entities`'"""
        skip = 0 if with_entity is None else ((1 << len(self._b.geoms)) - 1) & ~with_entity._own_geoms()
        for e in ignore_entities:
            skip |= e._own_geoms()
        return skip

    def _clearance_model(self):
        """(probes, links, probes on the device, own geom mask): derived once -- the model on the host, its probes on the device"""
        mir = self._mir
        model = self.__dict__.get("_sphere_model")
        if model is None or model[2].device != mir.device:
            probes, lk = self.collision_spheres()
            if len(lk) == 0:
                raise ValueError("no collision sphere to test (an entity without moving links or without geoms on them)")
            model = self._sphere_model = (probes, lk, torch.as_tensor(probes, device=mir.device), self._own_geoms())
        return model

    def get_clearance(self, qpos=None, envs_idx=None, links=None, with_entity=None, max_distance: float = 1.0, return_detail: bool = False):
        """(R,): the lowest signed distance between this entity's sphere model (collision_spheres(), or what set_collision_spheres()
        put in its place) and every geom that does not belong to the entity itself -- with `with_entity`, only that entity's geoms --
        from ONE launch; negative = penetration depth, max_distance when nothing is that near.  `qpos` (R, n) in this entity's own dof
        order, as inverse_kinematics returns it: the clearance AT that configuration, with the other entities where they are; None: at
        the current state.  `links` (local link indices or LinkViews): only the spheres on those links.  return_detail=True: a dict
        with clearance (R,), sphere (R,) index into the model, link (R,) body index, geom (R,) (-1: nothing within max_distance), closest
        (R, 3) surface point and normal (R, 3) of the minimum.
        The entity's spheres against each other are get_self_clearance()'s question; its spheres against its own geoms are not
        tested.  What lies between two
        configurations is get_path_clearance()'s question -- a clear start and a clear goal say nothing about the path -- and the way
        from one to the other plan_path()'s."""
        mir = self._mir
        fn = getattr(mir, "signed_distance", None)
        if fn is None:
            raise NotImplementedError("this scene has no signed distance (MirScene.signed_distance / mir_signed_distance)")
        probes, lk, dev_probes, own = self._clearance_model()
        sel = None
        if links is not None:
            want = set(self._link_bodies(links))
            sel = np.array([i for i, b in enumerate(lk) if int(b) in want], dtype=np.int64)
            if len(sel) == 0:
                raise ValueError("no collision sphere rides on the links asked for")
            dev_probes, lk = torch.as_tensor(probes[sel], device=mir.device), np.ascontiguousarray(lk[sel])
        idx, R, kw = self._state_rows(envs_idx, "get_clearance", qpos=qpos)
        r = fn(dev_probes, links=lk, env_idx=idx, max_distance=float(max_distance), skip_geoms=own | self._skip_mask(with_entity), geom=return_detail,
               closest=return_detail, normal=return_detail, row_min=True, **kw)
        if not return_detail:
            return r["row_min"]
        arg = r["row_argmin"].long()
        take = lambda t: t.gather(1, arg.view(R, 1, *([1] * (t.dim() - 2))).expand(R, 1, *t.shape[2:]))[:, 0]  # noqa: E731
        sphere = arg if sel is None else torch.as_tensor(sel, device=mir.device)[arg]
        return {"clearance": r["row_min"], "sphere": sphere, "link": torch.as_tensor(lk, device=mir.device).long()[arg],
                "geom": take(r["geom"]), "closest": take(r["closest"]), "normal": take(r["normal"])}

    def in_collision(self, qpos=None, envs_idx=None, margin: float = 0.0, links=None, with_entity=None) -> torch.Tensor:
        """(R,) bool: get_clearance(...) < margin -- the sphere model touches or penetrates something (margin = 0), or comes nearer than
        `margin`.  The scene only: in_self_collision() tests the sphere model against itself."""
        return self.get_clearance(qpos=qpos, envs_idx=envs_idx, links=links, with_entity=with_entity, max_distance=max(1.0, 2.0 * float(margin))) < float(margin)

    # ---- self-collision (MirScene.self_distance / mir_self_distance): the sphere model against itself.  A pair of links is tested
    # unless it is the same link, parent and child, or already overlapping at the neutral configuration (Genesis's
    # enable_neutral_collision=False rule).  What stays out: link geoms other than through spheres.  A carried object against the arm
    # is the attached_entity= argument of plan_path() / get_path_clearance() / get_carried_clearance().
    def _neutral_poses(self, neutral_qpos=None) -> dict:
        """float64 forward kinematics of this entity's links at `neutral_qpos` ((n,) in the entity's dof order; None: zero clipped into
        the joint limits) -> ({body: (position, quaternion)} relative to the root's parent, the rotation q, v -> q v q*)"""
        dofs, first, nd = self._b.dofs, {}, {0: 0, 1: 1, 2: 1, 3: 6}
        k = 0
        for i, b in enumerate(self._b.bodies):
            first[i] = k
            k += nd[b["jtype"]] if i > 0 else 0
        q = np.zeros(len(self.dof_idx)) if neutral_qpos is None else np.asarray(neutral_qpos, float).reshape(-1)
        if q.shape[0] != len(self.dof_idx):
            raise ValueError(f"neutral_qpos must be ({len(self.dof_idx)},), got {q.shape}")

        def value(d):
            v = q[self.dof_idx.index(d)] if d in self.dof_idx else 0.0
            return float(np.clip(v, *dofs[d]["range"])) if neutral_qpos is None and dofs[d]["limited"] else float(v)

        def qmul(a, b):
            return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                             a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])

        def qrot(a, v):
            t = 2.0 * np.cross(a[1:], v)
            return v + a[0] * t + np.cross(a[1:], t)

        poses = {}
        for b in self.link_idx:   # (body order: a parent comes before its children)
            body = self._b.bodies[b]
            P, Q, ax = np.asarray(body["pos"], float), np.asarray(body["quat"], float), np.asarray(body["axis"], float)
            if body["jtype"] == 1:
                h = 0.5 * value(first[b])
                Q = qmul(Q, np.append(np.cos(h), ax * np.sin(h)))
            elif body["jtype"] == 2:
                P = P + qrot(Q, value(first[b]) * ax)
            if b != self.root and body["jtype"] != 3:
                pp, pq = poses[body["parent"]]
                P, Q = pp + qrot(pq, P), qmul(pq, Q)
            poses[b] = (P, Q)
        return poses, qrot

    def self_collision_model(self, neutral_qpos=None, spacing=None):
        """-> (probes (N + E, 4) float32, probe_link (N + E,) int32, n_extra = E, link_mask (32,) uint32): what the self test reads.
        The first N spheres are collision_spheres() unchanged.  The E extra spheres are derived by the same rules (at `spacing`) from
        the geoms of the entity's links that collision_spheres() leaves out -- a base bolted to the floor -- and take part in the self
        test only: a base sphere sits in the floor by construction.  link_mask[a] bit b: the spheres on body a are tested against
        those on body b; symmetric, zero diagonal.  Set for every pair of the entity's links that carry spheres except the same link,
        parent and child, and every pair whose spheres overlap (lowest |ci - cj| - ri - rj < 0, float64) at `neutral_qpos` ((n,) in
        this entity's dof order; None: the zero configuration clipped into the joint limits) -- Genesis's
        enable_neutral_collision=False rule.  set_self_collision_pairs() edits the mask.  The model is derived once and kept; a call
        with `neutral_qpos` or `spacing` derives it again, and set_collision_spheres() drops it."""
        model = self.__dict__.get("_self_model")
        if model is None or neutral_qpos is not None or spacing is not None:
            probes, lk = self.collision_spheres()
            rest = [b for b in self.link_idx if b not in set(self._covered_links())]
            xp, xl, _ = self._derive_spheres(spacing, on_links=rest)
            allp, alll = np.concatenate([probes, xp]).astype(np.float32), np.concatenate([lk, xl]).astype(np.int32)
            poses, qrot = self._neutral_poses(neutral_qpos)
            centre = np.stack([poses[int(b)][0] + qrot(poses[int(b)][1], c[:3].astype(float)) for c, b in zip(allp, alll)]) if len(alll) else np.zeros((0, 3))
            radius = allp[:, 3].astype(float)
            mask = np.zeros(32, np.uint32)
            on = sorted(set(int(b) for b in alll))
            for a in on:
                for b in on:
                    if a >= b or self._b.bodies[b]["parent"] == a or self._b.bodies[a]["parent"] == b:
                        continue
                    ia, ib = np.flatnonzero(alll == a), np.flatnonzero(alll == b)
                    gap = np.linalg.norm(centre[ia][:, None] - centre[ib][None], axis=2) - radius[ia][:, None] - radius[ib][None]
                    if gap.min() < 0.0:
                        continue   # (already touching at the neutral configuration: the model's own coarseness, not a collision)
                    mask[a] |= np.uint32(1 << b)
                    mask[b] |= np.uint32(1 << a)
            model = self._self_model = (allp, alll, int(len(xl)), mask)
            self.__dict__.pop("_self_dev", None)
        return model[0].copy(), model[1].copy(), model[2], model[3].copy()

    def set_self_collision_pairs(self, pairs=None, disable=()) -> None:
        """Edit the pair filter of the self test.  `pairs`: the link pairs that are tested, replacing the derived set (None: keep it);
        `disable`: pairs taken out.  A link is a name, a LinkView of this entity or a local link index."""
        self.self_collision_model()
        probes, lk, n_extra, mask = self._self_model

        def body(l):
            return self._b.body_index(l) if isinstance(l, str) else self._link_body(l)

        def put(m, a, b, on):
            a, b = body(a), body(b)
            if a == b or a not in self.link_idx or b not in self.link_idx:
                raise ValueError("a self-collision pair names two different links of this entity")
            for x, y in ((a, b), (b, a)):
                m[x] = (int(m[x]) | (1 << y)) if on else (int(m[x]) & ~(1 << y))

        mask = mask.copy()
        if pairs is not None:
            mask[:] = 0
            for a, b in pairs:
                put(mask, a, b, True)
        for a, b in disable:
            put(mask, a, b, False)
        self._self_model = (probes, lk, n_extra, mask)

    def self_collision_pairs(self) -> list:
        """the link pairs the self test covers, as local link indices (a, b) with a < b: what set_self_collision_pairs(pairs=...) takes"""
        mask, lk = self.self_collision_model()[3], self.link_idx
        return [(i, j) for i in range(len(lk)) for j in range(i + 1, len(lk)) if (int(mask[lk[i]]) >> lk[j]) & 1]

    def _self_args(self, self_margin=0.0, max_distance=1.0):
        """the self model as MirScene takes it: (probes on the device, links, dict for self_model=)"""
        if not (np.isfinite(self_margin) and self_margin >= 0.0):
            raise ValueError(f"self_margin must be finite and >= 0, got {self_margin}")
        self.self_collision_model()
        probes, lk, n_extra, mask = self._self_model
        if len(lk) - n_extra < 1:
            raise ValueError("no collision sphere to test (an entity without moving links or without geoms on them)")
        dev = self.__dict__.get("_self_dev")
        if dev is None or dev.device != self._mir.device:
            dev = self._self_dev = torch.as_tensor(probes, device=self._mir.device)
        return dev, lk, dict(link_mask=mask, n_extra=n_extra, self_margin=float(self_margin), max_distance=max(float(max_distance), 2.0 * float(self_margin)))

    def get_self_clearance(self, qpos=None, envs_idx=None, max_distance: float = 1.0, return_detail: bool = False):
        """(R,): the lowest signed distance |ci - cj| - ri - rj between two spheres of this entity's self model
        (self_collision_model()) that ride on a pair of links the filter enables, from ONE launch (MirScene.self_distance /
        mir_self_distance); negative = the spheres overlap by that much, max_distance when no pair is that near.  `qpos` (R, n) in this
        entity's own dof order: AT that configuration; None: at the current state.  return_detail=True: a dict with clearance (R,),
        spheres (R, 2) indices into the self model (-1: none) and links (R, 2) their body indices (-1: none)."""
        mir = self._mir
        fn = getattr(mir, "self_distance", None)
        if fn is None:
            raise NotImplementedError("this scene has no self-collision queries (MirScene.self_distance / mir_self_distance)")
        dev, lk, sm = self._self_args(0.0, max_distance)
        idx, R, kw = self._state_rows(envs_idx, "get_self_clearance", qpos=qpos)
        r = fn(dev, links=lk, link_mask=sm["link_mask"], env_idx=idx, max_distance=float(max_distance), n_extra=sm["n_extra"], row_min=True, **kw)
        if not return_detail:
            return r["row_min"]
        pair = r["row_pair"].long()
        links = torch.as_tensor(lk, device=mir.device).long()[pair.clamp(min=0)]
        return {"clearance": r["row_min"], "spheres": pair, "links": torch.where(pair >= 0, links, torch.full_like(links, -1))}

    def in_self_collision(self, qpos=None, envs_idx=None, margin: float = 0.0) -> torch.Tensor:
        """(R,) bool: get_self_clearance(...) < margin -- two spheres of the self model on an enabled pair of links touch or overlap
        (margin = 0), or come nearer than `margin`."""
        return self.get_self_clearance(qpos=qpos, envs_idx=envs_idx, max_distance=max(1.0, 2.0 * float(margin))) < float(margin)

    def _self_on(self, self_collision) -> bool:
        """self_collision=None follows the scene's enable_self_collision option"""
        return bool(self._b.opt.get("enable_self_collision", 0)) if self_collision is None else bool(self_collision)

    # ---- motion planning (MirScene.plan_path / path_clearance: mir_plan_path, mir_path_clearance).  The planner is this package's own
    # (RRT-Connect on the GPU, one wave per env, deterministic in `seed`): parity with Genesis (OMPL) is unpinned.
    def attached_links_default(self, ee_link_name) -> list:
        """the links (body indices) a carried object attached to `ee_link_name` is tested against by default: every link of this
        entity that carries spheres of the self model, except the attach link, its descendants (the fingers) and every link joined to
        the attach link through fixed joints only"""
        bodies, at = self._b.bodies, self._attach_body(ee_link_name)
        out_of, grew = {at}, True
        while grew:   # (links joined to the attach link through fixed joints only, up and down)
            grew = False
            for b in self.link_idx:
                par = bodies[b]["parent"]
                if bodies[b]["jtype"] == 0 and par in self.link_idx and (b in out_of) != (par in out_of):
                    out_of.update((b, par))
                    grew = True
        below = {at}
        for b in self.link_idx:   # (body order: a parent comes before its children)
            if bodies[b]["parent"] in below:
                below.add(b)
        out_of |= below
        lk = self.self_collision_model()[1]
        return [b for b in sorted(set(int(x) for x in lk)) if b not in out_of]

    def _attach_body(self, ee_link_name) -> int:
        if ee_link_name is None:
            raise ValueError("attached_entity needs ee_link_name: the link of this entity the object is attached to")
        b = ee_link_name.idx if isinstance(ee_link_name, LinkView) else self._b.body_index(ee_link_name)
        if b not in self.link_idx:
            raise ValueError(f"ee_link_name {ee_link_name!r} is not a link of this entity")
        return b

    def carried_model(self, attached_entity, ee_link_name, attached_links=None, self_collision=None):
        """-> (probes (N + E, 4) float32, probe_link (N + E,) int32, n_extra = E, link_mask (32,) uint32, C, Lk): what plan_path() hands
        to mir_plan_path_carry for `attached_entity` on `ee_link_name`, composed on the host.  The object's spheres (its own
        collision_spheres(), or what set_collision_spheres() put in their place; they ride on its body C) stand behind the arm's inside
        the first N, the E self-only spheres of self_collision_model() behind them.  link_mask: the arm-against-arm filter when
        `self_collision` is on (None: the scene's option), else zero, plus bit b of word C and bit C of word b for every link b of
        `attached_links` (names, LinkViews or local link indices; None: attached_links_default(); []: none).  Lk: the attach link."""
        if not isinstance(attached_entity, EntityView) or len(attached_entity.link_idx) != 1 or self._b.bodies[attached_entity.root]["jtype"] != 3:
            raise ValueError("attached_entity must be an EntityView of one free body (a cube), not an articulated or a fixed entity")
        C, at = attached_entity.root, self._attach_body(ee_link_name)
        against = self.attached_links_default(ee_link_name) if attached_links is None else [
            self._b.body_index(l) if isinstance(l, str) else self._link_body(l) for l in attached_links]
        if any(b not in self.link_idx for b in against):
            raise ValueError("attached_links names a link that does not belong to this entity")
        cp, cl = attached_entity.collision_spheres()
        if len(cl) == 0:
            raise ValueError("attached_entity has no collision sphere")
        self.self_collision_model()
        probes, lk, n_extra, mask = self._self_model
        N = len(lk) - n_extra
        m = mask.copy() if self._self_on(self_collision) else np.zeros(32, np.uint32)
        for b in against:
            m[C] |= np.uint32(1 << b)
            m[b] |= np.uint32(1 << C)
        return (np.concatenate([probes[:N], cp, probes[N:]]).astype(np.float32), np.concatenate([lk[:N], cl, lk[N:]]).astype(np.int32), n_extra, m,
                C, at)

    def _carry_args(self, args, R, attached_entity, ee_link_name, grasp_pose, attached_links, self_collision, self_margin):
        """the carried object composed into the arguments of MirScene.plan_path / path_clearance: carried_model() on the device (kept
        until one of its inputs changes), the object's geoms skipped, carry=dict(body, link, grasp)"""
        allp, alll, n_extra, m, C, at = self.carried_model(attached_entity, ee_link_name, attached_links, self_collision)
        grasp = None
        if grasp_pose is not None:
            grasp = torch.as_tensor(grasp_pose, device=self._mir.device).to(torch.float32)
            if grasp.dim() == 1 and grasp.shape[0] == 7:
                grasp = grasp[None].expand(R, 7)
            if tuple(grasp.shape) != (R, 7):
                raise ValueError(f"grasp_pose must be ({R}, 7) or (7,): position xyz and quaternion wxyz in the link's frame, got {tuple(grasp.shape)}")
            grasp = grasp.contiguous()
        kept = self.__dict__.get("_carry_dev")
        if kept is None or kept[1].device != self._mir.device or kept[0] != allp.tobytes():
            kept = self._carry_dev = (allp.tobytes(), torch.as_tensor(allp, device=self._mir.device))
        args.update(probes=kept[1], links=alll, carry=dict(body=C, link=at, grasp=grasp),
                    self_model=dict(link_mask=m, n_extra=n_extra, self_margin=float(self_margin), max_distance=max(1.0, 2.0 * float(self_margin))))
        args["skip_geoms"] |= attached_entity._own_geoms()
        return args

    def _plan_args(self, envs_idx, qpos_start, with_entity, ignore_entities, who, self_collision=None, self_margin=0.0, attached_entity=None,
                   ee_link_name=None, grasp_pose=None, attached_links=None):
        self._need("plan_path", "motion planning")
        if not self.dof_idx:
            raise NotImplementedError(f"{who}: an entity without scalar joints")
        _, lk, dev_probes, own = self._clearance_model()
        extra = {}
        if self._self_on(self_collision):
            self._need("self_distance", "self-collision queries")
            dev_probes, lk, extra["self_model"] = self._self_args(self_margin)
        idx, R, kw = self._state_rows(envs_idx, who, qpos=qpos_start)
        args = dict(probes=dev_probes, links=lk, dof_qadr=self._qcols, env_idx=idx, qpos_start=kw.get("qpos"),
                    skip_geoms=own | self._skip_mask(with_entity, ignore_entities), **extra)
        if attached_entity is not None:
            if not (np.isfinite(self_margin) and self_margin >= 0.0):
                raise ValueError(f"self_margin must be finite and >= 0, got {self_margin}")
            args = self._carry_args(args, R, attached_entity, ee_link_name, grasp_pose, attached_links, self_collision, self_margin)
        elif ee_link_name is not None or grasp_pose is not None or attached_links is not None:
            raise ValueError(f"{who}: ee_link_name, grasp_pose and attached_links belong to attached_entity, which is None")
        return args, R

    def _need(self, method: str, what: str) -> None:
        """refuses a scene whose backend has no MirScene.<method>"""
        if getattr(self._mir, method, None) is None:
            raise NotImplementedError(f"this scene has no {what} (MirScene.{method} / mir_{method})")

    def _plan_args_grasp_at_start(self, who, entry, grasp_pose, envs_idx, qpos_start, with_entity, ignore_entities, self_collision, self_margin,
                                  attached_entity, ee_link_name, attached_links):
        """_plan_args() for a method whose entry point has no grasp rows: `grasp_pose` is refused, carry = dict(body, link) alone"""
        if grasp_pose is not None:
            raise NotImplementedError(f"{who}: the grasp is taken from where the attached entity is at the start ({entry} has no grasp rows); "
                                      "grasp_pose must be None")
        args, R = self._plan_args(envs_idx, qpos_start, with_entity, ignore_entities, who, self_collision, self_margin, attached_entity, ee_link_name,
                                  None, attached_links)
        if "carry" in args:
            args["carry"] = dict(body=args["carry"]["body"], link=args["carry"]["link"])
        return args, R

    def _path_rows(self, path, R: int, kmin: int, name: str, axis: int, letter: str = "K") -> torch.Tensor:
        """`path` as float32 device rows (R, K, n), K >= kmin.  axis: where its K stands -- 0: (K, R, n), the layout plan_path() returns;
        1: (R, K, n), blend_path's poly.  An unbatched task may leave the env axis out."""
        n = len(self._qcols)
        p = torch.as_tensor(path, device=self._mir.device).to(torch.float32)
        if self.__dict__.get("unbatched") and p.dim() == 2:
            p = p.unsqueeze(1 - axis)
        if p.dim() != 3 or p.shape[1 - axis] != R or p.shape[2] != n or p.shape[axis] < kmin:
            k = f"{letter} >= {kmin}" if kmin > 0 else letter
            raise ValueError(f"{name} must be ({f'{R}, {k}' if axis else f'{k}, {R}'}, {n}), got {tuple(p.shape)}")
        return (p if axis else p.permute(1, 0, 2)).contiguous()

    def _drop_env_axis(self, detail: dict, axis1=("path",)) -> dict:
        """on an unbatched task (no env axis anywhere): every entry of `detail` without it -- axis 1 of those named in `axis1`, axis 0 of the
        others"""
        if not self.__dict__.get("unbatched"):
            return detail
        return {k: (v[:, 0] if k in axis1 else v[0]) for k, v in detail.items()}

    def plan_path(self, qpos_goal, qpos_start=None, timeout=None, smooth_path=True, num_waypoints=100, ignore_collision=False,
                  planner="RRTConnect", envs_idx=None, return_valid_mask=False, resolution=0.05, step=0.3, margin=0.0, max_nodes=256,
                  max_iterations=2000, seed=0, with_entity=None, ignore_entities=(), return_detail=False, self_collision=None, self_margin=0.0,
                  attached_entity=None, ee_link_name=None, grasp_pose=None, attached_links=None):
        """``robot.plan_path(qpos_goal=q_goal, num_waypoints=100)`` -> (W, R, n): waypoints in this entity's own dof order (what
        inverse_kinematics returns and control_dofs_position takes) from `qpos_start` ((R, n); None: the current state) to `qpos_goal`
        (R, n), through configurations at which the entity's sphere model (collision_spheres()) keeps `margin` from every geom that
        does not belong to the entity -- with `with_entity`, only that entity's geoms; the geoms of `ignore_entities` (a cube in the
        fingers, the cube the hand reaches for) are left out too.  ONE launch for all rows (MirScene.plan_path / mir_plan_path, where
        the algorithm is written down: RRT-Connect with `step`, edges checked every `resolution` rad / m per joint, at most `max_nodes`
        per tree and `max_iterations` samples, 64 shortcut attempts when `smooth_path`, resampled at equal arc length).  Deterministic in
        `seed`; a row's plan does not depend on the other rows.  A row without a plan holds its start W times (the arm stays put):
        return_valid_mask=True -> (path, valid (R,) bool); return_detail=True -> a dict with path, valid, status (R,) int32
        (spec.PLAN_STATUS), poly (R, 128, n) the polyline behind the waypoints, n_poly (R,) and stats (R, 4).  On an unbatched task
        (num_envs = 0) every result comes without its env axis: path (W, n), valid a scalar.
        `timeout` is accepted and ignored: the budget is `max_iterations`, which is deterministic.  Only planner="RRTConnect".
        `self_collision` (None: the scene's enable_self_collision option): a configuration must also keep `self_margin` between the
        spheres of the self model (self_collision_model(): the sphere model plus the spheres of a bolted base, link pairs filtered by
        the neutral rule); status 7 / 8 = the start / the goal is in self-collision (mir_plan_path_self).
        `attached_entity` (an EntityView of one free body, the cube in the fingers) with `ee_link_name` (the link of this entity it is
        attached to): the object is planned for (mir_plan_path_carry).  Genesis calls the attached object `with_entity`; here
        `with_entity` keeps its meaning above.  The object's spheres (its own collision_spheres(), or what set_collision_spheres() put
        in their place) follow the link by a rigid grasp transform per row -- `grasp_pose` (R, 7) or (7,): the object's position xyz
        and quaternion wxyz in the link's frame; None: taken on the device from where the object is at the start -- and are tested
        against the scene like the arm's and, at `self_margin`, against the spheres of `attached_links` (names, LinkViews or local
        link indices; None: attached_links_default(), every sphere-carrying link but the attach link, its descendants and what is
        fixed to it; []: not against the arm), whether or not `self_collision` (arm against arm) is on.  The object's own geoms are
        left out of the scene test.  return_detail gains grasp (R, 7): the transform each row used.
        The planner is this package's own, not OMPL's: parity with Genesis is unpinned.  The other entities stay where they are, and
        only the sphere model stands for the entity and for what it carries."""
        if planner != "RRTConnect":
            raise NotImplementedError(f"planner {planner!r}: only 'RRTConnect' is implemented")
        args, R = self._plan_args(envs_idx, qpos_start, with_entity, ignore_entities, "plan_path", self_collision, self_margin, attached_entity,
                                  ee_link_name, grasp_pose, attached_links)
        goal = self._entity_rows(qpos_goal, R, "qpos_goal")
        r = self._mir.plan_path(qpos_goal=goal, num_waypoints=int(num_waypoints), max_nodes=int(max_nodes), max_iterations=int(max_iterations),
                                smooth_passes=64 if smooth_path else 0, ignore_collision=bool(ignore_collision), seed=int(seed),
                                resolution=float(resolution), step=float(step), margin=float(margin), max_distance=max(1.0, 2.0 * float(margin)), **args)
        detail = {"path": r["path"].permute(1, 0, 2).contiguous(), "valid": r["status"] == 0, "status": r["status"], "poly": r["poly"],
                  "n_poly": r["n_poly"], "stats": r["stats"]}
        if "grasp" in r:
            detail["grasp"] = r["grasp"]
        detail = self._drop_env_axis(detail)
        if return_detail:
            return detail
        return (detail["path"], detail["valid"]) if return_valid_mask else detail["path"]

    def plan_path_to_goals(self, qpos_goals, n_goals=None, qpos_start=None, timeout=None, smooth_path=True, num_waypoints=100,
                           ignore_collision=False, planner="RRTConnect", envs_idx=None, return_valid_mask=False, resolution=0.05, step=0.3,
                           margin=0.0, max_nodes=256, max_iterations=2000, seed=0, with_entity=None, ignore_entities=(), return_detail=False,
                           self_collision=None, self_margin=0.0, attached_entity=None, ee_link_name=None, grasp_pose=None, attached_links=None):
        """``robot.plan_path_to_goals(qpos_goals=[q_a, q_b])`` -> (W, R, n): plan_path() to whichever of several goal configurations can be
        reached -- two grasp approaches, the symmetric grasps of a cube, several inverse-kinematics solutions of one pose.  `qpos_goals`
        (G, R, n), G = 1 .. 8, in the layout of a stack of plan_path() goals ((G, n) on an unbatched task); `n_goals` (R,): how many
        of a row's goals count (None: all G; the entries behind a row's count are never read).  ONE launch (MirScene.plan_path_goals /
        mir_plan_path_goals, where the rule is written down): every goal is judged like plan_path()'s; the straight edge is tried to the
        valid ones, nearest to the start first; otherwise RRT-Connect grows its goal tree from all valid goals at once and the plan ends at
        the goal the trees meet through.  A row without a valid goal has status 9 (NO_VALID_GOAL; spec.PLAN_GOAL_STATUS) and, like every row without a plan,
        holds its start W times.  Every other keyword means what it means in plan_path(), and the result has plan_path()'s layout;
        return_detail gains goal_index (R,): the goal the plan ends at (-1: no plan) and goal_status (R, G): spec.PLAN_STATUS per goal,
        -1 where a goal was not judged.  With one valid goal the result is plan_path()'s bit for bit.
        NOTE: a row status of this method can be 9, which spec.PLAN_STATUS (nine names, as it always had) does not hold: name row
        statuses with spec.PLAN_GOAL_STATUS[status]; goal_status entries are 0 .. 8 and spec.PLAN_STATUS names them."""
        if planner != "RRTConnect":
            raise NotImplementedError(f"planner {planner!r}: only 'RRTConnect' is implemented")
        args, R = self._plan_args(envs_idx, qpos_start, with_entity, ignore_entities, "plan_path_to_goals", self_collision, self_margin, attached_entity,
                                  ee_link_name, grasp_pose, attached_links)
        goals = self._path_rows(qpos_goals, R, 1, "qpos_goals", 0, "G")
        if n_goals is not None:
            n_goals = torch.as_tensor(n_goals, device=self._mir.device).to(torch.int32).reshape(-1)
        r = self._mir.plan_path_goals(qpos_goals=goals, n_goals=n_goals, num_waypoints=int(num_waypoints), max_nodes=int(max_nodes),
                                      max_iterations=int(max_iterations), smooth_passes=64 if smooth_path else 0,
                                      ignore_collision=bool(ignore_collision), seed=int(seed), resolution=float(resolution), step=float(step),
                                      margin=float(margin), max_distance=max(1.0, 2.0 * float(margin)), **args)
        detail = {"path": r["path"].permute(1, 0, 2).contiguous(), "valid": r["status"] == 0, "status": r["status"], "poly": r["poly"],
                  "n_poly": r["n_poly"], "stats": r["stats"], "goal_index": r["goal_index"], "goal_status": r["goal_status"]}
        if "grasp" in r:
            detail["grasp"] = r["grasp"]
        detail = self._drop_env_axis(detail)
        if return_detail:
            return detail
        return (detail["path"], detail["valid"]) if return_valid_mask else detail["path"]

    def plan_path_to_pose(self, link, pos, quat=None, max_goals=4, max_samples=16, dedup=None, qpos_start=None, timeout=None, smooth_path=True,
                          num_waypoints=100, ignore_collision=False, planner="RRTConnect", envs_idx=None, return_valid_mask=False,
                          resolution=0.05, step=0.3, margin=0.0, max_nodes=256, max_iterations=2000, seed=0, with_entity=None,
                          ignore_entities=(), return_detail=False, self_collision=None, self_margin=0.0, attached_entity=None,
                          ee_link_name=None, grasp_pose=None, attached_links=None, **ik_options):
        """``robot.plan_path_to_pose(hand, pos=(R, 3), quat=(R, 4))`` -> (W, R, n): plan_path() to a POSE of `link` (a LinkView or a local
        link index) instead of a goal configuration -- above the cube, at the cube, over the stack -- in ONE launch
        (MirScene.plan_path_pose / mir_plan_path_pose, where the rule is written down).  The row's wave solves the inverse kinematics of
        the pose from up to `max_samples` seeds (the start configuration, then random draws inside the joint limits; `ik_options`:
        those of inverse_kinematics), keeps up to `max_goals` (<= 8) solutions that converged, lie inside the limits, are clear by the
        collision tests of the call and differ from one another by `dedup` (None: `resolution`) in some joint, and runs the goal-set
        planner of plan_path_to_goals() on them: nothing is decided on the host between the pose and the plan.  `quat` (R, 4) wxyz or
        one quaternion for all; None: position only.  Dofs of the entity that are not on the chain to `link` (the fingers) keep their
        start value.  Every other keyword means what it means in plan_path(); the result has plan_path()'s layout.  A row that keeps
        no goal has status 9 (NO_VALID_GOAL; name row statuses with spec.PLAN_GOAL_STATUS, not spec.PLAN_STATUS), a target that is not
        finite 17 (spec.CART_STATUS: NOT_FINITE).  return_detail gains goal_index (R,), goal_status (R, G), goals (R, G, n): the kept
        configurations, n_goals (R,) and goal_stats (R, 4): samples tried, converged, converged but rejected, IK iterations --
        converged = 0 tells "unreachable" from "every solution collides"."""
        if planner != "RRTConnect":
            raise NotImplementedError(f"planner {planner!r}: only 'RRTConnect' is implemented")
        args, R = self._plan_args(envs_idx, qpos_start, with_entity, ignore_entities, "plan_path_to_pose", self_collision, self_margin, attached_entity,
                                  ee_link_name, grasp_pose, attached_links)
        self._need("plan_path_pose", "pose goals")
        dev = self._mir.device
        p = torch.as_tensor(pos, device=dev).to(torch.float32)
        p = p.reshape(1, 3).expand(R, 3) if p.numel() == 3 else p
        if tuple(p.shape) != (R, 3):
            raise ValueError(f"pos must be ({R}, 3), got {tuple(p.shape)}")
        q = None
        if quat is not None:
            q = torch.as_tensor(quat, device=dev).to(torch.float32)
            q = q.reshape(1, 4).expand(R, 4) if q.numel() == 4 else q
            if tuple(q.shape) != (R, 4):
                raise ValueError(f"quat must be ({R}, 4) or (4,), got {tuple(q.shape)}")
            q = q.contiguous()
        r = self._mir.plan_path_pose(link_body=self._link_body(link), target_pos=p.contiguous(), target_quat=q, max_goals=int(max_goals),
                                     max_samples=int(max_samples), dedup=0.0 if dedup is None else float(dedup), num_waypoints=int(num_waypoints),
                                     max_nodes=int(max_nodes), max_iterations=int(max_iterations), smooth_passes=64 if smooth_path else 0,
                                     ignore_collision=bool(ignore_collision), seed=int(seed), resolution=float(resolution), step=float(step),
                                     margin=float(margin), max_distance=max(1.0, 2.0 * float(margin)), **args, **ik_options)
        detail = {"path": r["path"].permute(1, 0, 2).contiguous(), "valid": r["status"] == 0, "status": r["status"], "poly": r["poly"],
                  "n_poly": r["n_poly"], "stats": r["stats"], "goal_index": r["goal_index"], "goal_status": r["goal_status"], "goals": r["goals"],
                  "n_goals": r["n_goals"], "goal_stats": r["goal_stats"]}
        if "grasp" in r:
            detail["grasp"] = r["grasp"]
        detail = self._drop_env_axis(detail)
        if return_detail:
            return detail
        return (detail["path"], detail["valid"]) if return_valid_mask else detail["path"]

    def get_path_clearance(self, path, envs_idx=None, qpos_start=None, resolution=0.05, margin=0.0, with_entity=None, ignore_entities=(),
                           max_distance: float = 1.0, return_detail: bool = False, self_collision=None, self_margin=0.0, attached_entity=None,
                           ee_link_name=None, grasp_pose=None, attached_links=None):
        """(R,): the lowest clearance of this entity's sphere model along the trajectory `path` ((K, R, n) as plan_path returns it, K >= 2)
        -- at every waypoint and at the configurations between two of them, at most `resolution` apart in every joint -- from ONE launch
        (MirScene.path_clearance / mir_path_clearance).  The other dofs of the scene are those of `qpos_start` ((R, n) for this entity;
        None: the current state).  return_detail=True: a dict with clearance (R,), seg_min (R, K-1) per segment and first_blocked (R,):
        the first segment that comes nearer than `margin`, -1: none.
        `self_collision` (None: the scene's enable_self_collision option) adds the self test of plan_path() on the same samples
        (mir_path_clearance_self): the detail gains self_clearance (R,) and self_seg_min (R, K-1), first_blocked counts either test, and
        without detail the result is min(clearance - margin, self_clearance - self_margin) + margin, so that "< margin" asks both.
        `attached_entity`, `ee_link_name`, `grasp_pose`, `attached_links`: the carried object of plan_path() (Genesis names it
        `with_entity`) on the same samples (mir_path_clearance_carry): its spheres count in clearance, and against the arm in
        self_clearance, which is then reported whether or not `self_collision` is on; the detail gains grasp (R, 7)."""
        args, R = self._plan_args(envs_idx, qpos_start, with_entity, ignore_entities, "get_path_clearance", self_collision, self_margin,
                                  attached_entity, ee_link_name, grasp_pose, attached_links)
        r = self._mir.path_clearance(paths=self._path_rows(path, R, 2, "path", 0), resolution=float(resolution), margin=float(margin),
                                     max_distance=max(float(max_distance), 2.0 * float(margin)), **args)
        out = {"clearance": r["row_min"], "seg_min": r["seg_min"], "first_blocked": r["row_first_blocked"]}
        if "self_model" in args:
            out["self_clearance"], out["self_seg_min"] = r["row_self_min"], r["seg_self_min"]
        if "grasp" in r:
            out["grasp"] = r["grasp"]
        out = self._drop_env_axis(out, ())
        if return_detail or "self_model" not in args:
            return out if return_detail else out["clearance"]
        return torch.minimum(out["clearance"] - float(margin), out["self_clearance"] - float(self_margin)) + float(margin)

    def path_in_collision(self, path, margin: float = 0.0, envs_idx=None, qpos_start=None, resolution=0.05, with_entity=None,
                          ignore_entities=(), self_collision=None, self_margin=0.0, attached_entity=None, ee_link_name=None, grasp_pose=None,
                          attached_links=None) -> torch.Tensor:
        """(R,) bool: get_path_clearance(path, ...) < margin -- somewhere along the trajectory the sphere model touches or penetrates
        something (margin = 0) or comes nearer than `margin`; with `self_collision`, or itself nearer than `self_margin`; with
        `attached_entity` (the carried object of plan_path(), which Genesis names `with_entity`), the object's spheres count in both."""
        return self.get_path_clearance(path, envs_idx=envs_idx, qpos_start=qpos_start, resolution=resolution, margin=margin, with_entity=with_entity,
                                       ignore_entities=ignore_entities, max_distance=max(1.0, 2.0 * float(margin)), self_collision=self_collision,
                                       self_margin=self_margin, attached_entity=attached_entity, ee_link_name=ee_link_name, grasp_pose=grasp_pose,
                                       attached_links=attached_links) < float(margin)

    # ---- certified clearance (MirScene.certify_path / mir_certify_path): the question get_path_clearance answers for samples, answered for
    # the whole of every segment.  The names and the arguments are this package's own: parity with Genesis is unpinned.
    def certify_path(self, path, margin=0.0, tol=0.002, guard=1e-5, max_depth=12, max_evaluations=4096, bracket=False, max_leaves=0,
                     max_distance=1.0, envs_idx=None, qpos_start=None, with_entity=None, ignore_entities=(), return_detail=False,
                     self_collision=False, attached_entity=None):
        """``robot.certify_path(path)`` -> (R,) int32, spec.CERT_STATUS by severity: 0 CLEAR -- the entity's sphere model keeps `margin`
        from every tested geom along the WHOLE trajectory `path` ((K, R, n) as plan_path returns it and get_path_clearance accepts it,
        K >= 2), not only at samples of it -- 1 UNDECIDED (the minimum is bracketed within `tol` and the bracket straddles the margin),
        2 DEPTH, 3 BUDGET (`max_depth`, `max_evaluations` per row ran out), 4 BLOCKED (a configuration below the margin was found),
        5 NOT_FINITE.  ONE launch for all rows (MirScene.certify_path / mir_certify_path, where the rule and the argument are written
        down).  `bracket`: close the bracket of every segment to `tol` instead of stopping at "clear of the margin".  `qpos_start`,
        `envs_idx`, `with_entity`, `ignore_entities` as in get_path_clearance.  return_detail=True: a dict with status, first (R,) the
        first segment that is not CLEAR (-1: none), lower, upper (R,), seg_lower, seg_upper, seg_status (R, K-1), stats (R, 4):
        evaluations, leaves, deepest level, segments finished, and with max_leaves > 0 leaves (R, max_leaves, 3).
        What it does not do: the arm against itself and a carried object need a bound on relative motion; this method keeps to the
        scene test, so `self_collision=True` or an `attached_entity` is refused: certify_sweep() certifies all three."""
        if self_collision or attached_entity is not None:
            raise ValueError("certify_path: the self and carried-object tests are sampled only (get_path_clearance); the certified rule "
                             "covers the sphere model against the static scene -- certify_sweep() certifies all three")
        return self._certify("certify_path", False, path, margin, tol, guard, max_depth, max_evaluations, bracket, max_leaves, max_distance,
                             return_detail, envs_idx, qpos_start, with_entity, ignore_entities)

    def _certify(self, who, sweep: bool, path, margin, tol, guard, max_depth, max_evaluations, bracket, max_leaves, max_distance, return_detail,
                 envs_idx, qpos_start, with_entity, ignore_entities, self_collision=False, self_margin=0.0, attached_entity=None,
                 ee_link_name=None, grasp_pose=None, attached_links=None):
        """certify_sweep(), and certify_path(): that without a self model and a carried object, and (`sweep` False) without their keys"""
        args, R = self._plan_args(envs_idx, qpos_start, with_entity, ignore_entities, who, self_collision, self_margin, attached_entity,
                                  ee_link_name, grasp_pose, attached_links)
        self._need("certify_path", "certified clearance")
        rows = self._path_rows(path, R, 2, "path", 0)
        K = int(rows.shape[1])
        r = self._mir.certify_path(paths=rows, margin=float(margin), tol=float(tol), guard=float(guard), max_depth=int(max_depth),
                                   max_evaluations=int(max_evaluations), bracket=bool(bracket), max_leaves=int(max_leaves),
                                   max_distance=max(float(max_distance), 2.0 * float(margin)), **args)
        out = {"status": r["row_status"], "first": r["row_first"], "lower": r["row_lower"], "upper": r["row_upper"], "seg_lower": r["seg_lower"],
               "seg_upper": r["seg_upper"], "seg_status": r["seg_status"], "stats": r["stats"]}
        if sweep:
            dev = self._mir.device
            inf = lambda *shape: torch.full((R, *shape), float("inf"), dtype=torch.float32, device=dev)  # noqa: E731
            out.update({"self_lower": r["row_self_lower"] if "row_self_lower" in r else inf(),
                        "self_upper": r["row_self_upper"] if "row_self_upper" in r else inf(),
                        "seg_self_lower": r["seg_self_lower"] if "seg_self_lower" in r else inf(K - 1),
                        "seg_self_upper": r["seg_self_upper"] if "seg_self_upper" in r else inf(K - 1),
                        "grasp": r["grasp"] if "grasp" in r else torch.full((R, 7), float("nan"), dtype=torch.float32, device=dev)})
        if "leaves" in r:
            out["leaves"] = r["leaves"]
        out = self._drop_env_axis(out, ())
        return out if return_detail else out["status"]

    def path_is_certified_clear(self, path, margin: float = 0.0, **kwargs) -> torch.Tensor:
        """(R,) bool: certify_path(path, margin, ...) is CLEAR -- the sphere model keeps `margin` from every tested geom along the whole
        trajectory.  False is "not proven": BLOCKED is a found collision, the other statuses say what ran out."""
        kwargs.pop("return_detail", None)
        return self.certify_path(path, margin=margin, **kwargs) == 0

    # ---- certified clearance with the self test and a carried object (MirScene.certify_path(self_model=, carry=) / mir_certify_path_self,
    # mir_certify_path_carry): what plan_path(self_collision=True, attached_entity=...) plans, certified for the whole of every segment.
    def certify_sweep(self, path, margin=0.0, self_margin=0.0, tol=0.002, guard=1e-5, max_depth=12, max_evaluations=4096, bracket=False,
                      max_leaves=0, max_distance=1.0, envs_idx=None, qpos_start=None, with_entity=None, ignore_entities=(), self_collision=None,
                      attached_entity=None, ee_link_name=None, grasp_pose=None, attached_links=None, return_detail=False):
        """``robot.certify_sweep(path, self_collision=True, attached_entity=cube, ee_link_name="hand")`` -> (R,) int32, spec.CERT_STATUS:
        certify_path() with the tests it refuses.  0 CLEAR -- along the WHOLE trajectory `path` ((K, R, n)) the sphere model keeps `margin`
        from every tested geom AND, with `self_collision` (None: the scene's enable_self_collision option), `self_margin` between the
        spheres of the self model AND, with `attached_entity` / `ee_link_name` / `grasp_pose` / `attached_links` (the carried object of
        plan_path()), the object's spheres keep `margin` from the scene and `self_margin` from the arm.  4 BLOCKED: a configuration
        below either margin was found; the other statuses as certify_path().  ONE launch for all rows (mir_certify_path_self / _carry,
        where the bound on the relative speed of two spheres is written down).  The arguments go through the same path as those of
        get_path_clearance().  return_detail=True: the dict of certify_path() plus self_lower, self_upper (R,), seg_self_lower,
        seg_self_upper (R, K-1) (+inf when neither a self model nor a carried object is in play) and grasp (R, 7) (NaN without a carried
        object).  Without self test and carried object this is certify_path()."""
        return self._certify("certify_sweep", True, path, margin, tol, guard, max_depth, max_evaluations, bracket, max_leaves, max_distance,
                             return_detail, envs_idx, qpos_start, with_entity, ignore_entities, self_collision, self_margin, attached_entity,
                             ee_link_name, grasp_pose, attached_links)

    def sweep_is_certified_clear(self, path, **kwargs) -> torch.Tensor:
        """(R,) bool: certify_sweep(path, ...) is CLEAR -- proven clear of the scene, of itself and with what it carries along the
        whole trajectory.  False is "not proven": BLOCKED is a found collision, the other statuses say what ran out."""
        kwargs.pop("return_detail", None)
        return self.certify_sweep(path, **kwargs) == 0

    # ---- straight-line end-effector paths (MirScene.cartesian_path / mir_cartesian_path): the approach, the lift and the place of a
    # grasp.  The name and the arguments are this package's own (MoveIt: computeCartesianPath): parity with Genesis is unpinned.
    def plan_cartesian_path(self, link, pos, quat=None, qpos_start=None, envs_idx=None, max_step=0.01, max_rot_step=0.05, jump_threshold=0.5,
                            max_points=256, num_waypoints=None, margin=0.0, ignore_collision=False, with_entity=None, ignore_entities=(),
                            self_collision=None, self_margin=0.0, attached_entity=None, ee_link_name=None, grasp_pose=None, attached_links=None,
                            return_fraction=False, return_detail=False, **ik_options):
        """``robot.plan_cartesian_path(hand, pos=(R, 3), quat=(R, 4))`` -> (W, R, n): waypoints in this entity's dof order, in the layout
        plan_path() returns (so they go into retime_path, get_path_clearance and control_dofs_position unchanged), along which `link` (a
        LinkView or a local link index) moves on a STRAIGHT LINE from where it is at `qpos_start` ((R, n); None: the current state) to
        `pos` -- (R, 3), or (R, K, 3) for a polyline of K segments -- turning along the shorter arc to `quat` ((R, 4) / (R, K, 4) wxyz, or
        one quaternion for all; None: the orientation is free).  ONE launch for all rows (MirScene.cartesian_path / mir_cartesian_path,
        where the rule is written down): inverse kinematics at samples at most `max_step` m and `max_rot_step` rad apart, each seeded
        with the one before; a sample whose IK does not converge (`ik_options`: those of inverse_kinematics), that moves a joint by more
        than `jump_threshold`, or whose edge from the sample before is in collision ends the row, which keeps the samples it achieved.
        `num_waypoints` = W: the accepted samples resampled at equal steps of their index; None: the dense samples themselves, W =
        `max_points` (the capacity: more samples than that and the row does not move), the last accepted one repeated behind the row's
        own count -- retime_path drops the repeats.  The collision keywords (`margin`, `ignore_collision`, `with_entity`,
        `ignore_entities`, `self_collision`, `self_margin`, `attached_entity`, `ee_link_name`, `attached_links`) mean what they mean in
        plan_path(); the carried object's grasp is where the object is at the start (`grasp_pose` must be None).
        return_fraction=True -> (path, fraction (R,)): the share of the line each row achieved, 1 = all of it.  return_detail=True -> a
        dict with path, fraction, valid (R,) = fraction is 1, status (R,) int32 (spec.CART_STATUS), points (R, P, n), n_points (R,)
        and stats (R, 4).  On an unbatched task every result comes without its env axis.
        What it does not do: no escape from a blocked line (that is plan_path's job), no null-space objective, one link, no axis
        masks; clearance between two samples is as coarse as the planner's edge rule."""
        args, R = self._plan_args_grasp_at_start("plan_cartesian_path", "mir_cartesian_path", grasp_pose, envs_idx, qpos_start, with_entity,
                                                 ignore_entities, self_collision, self_margin, attached_entity, ee_link_name, attached_links)
        self._need("cartesian_path", "Cartesian paths")
        dev = self._mir.device
        p = torch.as_tensor(pos, device=dev).to(torch.float32)
        if p.dim() <= 2:
            p = p.reshape(R, 1, 3)
        if p.dim() != 3 or p.shape[0] != R or p.shape[2] != 3:
            raise ValueError(f"pos must be ({R}, 3) or ({R}, K, 3), got {tuple(p.shape)}")
        K = int(p.shape[1])
        q = None
        if quat is not None:
            q = torch.as_tensor(quat, device=dev).to(torch.float32)
            q = q.reshape(1, 1, 4).expand(R, K, 4) if q.numel() == 4 else q.reshape(R, K, 4)
        W = None if num_waypoints is None else int(num_waypoints)
        r = self._mir.cartesian_path(link_body=self._link_body(link), target_pos=p.contiguous(), target_quat=None if q is None else q.contiguous(),
                                     max_pos_step=float(max_step), max_rot_step=float(max_rot_step), jump_threshold=float(jump_threshold),
                                     max_points=int(max_points), num_waypoints=0 if W is None else W, ignore_collision=bool(ignore_collision),
                                     margin=float(margin), max_distance=max(1.0, 2.0 * float(margin)), **args, **ik_options)
        path = (r["points"] if W is None else r["path"]).permute(1, 0, 2).contiguous()
        detail = {"path": path, "fraction": r["fraction"], "valid": r["status"] == 0, "status": r["status"], "points": r["points"],
                  "n_points": r["n_points"], "stats": r["stats"]}
        detail = self._drop_env_axis(detail)
        if return_detail:
            return detail
        return (detail["path"], detail["fraction"]) if return_fraction else detail["path"]

    # ---- corner blending (MirScene.blend_path / mir_blend_path): what stands between plan_path and retime_path.  The name and the
    # arguments are this package's own: parity with Genesis is unpinned.
    def blend_path(self, poly, n_poly=None, max_deviation=0.05, blend_points=8, max_shrinks=4, num_waypoints=None, max_points=None,
                   envs_idx=None, qpos_start=None, return_detail=False, resolution=0.05, margin=0.0, ignore_collision=False, with_entity=None,
                   ignore_entities=(), self_collision=None, self_margin=0.0, attached_entity=None, ee_link_name=None, grasp_pose=None,
                   attached_links=None):
        """``robot.blend_path(detail["poly"], detail["n_poly"])`` -> (W, R, n): the polyline `poly` ((R, K, n) in this entity's dof order,
        K <= 128: what plan_path(return_detail=True) returns as poly, with `n_poly` (R,) its count of valid leading nodes; None: all K)
        with every interior corner rounded by a quadratic Bezier blend that stays within `max_deviation` (L2 over the dofs) of the
        corner, `blend_points` chords per blend, in the layout plan_path() returns -- so it goes into retime_path, get_path_clearance and
        control_dofs_position unchanged.  ONE launch for all rows (MirScene.blend_path / mir_blend_path, where the rule is written
        down).  A blend cuts inside its corner, towards what the planner went round, so each one is checked like an edge of plan_path()
        (every `resolution` per joint; `margin`, `ignore_collision`, `with_entity`, `ignore_entities`, `self_collision`, `self_margin`,
        `attached_entity`, `ee_link_name`, `attached_links` mean what they mean there; the carried object's grasp is where the object
        is at the start: `grasp_pose` must be None); a blocked blend is halved up to `max_shrinks` times and then left sharp.
        `num_waypoints` = W: the smoothed path resampled at equal arc length; None: its dense points themselves, W = `max_points` (None:
        the worst case 2 + (K - 2)(blend_points + 1)), the last one repeated behind the row's own count -- retime_path drops the repeats.
        (The 128-node polyline of plan_path makes that 1136 points per row: where memory matters, slice `poly` to the nodes in use,
        poly[:, :int(n_poly.max())], or give `max_points`; a row that needs more comes back TOO_MANY_POINTS, as its start.)
        A row without motion (a failed plan: its start K times) comes back as its start.  return_detail=True -> a dict with path, valid
        (R,) = status is OK or NO_MOTION, status (R,) int32 (spec.BLEND_STATUS), points (R, P, n), n_points (R,), blend_len (R, 128): the
        accepted half-length at each input node, and stats (R, 4): nodes kept, corners blended, corners left sharp, configurations
        checked.  On an unbatched task every result comes without its env axis ((K, n) is accepted for poly).
        What it does not do: a reversal is still a stop; no jerk limit; the straight remainders of the input's segments are not checked
        again (the input was checked by whoever made it; get_path_clearance answers for the result)."""
        args, R = self._plan_args_grasp_at_start("blend_path", "mir_blend_path", grasp_pose, envs_idx, qpos_start, with_entity, ignore_entities,
                                                 self_collision, self_margin, attached_entity, ee_link_name, attached_links)
        self._need("blend_path", "corner blending")
        rows = self._path_rows(poly, R, 0, "poly", 1)
        if n_poly is not None:
            n_poly = torch.as_tensor(n_poly, device=self._mir.device).to(torch.int32).reshape(-1)
        W = None if num_waypoints is None else int(num_waypoints)
        r = self._mir.blend_path(poly=rows, n_poly=n_poly, max_deviation=float(max_deviation), blend_points=int(blend_points),
                                 max_shrinks=int(max_shrinks), max_points=None if max_points is None else int(max_points),
                                 num_waypoints=0 if W is None else W, ignore_collision=bool(ignore_collision), resolution=float(resolution),
                                 margin=float(margin), max_distance=max(1.0, 2.0 * float(margin)), **args)
        path = (r["points"] if W is None else r["path"]).permute(1, 0, 2).contiguous()
        detail = {"path": path, "valid": (r["status"] == 0) | (r["status"] == 32), "status": r["status"], "points": r["points"],
                  "n_points": r["n_points"], "blend_len": r["blend_len"], "stats": r["stats"]}
        detail = self._drop_env_axis(detail)
        return detail if return_detail else detail["path"]

    # ---- trajectory optimisation (MirScene.optimize_path / mir_optimize_path): the planner's path as a seed, a shorter, smoother path
    # further from the scene as the result.  The name and the arguments are this package's own: parity with Genesis, MoveIt's CHOMP /
    # TrajOpt and cuRobo is unpinned.
    def optimize_path(self, path, margin=0.0, resolution=0.05, smooth_weight=1.0, obstacle_weight=5.0, activation=0.05, step=0.25,
                      max_iterations=50, max_halvings=6, ftol=1e-4, envs_idx=None, qpos_start=None, with_entity=None, ignore_entities=(),
                      self_collision=None, self_margin=0.0, attached_entity=None, ee_link_name=None, grasp_pose=None, attached_links=None,
                      ignore_collision=False, return_detail=False):
        """``robot.optimize_path(path)`` -> (W, R, n): the joint path `path` ((W, R, n) as plan_path() and blend_path(num_waypoints=)
        return it, 3 <= W <= 128) with its interior waypoints moved down the covariant gradient of `smooth_weight` x smoothness +
        `obstacle_weight` x an obstacle cost of the entity's sphere model against the static scene, in the same layout -- so it goes into
        retime_path, get_path_clearance, certify_path and control_dofs_position unchanged.  ONE launch for all rows
        (MirScene.optimize_path / mir_optimize_path, where the rule is written down).  The obstacle cost starts `activation` metres
        beyond `margin`; every iteration starts at step length `step` and halves it up to `max_halvings` times while the cost does not
        fall; at most `max_iterations` iterations, fewer when the relative decrease falls below `ftol` (the defaults are spec.OPT_DEFAULTS,
        chosen on the float64 reference: DESIGN.md, Trajectory optimisation; None takes them too).  The
        result is swept like an edge of plan_path() (every `resolution` per joint; `margin`, `ignore_collision`, `with_entity`,
        `ignore_entities`, `self_collision`, `self_margin`, `attached_entity`, `ee_link_name`, `attached_links` mean what they mean
        there; the carried object's grasp is where the object is at the start: `grasp_pose` must be None), and a row that does not pass
        comes back as its input, bit for bit.  The ends never move; a row without motion (a failed plan) comes back as it is.
        return_detail=True -> a dict with path, valid (R,) = status is OK, status (R,) int32 (spec.OPT_STATUS), cost (R, 4): S and O
        of the input, S and O reached, stats (R, 6): iterations, accepted steps, halvings, configurations evaluated, configurations
        swept, stop (spec.OPT_STOP), and min_d (R,).  On an unbatched task every result comes without its env axis.
        What it does not do: no self-collision term in the cost (the sweep alone tests it); the cost looks at the waypoints only; no
        velocity, acceleration or torque limits (retime_path); fixed ends; no restarts; a BLOCKED row is not repaired."""
        args, R = self._plan_args_grasp_at_start("optimize_path", "mir_optimize_path", grasp_pose, envs_idx, qpos_start, with_entity,
                                                 ignore_entities, self_collision, self_margin, attached_entity, ee_link_name, attached_links)
        self._need("optimize_path", "trajectory optimisation")
        rows = self._path_rows(path, R, 3, "path", 0, letter="W")
        from ..backend.spec import OPT_DEFAULTS

        eps = OPT_DEFAULTS["activation"] if activation is None else float(activation)
        r = self._mir.optimize_path(paths=rows, smooth_weight=smooth_weight, obstacle_weight=obstacle_weight,
                                    activation=activation, step=step, max_iterations=max_iterations, max_halvings=max_halvings, ftol=ftol,
                                    ignore_collision=bool(ignore_collision), resolution=float(resolution), margin=float(margin),
                                    max_distance=max(1.0, 2.0 * (float(margin) + eps)), **args)
        detail = {"path": r["path"].permute(1, 0, 2).contiguous(), "valid": r["status"] == 0, "status": r["status"], "cost": r["cost"],
                  "stats": r["stats"], "min_d": r["min_d"]}
        detail = self._drop_env_axis(detail)
        return detail if return_detail else detail["path"]

    # ---- time parameterisation (MirScene.retime_path / mir_retime_path): what stands between plan_path and control_dofs_position.
    # get_dofs_force_range is a Genesis name (RigidEntity); retime_path is this package's own: parity with Genesis is unpinned.
    def get_dofs_force_range(self, dofs_idx_local=None):
        """``entity.get_dofs_force_range()`` (a Genesis name) -> (lower (n,), upper (n,)): the force range of this entity's dofs in its
        dof order, as the scene was built (frc_range).  A host-side getter: nothing is launched."""
        cols = self._jac_dofs()
        if dofs_idx_local is not None:
            cols = [cols[int(i)] for i in np.asarray(dofs_idx_local).ravel()]
        fr = np.asarray([self._b.dofs[d]["frc_range"] for d in cols], np.float32).reshape(-1, 2)
        return tuple(torch.as_tensor(np.ascontiguousarray(fr[:, k]), device=self._mir.device) for k in (0, 1))

    def _torque_rows(self, rows, idx, R: int, torque_limits):
        """the extra rows of retime_path(torque_limits=...): one per dof and waypoint of `rows` (R, K, n), lo <= alpha u + beta x <= hi
        with alpha = ID(q, 0, m) - g, beta = ID(q, m, c) - g, g = ID(q, 0, 0) and (lo, hi) = the limits - g, from three
        inverse_dynamics calls on R x K rows (evaluated at a scaled m, below).  m and c are the differences of mir_retime_path's step 2
        over the KEPT waypoints (a waypoint that repeats the one in front of it is dropped there, and its rows here are never read),
        found without a host read."""
        mir, (_, K, n) = self._mir, rows.shape
        if torque_limits is True:
            lo_lim, hi_lim = self.get_dofs_force_range()
        else:
            hi_lim = torch.as_tensor(torque_limits, device=mir.device).to(torch.float32).reshape(-1)
            if hi_lim.numel() != n:
                raise ValueError(f"torque_limits must be True or ({n},) over this entity's dofs, got {tuple(hi_lim.shape)}")
            lo_lim = -hi_lim
        ar = torch.arange(K, device=mir.device)
        kept = torch.cat([torch.ones((R, 1), dtype=torch.bool, device=mir.device), (rows[:, 1:] != rows[:, :-1]).any(-1)], 1)
        cand = torch.where(kept, ar[None, :], torch.full_like(ar, K)[None, :])
        upto = torch.flip(torch.cummin(torch.flip(cand, (1,)), 1).values, (1,))          # the first kept waypoint at or behind k
        nxt = torch.cat([upto[:, 1:], torch.full((R, 1), K, dtype=upto.dtype, device=mir.device)], 1)   # ... behind k (K: none)
        has_next = (nxt < K)[..., None]
        qn = torch.gather(rows, 1, nxt.clamp(max=K - 1)[..., None].expand(R, K, n))
        dn = torch.where(has_next, qn - rows, torch.zeros_like(rows))
        # (the waypoint in front of a kept one compares equal to the one kept before it)
        dp = torch.cat([torch.zeros_like(rows[:, :1]), rows[:, 1:] - rows[:, :-1]], 1)
        inner = has_next & (ar > 0)[None, :, None]
        m = torch.where(inner, (dn + dp) * 0.5, dn + dp)
        c = torch.where(inner, dn - dp, torch.zeros_like(rows))
        envs = (torch.arange(R, device=mir.device) if idx is None else idx).repeat_interleave(K)
        q, flat = rows.reshape(R * K, n), lambda t: t.reshape(R * K, n)  # noqa: E731
        zero = torch.zeros_like(q)
        # m is a few hundredths of a radian per waypoint: M m would be lost beside g in the float32 sum ID(q, 0, m).  The inverse dynamics
        # are linear in the acceleration and quadratic in the velocity, so a power of two s per waypoint gives
        # alpha = (ID(q, 0, s m) - g) / s and beta = (ID(q, s m, s^2 c) - g) / s^2 with the three terms at comparable sizes: s puts the
        # larger of |m| and |c| between 8 and 16 (c counts for a waypoint where the path turns round on itself, m = 0)
        size = torch.maximum(m.abs().amax(-1, keepdim=True), c.abs().amax(-1, keepdim=True)).clamp_min(2.0 ** -20)
        s = flat(torch.exp2(4.0 - torch.ceil(torch.log2(size))).expand(R, K, n))
        g = self.inverse_dynamics(zero, qpos=q, qvel=zero, envs_idx=envs)
        al = (self.inverse_dynamics(s * flat(m), qpos=q, qvel=zero, envs_idx=envs) - g) / s
        be = (self.inverse_dynamics(s * s * flat(c), qpos=q, qvel=s * flat(m), envs_idx=envs) - g) / (s * s)
        return tuple(t.reshape(R, K, n).contiguous() for t in (al, be, lo_lim[None, :] - g, hi_lim[None, :] - g))

    def retime_path(self, path, max_velocity, max_acceleration, dt=None, num_samples=None, torque_limits=None, refine: int = 1, envs_idx=None,
                    return_detail: bool = False):
        """``robot.retime_path(path, max_velocity, max_acceleration)`` -> (T, R, n): the joint path `path` ((K, R, n) as plan_path
        returns it, in this entity's dof order) as position targets every `dt` seconds (None: the scene's step) that
        control_dofs_position takes one per step: the fastest traversal of the polyline from rest to rest that keeps each dof's
        |velocity| <= `max_velocity` and |acceleration| <= `max_acceleration` (scalars or (n,)), from ONE launch for all rows
        (MirScene.retime_path / mir_retime_path, where the algorithm is written down: TOPP-RA on the waypoints).  A waypoint that
        repeats the one in front of it is dropped; a row whose waypoints are all equal (a failed plan) comes back as its start,
        status NO_MOTION, which is no error.  From a row's duration on its targets are its last waypoint.
        `refine` = r splits every segment into r equal parts first (the points stay on the polyline): the limits are collocated at the
        waypoints, so finer waypoints bound the motion more tightly.  Two distinct waypoints cannot be timed (rest to rest over one
        interval of constant path acceleration): a two-waypoint path with refine=1 raises ValueError.
        `num_samples` None: one launch without samples, ONE host read of the longest n_samples (the only synchronisation of this
        call), and a second launch with T sized to it.  An explicit `num_samples` = T is one launch without a host read; a row that
        needs more comes back TRUNCATED with its first T targets.
        `torque_limits` True (the dofs' force range, get_dofs_force_range()) or (n,): the torque of the rigid-body dynamics along the
        path stays within them, collocated at the waypoints, by one extra row per dof and waypoint from three inverse_dynamics calls
        on R x K rows (the other entities stay in their current state and at rest, as inverse_dynamics documents; no contact forces).
        return_detail=True -> a dict: samples (T, R, n), velocity (T, R, n), valid (R,) bool (OK or NO_MOTION), status (R,) int32
        (spec.RETIME_STATUS), duration (R,), n_samples (R,), and t, x (R, K'): time and squared path speed (waypoints^2 / s^2) at the
        waypoints of the refined path, K' = (K - 1) r + 1.  On an unbatched task (num_envs = 0) every result comes without its env axis.
        Not done: corners are not blended (a dof's velocity changes at a kink within one sample), no jerk limit, rest at both ends."""
        mir = self._mir
        self._need("retime_path", "time parameterisation")
        n = len(self._qcols)
        if not n:
            raise NotImplementedError("retime_path: an entity without scalar joints")
        one = bool(self.__dict__.get("unbatched"))
        idx = _env_index(mir, envs_idx)
        R = mir.num_envs if idx is None else int(idx.numel())
        rows = self._path_rows(path, R, 2, "path", 0)   # (R, K, n)
        r = int(refine)
        if r < 1:
            raise ValueError(f"refine must be >= 1, got {refine}")
        if rows.shape[1] == 2 and r == 1:
            raise ValueError("a path of two waypoints cannot be timed (rest to rest needs three): pass refine >= 2 to split its segment")

        def limit(v, name):
            a = np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, np.float32).reshape(-1)
            a = np.full(n, a[0], np.float32) if a.size == 1 else a
            if a.size != n or not (np.isfinite(a).all() and (a > 0).all()):
                raise ValueError(f"{name} must be a scalar or ({n},), finite and > 0, got {v!r}")
            return [float(x) for x in a]

        vmax, amax = limit(max_velocity, "max_velocity"), limit(max_acceleration, "max_acceleration")
        dt = float(self._b.opt["dt"] if dt is None else dt)
        if not (np.isfinite(dt) and dt > 0.0):
            raise ValueError(f"dt must be finite and > 0, got {dt}")
        if r > 1:
            f = (torch.arange(r, dtype=torch.float32, device=mir.device) / float(r))[None, None, :, None]
            a, b = rows[:, :-1, None, :], rows[:, 1:, None, :]
            rows = torch.cat([(a + f * (b - a)).reshape(R, -1, n), rows[:, -1:]], 1).contiguous()
        kw = dict(vmax=vmax, amax=amax, dt=dt)
        if torque_limits is not None and torque_limits is not False:
            kw["extra"] = self._torque_rows(rows, idx, R, torque_limits)
        if num_samples is None:
            first = mir.retime_path(rows, num_samples=0, **kw)
            T = max(int(first["n_samples"].max().item()), 1) if R > 0 else 1   # (the one host read: it waits for the launch above)
            if R * T * n > 0x7fffffff:   # (mir_retime_path's MIR_E_CAPACITY, met before anything of that size is allocated)
                raise ValueError(f"the longest row takes {T} samples at dt = {dt}: {R} x {T} x {n} targets are beyond 2^31 - 1 "
                                 "(raise the limits or dt, or pass num_samples and read the rows that come back TRUNCATED)")
        else:
            T = int(num_samples)
            if T < 1:
                raise ValueError(f"num_samples must be >= 1 or None, got {num_samples}")
        res = mir.retime_path(rows, num_samples=T, velocity=bool(return_detail), **kw)
        samples = res["samples"].permute(1, 0, 2).contiguous()
        if not return_detail:
            return samples[:, 0] if one else samples
        detail = {"samples": samples, "velocity": res["sample_vel"].permute(1, 0, 2).contiguous(), "valid": res["status"] <= 1,
                  "status": res["status"], "duration": res["duration"], "n_samples": res["n_samples"], "t": res["t"], "x": res["x"]}
        return self._drop_env_axis(detail, ("samples", "velocity"))

    def get_carried_clearance(self, qpos=None, attached_entity=None, ee_link_name=None, grasp_pose=None, attached_links=None, envs_idx=None,
                              with_entity=None, ignore_entities=(), max_distance: float = 1.0, self_collision=None) -> dict:
        """{clearance (R,), self_clearance (R,)} of ONE configuration with the carried object of plan_path() attached: `qpos` (R, n) in
        this entity's dof order (None: the current state; the object's grasp is taken there too unless `grasp_pose` is given).
        clearance: the arm's and the object's spheres against the scene; self_clearance: the object's spheres against the arm (and,
        with `self_collision`, the arm against itself).  There is no point kernel for this: the two-point trajectory [q, q] goes
        through mir_path_clearance_carry, which evaluates the configuration twice."""
        if attached_entity is None:
            raise ValueError("get_carried_clearance needs attached_entity (and ee_link_name)")
        args, R = self._plan_args(envs_idx, qpos, with_entity, ignore_entities, "get_carried_clearance", self_collision, 0.0, attached_entity,
                                  ee_link_name, grasp_pose, attached_links)
        args["self_model"]["max_distance"] = float(max_distance)
        q = self.get_dofs_position(envs_idx=envs_idx) if qpos is None else self._entity_rows(qpos, R, "qpos")
        r = self._mir.path_clearance(paths=torch.stack([q, q], 1).contiguous(), max_distance=float(max_distance), **args)
        out = {"clearance": r["row_min"], "self_clearance": r["row_self_min"]}
        return self._drop_env_axis(out, ())

    def get_link(self, name: str) -> LinkView:
        return LinkView(self._mir, self._b.body_index(name), name)

    def get_pos(self, envs_idx=None) -> torch.Tensor:
        return _rows(self._mir.get_links()[0][:, self.root, :].contiguous(), envs_idx)

    def get_quat(self, envs_idx=None) -> torch.Tensor:
        return _rows(self._mir.get_links()[1][:, self.root, :].contiguous(), envs_idx)

    def get_dofs_position(self, dofs_idx_local=None, envs_idx=None) -> torch.Tensor:
        q = self._mir.get_state()[0][:, self._qcols].contiguous()
        if dofs_idx_local is not None:
            q = q[:, [int(i) for i in np.asarray(dofs_idx_local).ravel()]].contiguous()
        return _rows(q, envs_idx)

    def get_dofs_velocity(self, dofs_idx_local=None, envs_idx=None) -> torch.Tensor:
        v = self._mir.get_state()[1][:, self.dof_idx].contiguous()
        if dofs_idx_local is not None:
            v = v[:, [int(i) for i in np.asarray(dofs_idx_local).ravel()]].contiguous()
        return _rows(v, envs_idx)

    def get_qpos(self, envs_idx=None) -> torch.Tensor:
        """(`robot.get_qpos(envs_idx=np.arange(B))`: /root/reference/examples/so_101/collect_task_stack_cube_batch.py:73,90)"""
        return self.get_dofs_position(envs_idx=envs_idx)

    def _cols(self, t: torch.Tensor) -> torch.Tensor:
        """Columns `_qcols` of a (B, n) tensor: a slice when they are a run (every scene built here), else through an index tensor kept on
        the device (a Python list as index is uploaded by every call: a synchronous copy in front of the launch)."""
        qc = self._qcols
        if self._qcols_run:
            return t[:, qc[0]:qc[0] + len(qc)]
        ix = self.__dict__.get("_qcols_t")
        if ix is None or ix.device != t.device:
            ix = self._qcols_t = torch.as_tensor(qc, dtype=torch.long, device=t.device)
        return t.index_select(1, ix)

    def inverse_kinematics_multilink(self, links, poss, quats=None, init_qpos=None, envs_idx=None, pos_mask=(True, True, True),
                                     rot_mask=(True, True, True), dofs_idx_local=None, max_samples=1, seed=0, return_error=False, **opts):
        """``robot.inverse_kinematics_multilink(links=[left_finger, right_finger], poss=[...], quats=[...])`` -> (R, n_dofs): joint
        positions that bring every link of `links` (LinkViews of this entity or local link indices, 1 .. 4) to its target at once, from
        ONE launch (MirScene.inverse_kinematics_multilink / mir_inverse_kinematics_multilink, where the iteration is defined).
        `poss` / `quats`: one (R, 3) / (R, 4) tensor per link, or one quaternion (4 numbers) per link or for all links; quats None:
        positions only.  R is the batch when `envs_idx` is None (row k = env k), else len(envs_idx), and then every argument is
        addressed by row.  `pos_mask` / `rot_mask` (world axes of the position error; 0, 1 or 3 axes of the link to align) are shared
        by the links; `dofs_idx_local` are the dofs of this entity that may move (None: every joint on a chain), every other entry of
        the result is the seed (`init_qpos` (R, n_dofs), else the current state); `max_samples` restarts from seeded random joint
        positions, the first converged sample wins.  With `return_error` also (R, L, 2): |e_pos|, |e_rot| per link."""
        if sum(bool(v) for v in rot_mask) == 2:
            raise ValueError("You can only align 0, 1 axis or all 3 axes.")
        mir = self._mir
        fn = getattr(mir, "inverse_kinematics_multilink", None)
        if fn is None:
            raise NotImplementedError("this scene has no multi-link IK (MirScene.inverse_kinematics_multilink / mir_inverse_kinematics_multilink)")
        bodies = [self._link_body(l) for l in links]
        L = len(bodies)
        idx = _env_index(mir, envs_idx)   # (None also for an arange(B) given on the host: row k = env k)
        R = mir.num_envs if idx is None else int(idx.numel())

        def per_link(ts, k, name):
            if not isinstance(ts, (list, tuple)) or (len(ts) == k and not hasattr(ts[0], "__len__")):
                ts = [ts] * L   # (one quaternion for every link)
            if len(ts) != L:
                raise ValueError(f"{name} must hold one entry per link ({L}), got {len(ts)}")
            return [torch.as_tensor(t, dtype=torch.float32, device=mir.device) for t in ts]

        def rows(ts, k, name):
            out = []
            for t in ts:
                t = t.expand(R, k) if t.numel() == k else t.reshape(-1, k)
                if t.shape[0] != R:
                    raise ValueError(f"{name}: expected {R} rows of {k}, got {tuple(t.shape)}")
                out.append(t)
            return torch.stack(out, dim=1).contiguous()

        p = rows(per_link(poss, 3, "poss"), 3, "poss")
        q, flags = None, 0
        if quats is not None:
            qs = per_link(quats, 4, "quats")
            if all(t.numel() == 4 for t in qs):
                q, flags = torch.stack([t.reshape(4) for t in qs]).contiguous(), IK_QUAT_ONE
            else:
                q = rows(qs, 4, "quats")
        qc = self._qcols
        run = self._qcols_run
        iq, col0, ncols = None, 0, 0
        if init_qpos is not None:
            iq = torch.as_tensor(init_qpos, dtype=torch.float32, device=mir.device).reshape(-1, len(qc))
            if iq.shape[0] != R:
                raise ValueError(f"init_qpos: expected {R} rows of {len(qc)}, got {tuple(iq.shape)}")
            if run:
                iq, col0, ncols = iq.contiguous(), qc[0], len(qc)
            else:
                cur = _rows(mir.get_state()[0][:, :mir.n_arm], idx).clone()
                cur[:, torch.as_tensor(qc, dtype=torch.long, device=mir.device)] = iq
                iq = cur
        dof_mask = None
        if dofs_idx_local is not None:
            dof_mask = [False] * mir.n_arm
            for i in np.asarray(dofs_idx_local).ravel():
                if not -self.n_dofs <= int(i) < self.n_dofs:
                    raise IndexError(f"dofs_idx_local: {int(i)} outside the entity's {self.n_dofs} dofs")
                dof_mask[qc[int(i)]] = True
        res = fn(bodies, p, q, iq, env_idx=idx, flags=flags, init_col0=col0, init_ncols=ncols, pos_mask=tuple(bool(v) for v in pos_mask),
                 rot_mask=tuple(bool(v) for v in rot_mask), dof_mask=dof_mask, max_samples=int(max_samples), seed=int(seed),
                 return_error=return_error, **opts)
        qout, err = (res if return_error else (res, None))
        qout = self._cols(qout).contiguous()
        return (qout, err) if return_error else qout

    def inverse_kinematics(self, link, pos=None, quat=None, init_qpos=None, envs_idx=None, return_error=False, pos_mask=(True, True, True),
                           rot_mask=(True, True, True), dofs_idx_local=None, max_samples=1, seed=0, **opts):
        """``robot.inverse_kinematics(link=eef, pos=(B,3), quat=(B,4), init_qpos=..., envs_idx=...)`` -> (B, n_dofs)
        (/root/reference/examples/franka/pick_cube_state.py:46-51).  One batched launch for all envs; `envs_idx` selects
        the rows returned (and addressed by pos / quat / init_qpos) as in Genesis.  `pos` is required (a quat-only target
        is not on the reference's path).  (The reference's experts pass full-batch targets with `envs_idx=arange(B)` on every step of
        their loops: that case costs the launch and one row gather -- no scatter, no clone, no index upload.)"""
        if pos is None:
            raise ValueError("inverse_kinematics needs a target position")
        if not (all(bool(v) for v in pos_mask) and all(bool(v) for v in rot_mask) and dofs_idx_local is None and int(max_samples) == 1 and int(seed) == 0):
            # Genesis's further arguments: the multi-link kernel with one link (every argument addressed by row, see there)
            res = self.inverse_kinematics_multilink([link], [pos], None if quat is None else [quat], init_qpos=init_qpos, envs_idx=envs_idx,
                                                    pos_mask=pos_mask, rot_mask=rot_mask, dofs_idx_local=dofs_idx_local, max_samples=max_samples,
                                                    seed=seed, return_error=return_error, **opts)
            return (res[0], res[1][:, 0].contiguous()) if return_error else res
        mir = self._mir
        B = mir.num_envs
        idx = None if envs_idx is None else torch.as_tensor(envs_idx, device=mir.device).long().reshape(-1)
        qc = self._qcols
        if IK_ROWS and hasattr(mir, "inverse_kinematics_rows") and self._qcols_run:
            # ONE launch (mir_inverse_kinematics_rows): the kernel addresses targets and seeds by row or by env itself and writes row k for
            # env envs_idx[k] -- what the scatter / clone / gather around the full-batch launch below did with five torch kernels
            n = B if idx is None else int(idx.numel())

            def arg(t, k, by_env_flag):
                t = torch.as_tensor(t, dtype=torch.float32, device=mir.device)
                if k == 4 and (t.numel() == 4 or (t.dim() == 2 and t.stride(0) == 0)):  # (one quaternion, e.g. `.expand(B, -1)`: read in place)
                    return (t.reshape(-1, 4)[0] if t.numel() == 4 else t[0]).contiguous(), IK_QUAT_ONE
                t = t.reshape(-1, k).contiguous()
                if t.shape[0] == B:
                    return t, by_env_flag
                if t.shape[0] != n:
                    raise ValueError(f"inverse_kinematics: expected {n} or {B} rows of {k}, got {tuple(t.shape)}")
                return t, 0

            p, fp = arg(pos, 3, IK_POS_BY_ENV)
            q, fq = (None, 0) if quat is None else arg(quat, 4, IK_QUAT_BY_ENV)
            iq, fi = (None, 0) if init_qpos is None else arg(init_qpos, len(qc), IK_INIT_BY_ENV)
            if CHECK_IK_IDX and idx is not None and bool(((idx < 0) | (idx >= B)).any()):
                raise IndexError("inverse_kinematics: envs_idx outside the batch")
            res = mir.inverse_kinematics_rows(link.idx, p, q, iq, None if idx is None else idx.contiguous(), fp | fq | fi, qc[0], len(qc) if iq is not None else 0,
                                              return_error=return_error, **opts)
            qout, err = (res if return_error else (res, None))
            if len(qc) != qout.shape[1]:
                qout = qout[:, qc[0]:qc[0] + len(qc)].contiguous()
            return (qout, err) if return_error else qout

        def full(t, k):
            """-> (tensor of B rows, owned): owned = a tensor made here (rows scattered to `idx`), which may be edited in place; a
            full-batch argument comes back as it is -- possibly the caller's own tensor, never written"""
            if t is None:
                return None, False
            t = torch.as_tensor(t, dtype=torch.float32, device=mir.device).reshape(-1, k)
            if idx is None or t.shape[0] == B:
                return t, False
            out = torch.zeros((B, k), dtype=torch.float32, device=mir.device)
            out[idx] = t
            return out, True

        (p, _), (q, q_owned) = full(pos, 3), full(quat, 4)
        if q is not None and q_owned:
            q[:, 0] += (q.abs().sum(1) == 0).float()  # unaddressed rows: identity, so normalisation stays finite
        init = None
        if init_qpos is not None:
            iq = torch.as_tensor(init_qpos, dtype=torch.float32, device=mir.device).reshape(-1, len(qc))
            cur = mir.get_state()[0][:, :mir.n_arm].clone()
            if idx is not None and iq.shape[0] != B:
                cur[idx[:, None], torch.as_tensor(qc, device=mir.device)[None, :]] = iq
            elif self._qcols_run:
                cur[:, qc[0]:qc[0] + len(qc)] = iq
            else:
                cur[:, qc] = iq
            init = cur
        res = mir.inverse_kinematics(link.idx, p, q, init, return_error=return_error, **opts)
        qout, err = (res if return_error else (res, None))
        qout = self._cols(qout).contiguous()
        if idx is not None:
            qout = qout[idx]
            err = None if err is None else err[idx]
        return (qout, err) if return_error else qout

    def control_dofs_position(self, position, dofs_idx_local=None) -> None:
        """PD targets for a subset of this entity's dofs (others keep their current target)."""
        tgt = self._mir.get_state()[2]
        pos = torch.as_tensor(position, dtype=torch.float32, device=tgt.device)
        idx = list(range(self.n_dofs)) if dofs_idx_local is None else [int(i) for i in np.asarray(dofs_idx_local).ravel()]
        cols = [self._ucols[i] for i in idx]
        tgt[:, cols] = pos.reshape(tgt.shape[0], len(cols))
        self._mir.set_pd_targets(tgt)


class CameraView:
    """``scene.add_camera(res, pos, lookat, fov)`` + ``cam.set_pose`` + ``cam.render()``
    (/root/reference/gym_genesis/tasks/franka/cube_pick.py:56-63,166-176; /root/reference/gym_genesis/env.py:97-98).
    ``render()`` draws ALL envs of this process at their grid offsets from the camera's current pose, like the
    reference's single shared scene, and returns ``(rgb, None, None, None)`` with ``rgb`` a NumPy uint8 (H, W, 3)
    array; depth, segmentation and normal images on request (Genesis returns rgb, depth, segmentation, normal).  ``render_envs()`` is the batched per-env image
    tensor used for the ``pixels`` observation: one launch instead of the reference's B renders."""

    def __init__(self, mir, builder, scene, res, pos, lookat, fov, up=(0.0, 0.0, 1.0), round_geoms=False):
        from ..backend.spec import make_camera

        self._mir, self._scene = mir, scene
        self.res = (int(res[0]), int(res[1]))
        self.fov = float(fov)
        self._make = make_camera
        # round_geoms: spheres and capsules drawn as themselves (MIR_VIS_ROUND_GEOMS), in every image and channel of this camera
        self._vis = builder.visual(round_geoms=round_geoms)
        self._up = tuple(up)
        self._home = (tuple(float(v) for v in pos), tuple(float(v) for v in lookat))
        self.set_pose(pos=pos, lookat=lookat)
        self._offsets = torch.as_tensor(np.ascontiguousarray(scene.envs_offset, dtype=np.float32), device=mir.device)

    def set_pose(self, pos=None, lookat=None) -> None:
        if pos is not None:
            self.pos = tuple(float(v) for v in np.asarray(pos).ravel())
        if lookat is not None:
            self.lookat = tuple(float(v) for v in np.asarray(lookat).ravel())

    def _spec(self, pos, lookat):
        # (the ctypes struct of a pose is built once: the observation renders ask for the same few poses every step)
        key = (tuple(pos), tuple(lookat), self.res, self.fov, self._up)
        cache = self.__dict__.setdefault("_specs", {})
        spec = cache.get(key)
        if spec is None:
            if len(cache) > 64:
                cache.clear()
            spec = cache[key] = self._make(self.res[0], self.res[1], pos, lookat, self.fov, self._up)
        return spec

    def render_global(self) -> torch.Tensor:
        """(H, W, 3) uint8 device tensor: every env at its grid offset, camera at its current pose."""
        img = self._mir.render(self._spec(self.pos, self.lookat), self._vis, mode=1, env_offset=self._offsets)
        # (what render() may reuse: the image is the tensor handed out as observation['pixels'], so its in-place version counter is kept
        #  too -- an edit by the caller, a normalisation or an overlay, makes render() draw again)
        self._last_global = (getattr(self._mir, "state_version", None), self.pos, self.lookat, self.res, self.fov, self._up, (id(self._vis), self._vis.flags),
                             img, img._version)
        self._record(img)
        return img

    def render_envs(self, pos=None, lookat=None, out=None) -> torch.Tensor:
        """(B, H, W, 3) uint8 device tensor: env i alone, seen from `pos` -> `lookat` relative to the env's origin
        (defaults: the pose the camera was created with)."""
        return self._mir.render(self._spec(self._home[0] if pos is None else pos, self._home[1] if lookat is None else lookat),
                                self._vis, mode=0, out=out)

    def render_cams(self, pos, lookat, up=None) -> torch.Tensor:
        """(B, H, W, 3) uint8 device tensor: env i seen from its OWN camera pos[i] -> lookat[i] (B,3 tensors in the env's
        frame; the link-mounted wrist cameras)."""
        return self._mir.render_cams(self._spec(self._home[0], self._home[1]), self._vis, pos, lookat, up)

    def render(self, rgb=True, depth=False, segmentation=False, normal=False, segmentation_level="link"):
        """Genesis's ``cam.render(rgb, depth, segmentation, normal)`` of the global view: NumPy arrays (rgb (H,W,3) uint8, depth (H,W)
        float32 planar camera-z metres with 0 for sky, segmentation (H,W) int32 body ("link") or geom ("geom") index with -1 for sky,
        normal (H,W,3) uint8), None for a channel not asked for.  The rgb image is the one of an rgb-only call (reused and recorded
        alike); the other channels come from one further pass (mir_render_outputs) and are never recorded."""
        if not (depth or segmentation or normal):
            return self._to_host(self._global_rgb()), None, None, None
        img = self._global_rgb() if rgb else None
        _, d, sg, n = self._mir.render_outputs(self._spec(self.pos, self.lookat), self._vis, mode=1, env_offset=self._offsets, rgb=False,
                                               depth=depth, segmentation=segmentation, normal=normal, seg_level=segmentation_level)
        return tuple(None if t is None else self._to_host(t, slot=k) for k, t in enumerate((img, d, sg, n)))

    def render_batch(self, rgb=True, depth=False, segmentation=False, normal=False, pos=None, lookat=None, cam_pos=None, cam_lookat=None,
                     cam_up=None, segmentation_level="link"):
        """Per-env images as device tensors, (rgb, depth, segmentation, normal) with the channels of render(), each (B,H,W[,3]) or None.
        Env i alone, seen from `pos` -> `lookat` relative to its origin (defaults: the creation pose, as render_envs()), or -- with
        cam_pos / cam_lookat (B,3), cam_up optional -- from its OWN camera, as render_cams() (the wrist cameras)."""
        if cam_pos is not None:
            if cam_lookat is None:
                raise ValueError("render_batch: cam_pos needs cam_lookat")
            spec = self._spec(self._home[0], self._home[1])
        else:
            spec = self._spec(self._home[0] if pos is None else pos, self._home[1] if lookat is None else lookat)
        return self._mir.render_outputs(spec, self._vis, mode=0, cam_pos=cam_pos, cam_lookat=cam_lookat, cam_up=cam_up, rgb=rgb, depth=depth,
                                        segmentation=segmentation, normal=normal, seg_level=segmentation_level)

    def _global_rgb(self):
        # (the reference's README loop calls env.render() right behind an env.step() whose pixels observation IS this image: nothing has
        #  moved since -- mir_get_state_version -- so it is copied out, not drawn again; the caller gets a fresh array either way)
        last = self.__dict__.get("_last_global")
        ver = getattr(self._mir, "state_version", None)
        same = (last is not None and ver is not None and last[:7] == (ver, self.pos, self.lookat, self.res, self.fov, self._up, (id(self._vis), self._vis.flags))
                and last[7]._version == last[8])
        if same:
            img = last[7]
            self._record(img)  # (a frame per call, as in Genesis)
        else:
            img = self.render_global()
        return img

    _PIN_MAX = 8  # pinned image buffers a camera lends out at a time

    def _to_host(self, img, slot=0) -> np.ndarray:
        """A fresh NumPy array of a device image.  The array IS a pinned buffer the device copies into (27 us for 480 x 640): the camera
        lends out up to `_PIN_MAX` of them and takes one back when its array is garbage-collected (`weakref.finalize`; a view keeps its
        base alive, so nothing the caller still holds is ever reused) -- the README loop drops each frame before it asks for the next and
        never pays a host memcpy.  A caller that keeps more frames than that gets copies from a staging buffer (60 - 74 us; `img.cpu()`,
        which this replaces, copies into pageable memory: 67 us per image when the frames are dropped, 224 us when they are kept and
        every array is new pages the driver has to fault in and pin).  `slot` k > 0: the k-th channel of render() (depth,
        segmentation, normal), lent from a pool of its own."""
        if not img.is_cuda:
            return img.cpu().numpy()
        import weakref

        d = self.__dict__ if slot == 0 else self.__dict__.setdefault("_pin_slots", {}).setdefault(slot, {})
        key = (tuple(img.shape), img.dtype)
        if d.get("_pin_key") != key:
            d["_pin_key"], d["_pin_pool"], d["_pin_stage"] = key, [], None   # (buffers of another size still out die with their arrays)
        pool = d["_pin_pool"]
        buf = pool.pop() if pool else (torch.empty(img.shape, dtype=img.dtype, pin_memory=True) if d.get("_pin_out", 0) < self._PIN_MAX else None)
        if buf is None:
            stage = d.get("_pin_stage")
            if stage is None:
                stage = d["_pin_stage"] = torch.empty(img.shape, dtype=img.dtype, pin_memory=True)
            stage.copy_(img, non_blocking=True)
            torch.cuda.current_stream(img.device).synchronize()
            return stage.numpy().copy()
        buf.copy_(img, non_blocking=True)
        torch.cuda.current_stream(img.device).synchronize()
        arr = buf.numpy()
        d["_pin_out"] = d.get("_pin_out", 0) + 1
        weakref.finalize(arr, self._pin_back, buf, key, slot)
        return arr

    def _pin_back(self, buf, key, slot=0) -> None:
        d = self.__dict__ if slot == 0 else self.__dict__["_pin_slots"][slot]
        d["_pin_out"] = d.get("_pin_out", 1) - 1
        if d.get("_pin_key") == key and len(d["_pin_pool"]) < self._PIN_MAX:
            d["_pin_pool"].append(buf)

    # ---- recording (cam.start_recording() at reset -- the reference: always with pixels, cube_pick.py:109-110; here: when the env was
    # made with record_video=True, see env.py; env.save_video -> cam.stop_recording: env.py:71-79).  Genesis appends the image of every cam.render() while a recording runs.  Here the GLOBAL renders are recorded --
    # render() and the `global` pixels observation -- as references to the device tensors they returned (no copy, nothing on the
    # env.step() path); the per-env observation images (one launch for all envs, into a reused buffer) are not: the reference's B
    # separate renders of a moving camera make no film either.  At most `max_recorded_frames` are kept (the newest).
    max_recorded_frames = 1024

    @property
    def recording(self) -> bool:
        return bool(self.__dict__.get("_recording"))

    def start_recording(self) -> None:
        self._recording = True
        self._frames = []
        self._frames_dropped = 0

    def _record(self, img) -> None:
        if self.__dict__.get("_recording"):
            fr = self._frames
            fr.append((img, getattr(img, "_version", None)))
            if len(fr) > self.max_recorded_frames:
                del fr[0]
                self._frames_dropped += 1

    def stop_recording(self, save_to_filename=None, fps=60) -> None:
        """Ends the recording and writes it: `.mp4` as Motion-JPEG in an ISO media file, `.gif` (tasks/video.py: this image has no H.264
        encoder).  No file name: the frames are dropped, like Genesis."""
        import warnings

        frames, dropped = self.__dict__.get("_frames") or [], self.__dict__.get("_frames_dropped", 0)
        was_on = bool(self.__dict__.get("_recording"))
        self._recording, self._frames, self._frames_dropped = False, [], 0
        if not was_on:
            # (the reference's collectors call cam.stop_recording("top.mp4") after every episode -- so_101/collect_task_stack_cube_batch.py:
            #  199-201 -- and its tasks start a recording at every reset; here that takes record_video=True: the loop goes on)
            warnings.warn(f"no recording is running (GenesisEnv(..., record_video=True) starts one at every reset, or call "
                          f"cam.start_recording()): nothing was written to {save_to_filename!r}", stacklevel=2)
            return
        if save_to_filename is None:
            return
        if dropped:
            warnings.warn(f"the recording keeps the last {self.max_recorded_frames} frames: {dropped} older ones were dropped", stacklevel=2)
        if not frames:
            warnings.warn(f"no global render since the recording started: nothing was written to {save_to_filename!r}", stacklevel=2)
            return
        edited = sum(1 for f, v in frames if v is not None and f._version != v)
        if edited:  # (frames are references to the tensors handed out as observations, not copies)
            warnings.warn(f"{edited} recorded frames were modified in place after they were handed out: the file shows them as they are now",
                          stacklevel=2)
        from .video import write_video

        write_video(save_to_filename, [self._to_host(f) if hasattr(f, "cpu") else np.asarray(f) for f, _ in frames], fps)


class SceneView:
    def __init__(self, mir, env_spacing=(1.0, 1.0), global_num_envs=None, offset=0):
        self._mir = mir
        n = mir.num_envs if global_num_envs is None else int(global_num_envs)
        per_row = max(1, int(math.ceil(math.sqrt(n))))
        idx = np.arange(n)
        rows, cols = idx // per_row, idx % per_row
        off = np.stack([(cols - (per_row - 1) / 2.0) * env_spacing[0], (rows - (math.ceil(n / per_row) - 1) / 2.0) * env_spacing[1],
                        np.zeros(n)], axis=1)
        # visual offsets only (the envs never interact); this shard's slice of the global grid
        self.envs_offset = off[offset:offset + mir.num_envs]
        self.n_envs = mir.num_envs

    def step(self) -> None:
        self._mir.step(1)

    @property
    def dt(self) -> float:
        """``scene.dt`` (a Genesis name): the step of the simulation in seconds, as the scene was built"""
        return float(self._mir.spec.opt.dt)

    def add_sensor(self, options):
        """``scene.add_sensor(gs.sensors.Lidar(...))``: a ray-cast range sensor (tasks/sensors.py: Raycaster / Lidar / DepthCamera options)
        on a link or fixed in the world; ``sensor.read()`` -> (points, distances) in one launch (mir_raycast).
        ``scene.add_sensor(gs.sensors.IMU(...))``: an accelerometer and gyro on a link; ``sensor.read()`` -> (lin_acc, ang_vel) in one
        launch (mir_link_accelerations).
        ``scene.add_sensor(sensors.Proximity(...))``: a proximity probe on a link or in the world; ``sensor.read()`` -> (distance, point,
        normal) in one launch (mir_signed_distance)."""
        from .sensors import make_sensor

        return make_sensor(self._mir, options)

    def signed_distance(self, points, radius=0.0, link=None, envs_idx=None, max_distance: float = 1.0, skip_geoms=0, geom: bool = False,
                        closest: bool = False, normal: bool = False) -> dict:
        """The plain point query (mir_signed_distance, one launch): the signed distance from `points` ((N, 3), or (3,); in the frame of
        `link` -- a LinkView or body index -- or in the world) with `radius` (a number or (N,)) to the nearest geom, negative inside a
        solid: a dict with distance (R, N) and, when asked for, geom (R, N), closest (R, N, 3), normal (R, N, 3)."""
        fn = getattr(self._mir, "signed_distance", None)
        if fn is None:
            raise NotImplementedError("this scene has no signed distance (MirScene.signed_distance / mir_signed_distance)")
        p = np.asarray(points.cpu() if isinstance(points, torch.Tensor) else points, dtype=np.float32).reshape(-1, 3)
        probes = np.concatenate([p, np.broadcast_to(np.asarray(radius, dtype=np.float32).reshape(-1, 1), (p.shape[0], 1))], axis=1)
        body = 0 if link is None else (link.idx if isinstance(link, LinkView) else int(link))
        links = None if body == 0 else np.full(p.shape[0], body, dtype=np.int32)
        return fn(probes, links=links, env_idx=_env_index(self._mir, envs_idx), max_distance=float(max_distance), skip_geoms=skip_geoms, geom=geom,
                  closest=closest, normal=normal)
