"""ctypes binding of libmirigid.so (include/mirigid.h) and a thin torch-facing wrapper.

There is deliberately NO CPU fallback: if the HIP library is missing or no GPU is
visible, creating a scene raises.  PyTorch is used only to own device buffers and
to supply the current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np
import torch

from .spec import PLAN_MAX_POLY, IK_DEFAULTS, IK_INIT_BY_ENV, IK_POS_BY_ENV, IK_QUAT_BY_ENV, IK_QUAT_ONE, MIR_VERSION, MirCameraSpec, MirCartQuery, MirDims, MirIkMulti, MirIkOptions, MirIkRows, MirAccQuery, MirBlendQuery, MirOptQuery, MirCarryQuery, MirGoalQuery, MirPoseGoalQuery, MirCertQuery, MirDistQuery, MirDynQuery, MirKinQuery, MirPlanQuery, MirRayQuery, MirRetimeQuery, MirSceneSpec, MirSelfQuery, MirTaskQuery, MirVisualSpec, make_acc_query, make_blend_query, make_opt_query, make_carry_query, make_goal_query, make_pose_goal_query, make_cart_query, make_cert_query, make_dist_query, make_dyn_query, make_ik_multi, make_kin_query, make_plan_query, make_ray_query, make_retime_query, make_self_query, make_task_query  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "csrc", "libmirigid.so"))

_lib = None


class MirError(RuntimeError):
    pass


class MirMaskError(MirError):
    """MIR_E_MASK: terminated bytes that a step kernel handed over before its solve had finished turned out wrong (include/mirigid.h,
    mir_step_begin).  A mask returned since the last successful call cannot be trusted; the scene continues with late bytes."""


def load_library() -> C.CDLL:
    """Load libmirigid.so (built in-tree by ``make -C gym-genesis_amd/csrc``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MirError(f"{LIB_PATH} not found: build it with `make -C gym-genesis_amd/csrc` "
                       "(python __graft_entry__.py build); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int32
    lib.mir_version.restype = C.c_int
    lib.mir_spec_sizeof.restype = C.c_int
    lib.mir_last_error.restype = C.c_char_p
    lib.mir_create.argtypes = [C.POINTER(MirSceneSpec), i32, i32, C.POINTER(vp)]
    lib.mir_destroy.argtypes = [vp]
    lib.mir_get_dims.argtypes = [vp, C.POINTER(MirDims)]
    lib.mir_get_model_consts.argtypes = [vp, vp, vp, vp]
    lib.mir_reset.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.mir_autoreset.argtypes = [vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.mir_set_pd_targets.argtypes = [vp, vp, vp]
    lib.mir_step.argtypes = [vp, i32, vp]
    lib.mir_step_fused.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.mir_step_begin.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.mir_step_begin.restype = C.c_int
    lib.mir_step_end.argtypes = [vp, vp]
    lib.mir_step_end.restype = C.c_int
    lib.mir_step_prepare.argtypes = [vp, vp, vp, vp, vp]
    lib.mir_step_prepare.restype = C.c_int
    lib.mir_step_go.argtypes = [vp, vp, vp]
    lib.mir_step_go.restype = C.c_int
    lib.mir_get_sync_mode.argtypes = [vp]
    lib.mir_get_sync_mode.restype = C.c_int
    lib.mir_debug_rotated_launches.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.mir_debug_rotated_launches.restype = C.c_int
    lib.mir_get_split_step.argtypes = [vp]
    lib.mir_get_split_step.restype = C.c_int
    lib.mir_debug_null_roundtrip.argtypes = [vp, i32, vp, C.POINTER(C.c_double)]
    lib.mir_debug_null_roundtrip.restype = C.c_int
    lib.mir_step_packed.argtypes = [vp, vp, vp, i32, vp]
    lib.mir_step_packed.restype = C.c_int
    lib.mir_rollout.argtypes = [vp, vp, i32, vp, i32, vp]
    lib.mir_rollout.restype = C.c_int
    lib.mir_rollout_autoreset.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp]
    lib.mir_rollout_autoreset.restype = C.c_int
    lib.mir_rollout_exact.argtypes = [vp, vp, i32, vp, i32, vp]
    lib.mir_rollout_exact.restype = C.c_int
    lib.mir_rollout_autoreset_exact.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp]
    lib.mir_rollout_autoreset_exact.restype = C.c_int
    lib.mir_get_rollout_exact_stats.argtypes = [vp, C.POINTER(C.c_uint64), i32]
    lib.mir_get_rollout_exact_stats.restype = C.c_int
    lib.mir_get_obs.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.mir_get_state.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.mir_set_state.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.mir_get_links.argtypes = [vp, vp, vp, vp]
    lib.mir_get_diag.argtypes = [vp, vp, vp, vp, vp]
    lib.mir_set_diag.argtypes = [vp, i32]
    lib.mir_set_diag.restype = C.c_int
    lib.mir_forward.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.mir_contact_forces.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mir_contact_forces.restype = C.c_int
    lib.mir_debug_render_path.argtypes = [vp, i32, i32]
    lib.mir_debug_render_path.restype = C.c_int
    lib.mir_debug_spec_active.argtypes = [vp]
    lib.mir_debug_spec_active.restype = C.c_int
    lib.mir_debug_early_mask_stats.argtypes = [vp, C.POINTER(C.c_uint32), i32, vp]
    lib.mir_debug_early_mask_stats.restype = C.c_int
    lib.mir_get_diag4.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.mir_get_diag4.restype = C.c_int
    lib.mir_get_bad.argtypes = [vp, vp, C.POINTER(C.c_uint32), i32, vp]
    lib.mir_get_bad.restype = C.c_int
    lib.mir_debug_raise_mask_flag.argtypes = [vp]
    lib.mir_debug_raise_mask_flag.restype = C.c_int
    lib.mir_get_early_mask.argtypes = [vp]
    lib.mir_get_early_mask.restype = C.c_int
    lib.mir_get_state_version.argtypes = [vp]
    lib.mir_get_state_version.restype = C.c_int
    lib.mir_set_exact_contacts.argtypes = [vp, C.POINTER(MirSceneSpec), i32]
    lib.mir_set_exact_contacts.restype = C.c_int
    lib.mir_get_exact_contacts.argtypes = [vp]
    lib.mir_get_exact_contacts.restype = C.c_int
    lib.mir_get_exact_stats.argtypes = [vp, C.POINTER(C.c_uint64), i32]
    lib.mir_get_exact_stats.restype = C.c_int
    lib.mir_get_exact_route.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.mir_get_exact_route.restype = C.c_int
    lib.mir_render.argtypes = [vp, C.POINTER(MirCameraSpec), C.POINTER(MirVisualSpec), i32, vp, vp, vp]
    lib.mir_render.restype = C.c_int
    lib.mir_visual_sizeof.restype = C.c_int
    lib.mir_render_cams.argtypes = [vp, C.POINTER(MirCameraSpec), C.POINTER(MirVisualSpec), vp, vp, vp, vp, vp]
    lib.mir_render_cams.restype = C.c_int
    lib.mir_render_outputs.argtypes = [vp, C.POINTER(MirCameraSpec), C.POINTER(MirVisualSpec), i32, vp, vp, vp, vp, C.POINTER(MirRenderOutputs), vp]
    lib.mir_render_outputs.restype = C.c_int
    lib.mir_inverse_kinematics.argtypes = [vp, i32, vp, vp, vp, C.POINTER(MirIkOptions), vp, vp, vp]
    lib.mir_inverse_kinematics.restype = C.c_int
    lib.mir_inverse_kinematics_rows.argtypes = [vp, i32, C.POINTER(MirIkRows), vp, vp, vp, C.POINTER(MirIkOptions), vp, vp, vp]
    lib.mir_inverse_kinematics_rows.restype = C.c_int
    lib.mir_ik_multi_sizeof.restype = C.c_int
    lib.mir_inverse_kinematics_multilink.argtypes = [vp, C.POINTER(MirIkMulti), vp, vp, vp, C.POINTER(MirIkOptions), vp, vp, vp, vp, vp]
    lib.mir_inverse_kinematics_multilink.restype = C.c_int
    lib.mir_kin_query_sizeof.restype = C.c_int
    lib.mir_link_kinematics.argtypes = [vp, C.POINTER(MirKinQuery), vp, i32, vp, vp, vp, vp, vp]
    lib.mir_link_kinematics.restype = C.c_int
    lib.mir_acc_query_sizeof.restype = C.c_int
    lib.mir_link_accelerations.argtypes = [vp, C.POINTER(MirAccQuery), vp, i32, vp, vp, vp, vp, vp]
    lib.mir_link_accelerations.restype = C.c_int
    lib.mir_dyn_query_sizeof.restype = C.c_int
    lib.mir_dynamics.argtypes = [vp, C.POINTER(MirDynQuery), vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mir_dynamics.restype = C.c_int
    lib.mir_task_query_sizeof.restype = C.c_int
    lib.mir_task_dynamics.argtypes = [vp, C.POINTER(MirTaskQuery), vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mir_task_dynamics.restype = C.c_int
    lib.mir_ray_query_sizeof.restype = C.c_int
    lib.mir_raycast.argtypes = [vp, C.POINTER(MirRayQuery), vp, vp, i32, vp, vp, vp, vp, vp]
    lib.mir_raycast.restype = C.c_int
    lib.mir_dist_query_sizeof.restype = C.c_int
    lib.mir_signed_distance.argtypes = [vp, C.POINTER(MirDistQuery), vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mir_signed_distance.restype = C.c_int
    lib.mir_plan_query_sizeof.restype = C.c_int
    lib.mir_plan_path.argtypes = [vp, C.POINTER(MirPlanQuery), vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mir_plan_path.restype = C.c_int
    lib.mir_path_clearance.argtypes = [vp, C.POINTER(MirPlanQuery), vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp]
    lib.mir_path_clearance.restype = C.c_int
    lib.mir_self_query_sizeof.restype = C.c_int
    lib.mir_self_distance.argtypes = [vp, C.POINTER(MirSelfQuery), i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.mir_self_distance.restype = C.c_int
    lib.mir_plan_path_self.argtypes = [vp, C.POINTER(MirPlanQuery), C.POINTER(MirSelfQuery), vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mir_plan_path_self.restype = C.c_int
    lib.mir_path_clearance_self.argtypes = [vp, C.POINTER(MirPlanQuery), C.POINTER(MirSelfQuery), vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.mir_carry_query_sizeof.restype = C.c_int
    lib.mir_plan_path_carry.argtypes = [vp, C.POINTER(MirPlanQuery), C.POINTER(MirSelfQuery), C.POINTER(MirCarryQuery), vp, vp, vp, vp, i32, vp, vp, vp, vp, vp,
                                        vp, vp, vp, vp, vp]
    lib.mir_plan_path_carry.restype = C.c_int
    lib.mir_goal_query_sizeof.restype = C.c_int
    lib.mir_plan_path_goals.argtypes = [vp, C.POINTER(MirPlanQuery), C.POINTER(MirSelfQuery), C.POINTER(MirCarryQuery), C.POINTER(MirGoalQuery), vp, vp, vp,
                                        vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mir_plan_path_goals.restype = C.c_int
    lib.mir_pose_goal_query_sizeof.restype = C.c_int
    lib.mir_plan_path_pose.argtypes = [vp, C.POINTER(MirPlanQuery), C.POINTER(MirSelfQuery), C.POINTER(MirCarryQuery), C.POINTER(MirPoseGoalQuery), vp, vp, vp,
                                       vp, i32, vp, vp, vp, vp, C.POINTER(MirIkOptions)] + [vp] * 12
    lib.mir_plan_path_pose.restype = C.c_int
    lib.mir_path_clearance_carry.argtypes = [vp, C.POINTER(MirPlanQuery), C.POINTER(MirSelfQuery), C.POINTER(MirCarryQuery), vp, vp, vp, vp, i32, vp, vp, vp,
                                             i32, vp, vp, vp, vp, vp, vp, vp]
    lib.mir_path_clearance_carry.restype = C.c_int
    lib.mir_path_clearance_self.restype = C.c_int
    lib.mir_retime_query_sizeof.restype = C.c_int
    lib.mir_retime_path.argtypes = [vp, C.POINTER(MirRetimeQuery), i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mir_retime_path.restype = C.c_int
    lib.mir_cart_query_sizeof.restype = C.c_int
    lib.mir_cartesian_path.argtypes = [vp, C.POINTER(MirCartQuery), C.POINTER(MirPlanQuery), C.POINTER(MirSelfQuery), C.POINTER(MirCarryQuery), vp, vp, vp,
                                       vp, i32, vp, vp, vp, C.POINTER(MirIkOptions), vp, vp, vp, vp, vp, vp, vp]
    lib.mir_cartesian_path.restype = C.c_int
    lib.mir_blend_query_sizeof.restype = C.c_int
    lib.mir_blend_path.argtypes = [vp, C.POINTER(MirBlendQuery), C.POINTER(MirPlanQuery), C.POINTER(MirSelfQuery), C.POINTER(MirCarryQuery), vp, vp, vp,
                                   vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mir_blend_path.restype = C.c_int
    lib.mir_opt_query_sizeof.restype = C.c_int
    lib.mir_optimize_path.argtypes = [vp, C.POINTER(MirOptQuery), C.POINTER(MirPlanQuery), C.POINTER(MirSelfQuery), C.POINTER(MirCarryQuery), vp, vp, vp,
                                      vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.mir_optimize_path.restype = C.c_int
    lib.mir_cert_query_sizeof.restype = C.c_int
    lib.mir_certify_path.argtypes = [vp, C.POINTER(MirCertQuery), C.POINTER(MirPlanQuery), vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mir_certify_path.restype = C.c_int
    lib.mir_certify_path_self.argtypes = [vp, C.POINTER(MirCertQuery), C.POINTER(MirPlanQuery), C.POINTER(MirSelfQuery), vp, vp, vp, vp, i32, vp, vp] + [vp] * 14
    lib.mir_certify_path_self.restype = C.c_int
    lib.mir_certify_path_carry.argtypes = [vp, C.POINTER(MirCertQuery), C.POINTER(MirPlanQuery), C.POINTER(MirSelfQuery), C.POINTER(MirCarryQuery), vp, vp, vp,
                                           vp, i32, vp, vp, vp] + [vp] * 15
    lib.mir_certify_path_carry.restype = C.c_int
    for name in ("mir_create", "mir_destroy", "mir_get_dims", "mir_get_model_consts", "mir_reset", "mir_autoreset", "mir_set_pd_targets",
                 "mir_step", "mir_step_fused", "mir_get_obs", "mir_get_state", "mir_set_state", "mir_get_links",
                 "mir_get_diag", "mir_forward"):
        getattr(lib, name).restype = C.c_int
    if lib.mir_spec_sizeof() != C.sizeof(MirSceneSpec) or lib.mir_version() != MIR_VERSION or lib.mir_visual_sizeof() != C.sizeof(MirVisualSpec):
        raise MirError("libmirigid.so ABI mismatch with gym_genesis.backend.spec (rebuild the library)")
    for fn, struct in (("mir_kin_query_sizeof", MirKinQuery), ("mir_acc_query_sizeof", MirAccQuery), ("mir_dyn_query_sizeof", MirDynQuery),
                       ("mir_task_query_sizeof", MirTaskQuery), ("mir_ray_query_sizeof", MirRayQuery), ("mir_dist_query_sizeof", MirDistQuery),
                       ("mir_plan_query_sizeof", MirPlanQuery), ("mir_self_query_sizeof", MirSelfQuery), ("mir_carry_query_sizeof", MirCarryQuery),
                       ("mir_goal_query_sizeof", MirGoalQuery), ("mir_pose_goal_query_sizeof", MirPoseGoalQuery),
                       ("mir_retime_query_sizeof", MirRetimeQuery), ("mir_cart_query_sizeof", MirCartQuery), ("mir_blend_query_sizeof", MirBlendQuery),
                       ("mir_opt_query_sizeof", MirOptQuery), ("mir_cert_query_sizeof", MirCertQuery), ("mir_ik_multi_sizeof", MirIkMulti)):
        if getattr(lib, fn)() != C.sizeof(struct):
            raise MirError(f"libmirigid.so ABI mismatch with gym_genesis.backend.spec: {struct.__name__} (rebuild the library)")
    _lib = lib
    _bind_fast(lib)
    return lib


_fast = None  # the _mirfast built-ins (csrc/mir_pyfast.c), bound to the loaded library; None = ctypes is used for those calls too


def _bind_fast(lib) -> None:
    """The three calls between two env.step launches as CPython built-ins (~0.06 us per call instead of ctypes' ~0.39 us: that
    difference is GPU idle time).  They are the SAME library functions, bound by address; without the module the ctypes route is
    taken, and a warning says so."""
    global _fast
    try:
        from . import _mirfast
    except ImportError as e:
        import warnings

        warnings.warn(f"gym_genesis.backend._mirfast is not built ({e}); env.step uses ctypes calls (run `make -C gym-genesis_amd/csrc`)", RuntimeWarning)
        return
    addr = lambda f: C.cast(f, C.c_void_p).value  # noqa: E731
    _mirfast.bind(addr(lib.mir_step_prepare), addr(lib.mir_step_go), addr(lib.mir_step_end))
    _fast = _mirfast


class MirRenderOutputs(C.Structure):
    """mir_render_outputs' channel table (include/mirigid.h): device pointers, each nullable."""
    _fields_ = [("struct_size", C.c_int32), ("seg_level", C.c_int32), ("rgb", C.c_void_p), ("depth", C.c_void_p),
                ("segmentation", C.c_void_p), ("normal", C.c_void_p)]


SEG_LEVELS = {"link": 0, "geom": 1}


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


# torch.cuda.current_stream(device).cuda_stream costs ~1.5 us per call (two Python objects); the raw getter is ~0.1 us.  It sits
# in front of every launch of the API path, where the GPU is idle while the host prepares the call.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


class StepHelpers:
    """Host-side helpers of the API path, shared by MirScene and the CPU test double (tests/fake_scene.py); they need
    `num_envs`, `device` and `step_fused` of the scene."""

    # ---- API-path helpers (GenesisEnv.step): the GPU idles while Python prepares a launch, so nothing that can wait is done
    # before it -- the output tensors of the NEXT call are allocated while this call's kernel runs
    def as_action(self, action, dim: int) -> torch.Tensor:
        """(B, dim) float32 contiguous device tensor from a torch tensor (device or CPU) or anything NumPy understands."""
        if type(action) is torch.Tensor and action.dtype is torch.float32 and action.device == self.device and action.is_contiguous():
            if action.shape[0] != self.num_envs or action.dim() != 2 or action.shape[1] != dim:
                raise ValueError(f"action must have shape {(self.num_envs, dim)}, got {tuple(action.shape)}")
            return action
        if not isinstance(action, torch.Tensor):
            action = torch.as_tensor(np.asarray(action))
        action = action.to(device=self.device, dtype=torch.float32).contiguous()
        if action.shape != (self.num_envs, dim):
            raise ValueError(f"action must have shape {(self.num_envs, dim)}, got {tuple(action.shape)}")
        return action

    def stage_action(self, action, dim: int) -> int:
        """Address of a (B, dim) float32 copy of a HOST action (NumPy array, list, CPU tensor) in pinned memory that the next step
        launch reads IN PLACE over PCIe (147 KB for 4096 x 9: one more read in the kernel's first batch of loads) -- no copy
        command, no device allocation.  `GenesisEnv.step(env.action_space.sample())` is how the reference is driven
        (reference env.py:61); a pageable array sent through `tensor.to(device)` costs ~25 us per step.  Two buffers take turns:
        a buffer is rewritten two steps later, and a step is closed (mir_step_end: the launch has read its action long before
        its terminated bytes leave) before the next one begins.  Only for the begin / end step path (fast_step)."""
        # (a host tensor may carry requires_grad or be a subclass: detach; device tensors never come here -- see the callers)
        a = np.asarray(action.detach().cpu().numpy() if isinstance(action, torch.Tensor) else action, dtype=np.float32)
        if a.shape != (self.num_envs, dim):
            raise ValueError(f"action must have shape {(self.num_envs, dim)}, got {tuple(a.shape)}")
        ring = self.__dict__.get("_act_stage")
        if ring is None or ring["dim"] != dim:
            bufs = [torch.empty((self.num_envs, dim), dtype=torch.float32) for _ in range(2)]
            if torch.device(self.device).type == "cuda":  # (the CPU test double reads the same address from plain memory)
                bufs = [b.pin_memory() for b in bufs]
            ring = self._act_stage = {"dim": dim, "np": [b.numpy() for b in bufs], "ptr": [b.data_ptr() for b in bufs], "bufs": bufs, "k": 0}
        k = ring["k"]
        ring["k"] = k ^ 1
        np.copyto(ring["np"][k], a)
        return ring["ptr"][k]

    def use_output_ring(self, steps: int, agent_dim: int, env_dim: int) -> torch.Tensor:
        """From now on the outputs of consecutive steps are consecutive ROWS of one preallocated (steps, B * (agent + env + 1)) float32
        buffer (row = [agent_pos (B, a) | environment_state (B, e) | reward (B)] of one step) instead of fresh allocations: the
        send buffer of a sharded run's observation gather IS the place the kernels write to (bench.py, sharding.CopyPathGather), no
        concatenation, no per-step allocation.  A row is overwritten `steps` steps later: what the caller keeps from a step is
        valid for that long (the default -- fresh tensors every step, like the reference -- is unchanged).  Returns the buffer."""
        B, w = self.num_envs, agent_dim + env_dim + 1
        buf = torch.empty((steps, B * w), dtype=torch.float32, device=self.device)
        term = torch.empty((steps, B), dtype=torch.uint8, device=self.device)
        slots = []
        for i in range(steps):
            row, base = buf[i], buf[i].data_ptr()
            outs = (row[:agent_dim * B].view(B, agent_dim), row[agent_dim * B:(agent_dim + env_dim) * B].view(B, env_dim),
                    row[(agent_dim + env_dim) * B:], term[i])
            slots.append((outs, (base, base + 4 * agent_dim * B, base + 4 * (agent_dim + env_dim) * B, term[i].data_ptr())))
        self.__dict__.get("_fresh", {}).clear()   # (outputs registered ahead came from the allocator)
        self._ring = {"dims": (agent_dim, env_dim), "slots": slots, "pos": 0, "n": steps, "buf": buf, "term": term}
        return buf

    def _alloc_outputs(self, agent_dim: int, env_dim: int):
        """Fresh output tensors of one step, with their device addresses (so the launch itself does no attribute lookups):
        ((agent_pos, environment_state, reward, terminated u8), (ptr, ptr, ptr, ptr))."""
        ring = self.__dict__.get("_ring")
        if ring is not None and ring["dims"] == (agent_dim, env_dim):
            i = ring["pos"]
            ring["pos"] = i + 1 if i + 1 < ring["n"] else 0
            return ring["slots"][i]
        B = self.num_envs
        buf = torch.empty(B * (agent_dim + env_dim + 1), dtype=torch.float32, device=self.device)
        term = torch.empty(B, dtype=torch.uint8, device=self.device)
        base = buf.data_ptr()
        outs = (buf[:agent_dim * B].view(B, agent_dim), buf[agent_dim * B:(agent_dim + env_dim) * B].view(B, env_dim),
                buf[(agent_dim + env_dim) * B:], term)
        return outs, (base, base + 4 * agent_dim * B, base + 4 * (agent_dim + env_dim) * B, term.data_ptr())

    def step_fresh(self, action, agent_dim: int, env_dim: int, host_terminated: bool = False):
        """(`action`: anything as_action / stage_action accept.)  One fused step into FRESH output tensors (callers may keep old observations, as with the reference):
        returns (agent_pos, environment_state, reward, terminated u8).  With host_terminated the launch also delivers the
        terminated bytes to the host (step_begin); the caller must then close the step with step_end().
        The GPU idles while Python prepares a launch, so nothing that can wait is done before it: the output tensors of the
        NEXT call (and, on the host path, their registration with the library) and the host array of THIS call are made
        while the kernel runs."""
        key = (agent_dim, env_dim, host_terminated)
        fresh = self.__dict__.get("_fresh")
        if fresh is None:
            fresh = self._fresh = {}
        slot = fresh.pop(key, None)
        if slot is None:
            slot = self._alloc_outputs(agent_dim, env_dim)
            if host_terminated:
                self.step_prepare_ptrs(slot[1])
        outs, ptrs = slot
        if host_terminated:
            # (a HOST action -- NumPy, list, CPU tensor -- is staged in pinned memory and read in place: stage_action; the step is
            #  closed by step_end() before the buffer comes round again)
            # (any tensor on a GPU -- this device or another, a subclass, a Parameter -- goes through as_action's .to(device); the
            #  converted tensor is held until step_end() has returned: with exact contacts the launches for the deferred envs read the
            #  action AGAIN from there, on the library's side stream -- ADVICE r5; include/mirigid.h: mir_set_exact_contacts)
            if isinstance(action, torch.Tensor) and action.is_cuda:
                action = self.as_action(action, self.nu)
                self._pend_action_ref = action
                self.step_go_ptr(action.data_ptr())
            else:
                self.step_go_ptr(self.stage_action(action, self.nu))
            host = np.empty(self.num_envs, dtype=np.bool_)
            self._host_pending = (host, host.ctypes.data)
        else:
            self.step_fused_ptrs(self.as_action(action, self.nu).data_ptr(), ptrs)
        nxt = self._alloc_outputs(agent_dim, env_dim)  # (while the kernel runs)
        if host_terminated:
            self.step_prepare_ptrs(nxt[1])
        fresh[key] = nxt
        return outs

    # pointer-level launches; the CPU test double (tests/fake_scene.py) overrides these
    def step_prepare_ptrs(self, ptrs):
        raise NotImplementedError

    def step_go_ptr(self, action_ptr):
        raise NotImplementedError

    def step_fused_ptrs(self, action_ptr, ptrs):
        raise NotImplementedError


class _SphereCall:
    """What plan_path, path_clearance, certify_path, cartesian_path, blend_path and optimize_path of MirScene share.  The constructor: the
    sphere model, the planned dofs and the rows on the device (MirScene._plan_front), D, the self query with N.  collision(), once the
    method has checked what is its own: the MirPlanQuery from the collision keywords and the carry query.  Then new() allocates (R, ...)
    outputs, head() is the argument list every C entry point starts with, symbol() picks among a call's three entry points."""

    def __init__(self, scene, probes, links, dof_qadr, env_idx, qpos_start, self_model=None):
        self.scene = scene
        self.p, self.lk, self.qa, self.idx, self.R, self.qpos_start = scene._plan_front(probes, links, dof_qadr, env_idx, qpos_start)
        self.D, self.N, self.sq, self.cq = int(self.qa.shape[0]), int(self.p.shape[0]), None, None
        self.grasp_used, self.grasp_in, self.grasp_out = None, (), ()
        self.new = scene._row_alloc(self.R)
        self.self_model(self_model)

    def self_model(self, self_model) -> None:
        if self_model is not None:
            self.sq, self.N = self.scene._self_query(self_model, int(self.p.shape[0]))

    def collision(self, carry=None, grasp_rows: bool = False, **plan) -> None:
        self.pq = make_plan_query(self.N, self.D, **plan)
        self.carry(carry, grasp_rows)

    def carry(self, carry, grasp_rows: bool) -> None:
        """carry = dict(body, link, grasp=None) or None.  With `grasp_rows` the entry point takes the rows' grasp and returns the one each row
        used (grasp_in, grasp_out: its two pointers as tuples, empty without a carried body); without, the grasp is the start row's."""
        if carry is not None and grasp_rows:
            self.cq, grasp, self.grasp_used = self.scene._carry_query(carry, self.R)
            self.grasp_in, self.grasp_out = (_ptr(grasp),), (_ptr(self.grasp_used),)
        elif carry is not None:
            self.cq = make_carry_query(carry["body"], carry["link"])

    def head(self, q=None, sq: bool = True, cq: bool = True) -> tuple:
        """(h, q?, pq, sq?, cq?, probes, links, dof_qadr, env_idx, R, qpos_start): q, the method's own query, where it has one; sq / cq
        (null without a self model / a carried body) where the entry point takes them"""
        ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
        return (self.scene.h, *(() if q is None else (C.byref(q),)), C.byref(self.pq), *((ref(self.sq),) if sq else ()),
                *((ref(self.cq),) if cq else ()), _ptr(self.p), None if self.lk is None else self.lk.ctypes.data_as(C.c_void_p),
                self.qa.ctypes.data_as(C.c_void_p), _ptr(self.idx), self.R, _ptr(self.qpos_start))

    def symbol(self, base: str, q=None):
        """-> (the entry point, its head, form): base + "_carry" with a carried body (sq may be null), base + "_self" with a self model
        alone, else base, which takes neither query"""
        form = "_carry" if self.cq is not None else "_self" if self.sq is not None else ""
        return getattr(self.scene.lib, base + form), self.head(q, sq=form != "", cq=form == "_carry"), form


class MirScene(StepHelpers):
    """A compiled, batched scene living on one GPU (``scene.build(n_envs=B)``)."""

    def __init__(self, spec: MirSceneSpec, num_envs: int, device: Optional[torch.device] = None):
        if not torch.cuda.is_available():
            raise MirError("no HIP device visible: gym_genesis (MI355X backend) has no CPU path")
        self.lib = load_library()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.spec = spec
        h = C.c_void_p()
        if self.device.index is None:  # "cuda" without an index means the CURRENT device, not device 0
            self.device = torch.device("cuda", torch.cuda.current_device())
        rc = self.lib.mir_create(C.byref(spec), int(num_envs), self.device.index, C.byref(h))
        self._check(rc)
        self.h = h
        self._hbox = [h.value]
        d = MirDims()
        self._check(self.lib.mir_get_dims(self.h, C.byref(d)))
        self.num_envs, self.nbody, self.nq, self.nv = d.num_envs, d.nbody, d.nq, d.nv
        self.ngeom, self.npair, self.agent_dim, self.env_dim = d.ngeom, d.npair, d.agent_dim, d.env_dim
        self.nfree, self.kernel = d.nfree, d.kernel
        self._go, self._devidx = self.lib.mir_step_go, self.device.index  # (looked up once: they sit in front of every API launch)
        self.nu = sum(1 for i in range(spec.ndof) if spec.dof[i].ctrl_mode == 1)
        self.n_arm = sum(1 for b in range(1, spec.nbody) if spec.body[b].jtype in (1, 2))
        # contact force sensing (contact_forces / contact_sensor): launches so far, the cached read and the counter of PD-target writes
        self.contact_force_launches, self._contact_sensor, self._targets_version = 0, None, 0

    # -- helpers -----------------------------------------------------------------------------
    def _check(self, rc: int) -> None:
        if rc != 0:
            raise (MirMaskError if rc == -5 else MirError)(f"libmirigid error {rc}: {self.lib.mir_last_error().decode()}")

    def _stream(self):
        if _raw_stream is not None:
            return _raw_stream(self.device.index)  # int; the c_void_p argtype converts it
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _launched(self, what: str) -> None:
        """counts a launch in self.<what>_launches"""
        key = what + "_launches"
        self.__dict__[key] = self.__dict__.get(key, 0) + 1

    def _row_alloc(self, R: int):
        """-> new(*shape, dtype=torch.float32): a fresh (R, *shape) device tensor"""
        return lambda *shape, dtype=torch.float32: torch.empty((R, *shape), dtype=dtype, device=self.device)

    def _rows_kd(self, t, name: str, R: int, D: int, kmin: int = 0):
        """`t` (the `paths` / `poly` / `target_pos` of a path method) as a float32 device tensor (R, K >= kmin, D) -> (t, K)"""
        t = torch.as_tensor(t, device=self.device).to(torch.float32).contiguous()
        if t.dim() != 3 or t.shape[0] != R or t.shape[2] != D or t.shape[1] < kmin:
            raise ValueError(f"{name} must be ({R}, {f'K >= {kmin}' if kmin > 0 else 'K'}, {D}), got {tuple(t.shape)}")
        return t, int(t.shape[1])

    def _f32(self, t, *cols: int) -> torch.Tensor:
        """Accept torch (any device) or NumPy, return a contiguous f32 device tensor (B, *cols)."""
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        # (a buffer handed out by staged() is read in place by the kernel -- its reuse is guarded by an event; any other host
        #  tensor, pinned or not, is copied: the caller may overwrite it as soon as this call returns)
        if not (t.device.type == "cpu" and t.data_ptr() in self.__dict__.get("_staged_ptrs", ())):
            t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if t.shape != (self.num_envs, *cols):
            raise ValueError(f"expected shape {(self.num_envs, *cols)}, got {tuple(t.shape)}")
        return t

    def _free(self, t, k: int) -> torch.Tensor:
        """Free-body poses: (B, nfree, k); (B, k) is accepted when the scene has one free body."""
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        if t.dim() == 2 and self.nfree == 1:
            t = t.unsqueeze(1)
        return self._f32(t, self.nfree, k)

    def staged(self, rows: np.ndarray) -> torch.Tensor:
        """NumPy float32 rows -> a pinned host tensor that the next reset() reads IN PLACE (its kernel loads the rows over PCIe).
        A pageable array handed to reset() goes through a synchronous copy on the DMA engine instead: 13 us when the engine is
        awake and a few hundred when it is not, on a path (reset-all every 200 steps) where nothing else waits for the GPU.  Two
        buffers per shape take turns; a buffer is reused only after the launch that read it has finished (event)."""
        ring = self.__dict__.setdefault("_stage", {})
        slot = ring.get(rows.shape)
        if slot is None:
            slot = ring[rows.shape] = {"buf": [torch.empty(rows.shape, dtype=torch.float32).pin_memory() for _ in range(2)],
                                       "ev": [torch.cuda.Event(), torch.cuda.Event()], "used": [False, False], "k": 0}
            self.__dict__.setdefault("_staged_ptrs", set()).update(b.data_ptr() for b in slot["buf"])
        k = slot["k"]
        slot["k"] = k ^ 1
        if slot["used"][k]:
            slot["ev"][k].synchronize()
        np.copyto(slot["buf"][k].numpy(), rows)
        self._stage_pending = (slot, k)
        return slot["buf"][k]

    def empty(self, *shape, dtype=torch.float32) -> torch.Tensor:
        return torch.empty((self.num_envs, *shape), dtype=dtype, device=self.device)

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.mir_destroy(self.h)
            self.h = None
            self._hbox[0] = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- C ABI, one method per entry point -------------------------------------------------------
    def model_consts(self):
        dw = np.zeros(self.nv)
        bw = np.zeros(self.nbody)
        mi = C.c_double()
        self._check(self.lib.mir_get_model_consts(self.h, dw.ctypes.data_as(C.c_void_p), bw.ctypes.data_as(C.c_void_p),
                                                  C.cast(C.byref(mi), C.c_void_p)))
        return dw, bw, mi.value

    def reset(self, obj_pos, obj_quat, arm_qpos, env_mask: Optional[torch.Tensor] = None) -> None:
        p = self._free(obj_pos, 3)   # all free bodies in body order (one for the pick scenes)
        q = self._free(obj_quat, 4)
        a = self._f32(arm_qpos, self.n_arm)
        mk = None
        if env_mask is not None:
            mk = torch.as_tensor(env_mask).to(device=self.device, dtype=torch.uint8).contiguous()
        self._check(self.lib.mir_reset(self.h, _ptr(p), _ptr(q), _ptr(a), _ptr(mk), self._stream()))
        pend = self.__dict__.pop("_stage_pending", None)
        if pend is not None:  # (the launch above reads a staged() buffer: it may be refilled once this event has passed)
            slot, k = pend
            slot["ev"][k].record(torch.cuda.current_stream(self.device))
            slot["used"][k] = True

    def autoreset(self, terminated, episode_len, max_len: int, spawn_pool, cursor, obj_quat, arm_qpos,
                  truncated_out=None, done_out=None) -> None:
        """Device-side episode bookkeeping + re-spawn of finished envs (mir_autoreset); every argument is a
        preallocated device tensor of the dtype the header names."""
        self._check(self.lib.mir_autoreset(self.h, _ptr(terminated), _ptr(episode_len), int(max_len), _ptr(spawn_pool),
                                           int(spawn_pool.shape[0]), _ptr(cursor), _ptr(obj_quat), _ptr(arm_qpos),
                                           _ptr(truncated_out), _ptr(done_out), self._stream()))

    def set_pd_targets(self, tgt) -> None:
        t = self._f32(tgt, self.nu)
        self._targets_version += 1  # (the PD targets enter the contact forces: contact_sensor())
        self._check(self.lib.mir_set_pd_targets(self.h, _ptr(t), self._stream()))

    def step(self, n_steps: int = 1) -> None:
        self._check(self.lib.mir_step(self.h, int(n_steps), self._stream()))

    def step_fused(self, action, agent_pos, env_state, reward, terminated) -> None:
        """Raw launch: all arguments are preallocated device tensors (action may be None)."""
        self._check(self.lib.mir_step_fused(self.h, _ptr(action), _ptr(agent_pos), _ptr(env_state), _ptr(reward),
                                            _ptr(terminated), self._stream()))

    def step_begin(self, action, agent_pos, env_state, reward, terminated) -> None:
        """mir_step_begin: step_fused whose terminated bytes also go to the host; close with step_end()."""
        self._check(self.lib.mir_step_begin(self.h, _ptr(action), _ptr(agent_pos), _ptr(env_state), _ptr(reward),
                                            _ptr(terminated), self._stream()))
        self._host_pending = None
        self._pend_action_ref = action  # (read again by the launches of step_end() when exact contacts are on)

    def step_prepare_ptrs(self, ptrs) -> None:
        rc = self.lib.mir_step_prepare(self.h, ptrs[0], ptrs[1], ptrs[2], ptrs[3])
        if rc:
            self._check(rc)

    def step_go_ptr(self, action_ptr) -> None:
        rc = self._go(self.h, action_ptr, _raw_stream(self._devidx) if _raw_stream is not None else self._stream())
        if rc:
            self._check(rc)

    def fast_calls(self):
        """-> (prepare, go, end, handle_box, raw_stream, device_index) for the flat env.step closure (tasks/fast_step.py): the
        _mirfast built-ins with everything they need as plain ints (handle_box[0] = the handle's address, 0 once the scene is
        closed: the library then answers "null MirHandle"), or None where ctypes has to do (no module, no raw stream getter)."""
        if _fast is None or _raw_stream is None:
            return None
        return _fast.prepare, _fast.go, _fast.end, self._hbox, _raw_stream, self._devidx

    def step_fused_ptrs(self, action_ptr, ptrs) -> None:
        rc = self.lib.mir_step_fused(self.h, action_ptr, ptrs[0], ptrs[1], ptrs[2], ptrs[3], self._stream())
        if rc:
            self._check(rc)

    def step_end(self) -> np.ndarray:
        """mir_step_end: wait for the launch of step_begin; a FRESH NumPy bool (B,) = terminated (env.py:64)."""
        pend = self.__dict__.get("_host_pending")
        if pend is None:  # (step_begin called directly: nothing was prepared during the kernel)
            host = np.empty(self.num_envs, dtype=np.bool_)
            pend = (host, host.ctypes.data)
        self._host_pending = None
        rc = self.lib.mir_step_end(self.h, pend[1])
        self._pend_action_ref = None
        if rc:
            self._check(rc)
        return pend[0]

    def step_end_ptr(self, host_ptr: int) -> None:
        """mir_step_end into a caller-provided host array (address): the flat fast path of GenesisEnv.step."""
        rc = self.lib.mir_step_end(self.h, host_ptr)
        self._pend_action_ref = None
        if rc:
            self._check(rc)

    def null_roundtrip_us(self, iters: int = 2000) -> float:
        """mir_debug_null_roundtrip: microseconds per empty-kernel launch + host-visible completion (the floor under env.step)."""
        out = C.c_double()
        self._check(self.lib.mir_debug_null_roundtrip(self.h, int(iters), self._stream(), C.byref(out)))
        return out.value

    @property
    def sync_mode(self) -> int:
        return int(self.lib.mir_get_sync_mode(self.h))

    def rotated_launches(self, actions: torch.Tensor, n: int, outputs=None) -> None:
        """mir_debug_rotated_launches: n back-to-back rotated launches cycling through actions (K,B,nu) (bench.py times them);
        `outputs` = (agent_pos, env_state, reward, terminated) tensors: every launch also writes them, like the launches of
        GenesisEnv.step (whose host-visible terminated bytes are left out: see mir_api.hip)."""
        outs = None if outputs is None else (C.c_void_p * 4)(*[t.data_ptr() for t in outputs])
        self._check(self.lib.mir_debug_rotated_launches(self.h, _ptr(actions), int(actions.shape[0]), int(n), outs, self._stream()))

    @property
    def split_step(self) -> int:
        """How step_begin launches (mir_get_split_step): 1 rotated, 2 two launches, 0 fused."""
        return int(self.lib.mir_get_split_step(self.h))

    def step_packed(self, action, rows: torch.Tensor) -> None:
        """One step; all outputs in one (B, row_stride) float32 row tensor (see mir_step_packed)."""
        self._check(self.lib.mir_step_packed(self.h, _ptr(action), _ptr(rows), int(rows.stride(0)), self._stream()))

    def rollout(self, actions: torch.Tensor, rows: torch.Tensor) -> None:
        """K env steps in one launch (mir_rollout): actions (K,B,nu), rows (K,B,row_stride) float32 device tensors."""
        K = actions.shape[0]
        if tuple(actions.shape) != (K, self.num_envs, self.nu) or rows.shape[0] != K or rows.shape[1] != self.num_envs or not (
                actions.is_contiguous() and rows.is_contiguous()):
            raise ValueError("rollout: actions (K,B,nu) and rows (K,B,row_stride) must be contiguous device tensors")
        self._check(self.lib.mir_rollout(self.h, _ptr(actions), int(K), _ptr(rows), int(rows.stride(1)), self._stream()))

    def rollout_autoreset(self, actions: torch.Tensor, rows: torch.Tensor, episode_len, max_len: int, spawn_pool, cursor, obj_quat,
                          arm_qpos) -> None:
        """K env steps + the device-side episode loop in one launch (mir_rollout_autoreset); rows need one spare column
        (truncated) after [agent | env_state | reward | terminated]."""
        K = actions.shape[0]
        if tuple(actions.shape) != (K, self.num_envs, self.nu) or rows.shape[0] != K or rows.shape[1] != self.num_envs or not (
                actions.is_contiguous() and rows.is_contiguous()):
            raise ValueError("rollout_autoreset: actions (K,B,nu) and rows (K,B,row_stride) must be contiguous device tensors")
        self._check(self.lib.mir_rollout_autoreset(self.h, _ptr(actions), int(K), _ptr(rows), int(rows.stride(1)), _ptr(episode_len), int(max_len),
                                                   _ptr(spawn_pool), int(spawn_pool.shape[0]), _ptr(cursor), _ptr(obj_quat), _ptr(arm_qpos),
                                                   self._stream()))

    def rollout_exact(self, actions: torch.Tensor, rows: torch.Tensor) -> None:
        """K env steps that keep every contact point, on the device (mir_rollout_exact): bit-identical to K x (step_begin; step_end)
        with exact contacts on; rollout() itself when they are off.  actions (K,B,nu), rows (K,B,row_stride) as in rollout()."""
        K = actions.shape[0]
        if tuple(actions.shape) != (K, self.num_envs, self.nu) or rows.shape[0] != K or rows.shape[1] != self.num_envs or not (
                actions.is_contiguous() and rows.is_contiguous()):
            raise ValueError("rollout_exact: actions (K,B,nu) and rows (K,B,row_stride) must be contiguous device tensors")
        self._check(self.lib.mir_rollout_exact(self.h, _ptr(actions), int(K), _ptr(rows), int(rows.stride(1)), self._stream()))

    def rollout_autoreset_exact(self, actions: torch.Tensor, rows: torch.Tensor, episode_len, max_len: int, spawn_pool, cursor, obj_quat,
                                arm_qpos) -> None:
        """rollout_autoreset() that keeps every contact point (mir_rollout_autoreset_exact): bit-identical to K x (step_begin; step_end;
        mir_autoreset) with exact contacts on; rollout_autoreset() itself when they are off."""
        K = actions.shape[0]
        if tuple(actions.shape) != (K, self.num_envs, self.nu) or rows.shape[0] != K or rows.shape[1] != self.num_envs or not (
                actions.is_contiguous() and rows.is_contiguous()):
            raise ValueError("rollout_autoreset_exact: actions (K,B,nu) and rows (K,B,row_stride) must be contiguous device tensors")
        self._check(self.lib.mir_rollout_autoreset_exact(self.h, _ptr(actions), int(K), _ptr(rows), int(rows.stride(1)), _ptr(episode_len),
                                                         int(max_len), _ptr(spawn_pool), int(spawn_pool.shape[0]), _ptr(cursor), _ptr(obj_quat),
                                                         _ptr(arm_qpos), self._stream()))

    def rollout_exact_stats(self, reset: bool = False) -> dict:
        """mir_get_rollout_exact_stats (synchronises the device): device-resident calls, env-steps on the three-contacts-per-lane
        instantiation, env-steps on the wave-per-env kernel, most envs handed off in one call."""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.mir_get_rollout_exact_stats(self.h, out, 1 if reset else 0))
        return {"calls": int(out[0]), "list_env_steps": int(out[1]), "wave_env_steps": int(out[2]), "max_handed": int(out[3])}

    def get_obs(self):
        agent, env = self.empty(self.agent_dim), self.empty(self.env_dim)
        rew, term = self.empty(), self.empty(dtype=torch.uint8)
        self._check(self.lib.mir_get_obs(self.h, _ptr(agent), _ptr(env), _ptr(rew), _ptr(term), self._stream()))
        return agent, env, rew, term

    def get_state(self):
        q, v = self.empty(self.nq), self.empty(self.nv)
        t, w = self.empty(self.nu), self.empty(self.nv)
        self._check(self.lib.mir_get_state(self.h, _ptr(q), _ptr(v), _ptr(t), _ptr(w), self._stream()))
        return q, v, t, w

    def set_state(self, qpos=None, qvel=None, target=None, warmstart=None) -> None:
        q = None if qpos is None else self._f32(qpos, self.nq)
        v = None if qvel is None else self._f32(qvel, self.nv)
        t = None if target is None else self._f32(target, self.nu)
        w = None if warmstart is None else self._f32(warmstart, self.nv)
        self._check(self.lib.mir_set_state(self.h, _ptr(q), _ptr(v), _ptr(t), _ptr(w), self._stream()))

    def get_links(self):
        pos, quat = self.empty(self.nbody, 3), self.empty(self.nbody, 4)
        self._check(self.lib.mir_get_links(self.h, _ptr(pos), _ptr(quat), self._stream()))
        return pos, quat

    def set_diag(self, on: bool) -> None:
        """Switch the per-env solver diagnostics (ncon / nefc / niter, 16 B per env-step) on or off (mir_set_diag)."""
        self._check(self.lib.mir_set_diag(self.h, 1 if on else 0))

    def get_diag(self, points: bool = False):
        """(ncon, nefc, niter) of the last step, int32 (B,) each; points=True adds the candidate contact points found before the
        contact capacity was applied (mir_get_diag4: more than `max_contacts` = the manifolds were thinned)."""
        a, b, c = (self.empty(dtype=torch.int32) for _ in range(3))
        if points:
            d = self.empty(dtype=torch.int32)
            self._check(self.lib.mir_get_diag4(self.h, _ptr(a), _ptr(b), _ptr(c), _ptr(d), self._stream()))
            return a, b, c, d
        self._check(self.lib.mir_get_diag(self.h, _ptr(a), _ptr(b), _ptr(c), self._stream()))
        return a, b, c

    def get_bad(self, reset: bool = False):
        """Divergence guard (mir_get_bad; diagnostics must be on): (uint8 (B,) device tensor, 1 = the env's state was non-finite after
        the last step launch; env-steps flagged since the counter was last reset)."""
        bad = self.empty(dtype=torch.uint8)
        n = C.c_uint32()
        self._check(self.lib.mir_get_bad(self.h, _ptr(bad), C.byref(n), 1 if reset else 0, self._stream()))
        return bad, int(n.value)

    def forward(self):
        M, bias = self.empty(self.nv, self.nv), self.empty(self.nv)
        qas, qacc = self.empty(self.nv), self.empty(self.nv)
        self._check(self.lib.mir_forward(self.h, _ptr(M), _ptr(bias), _ptr(qas), _ptr(qacc), self._stream()))
        return M, bias, qas, qacc

    MAX_CONTACT = 48  # MIR_MAX_CONTACT: rows of the contact list

    def contact_forces(self, contacts: bool = True, link_force: bool = True) -> dict:
        """mir_contact_forces: ONE forward-dynamics evaluation at the current state with the current PD targets -- the contact forces
        the next step applies if the targets stay as they are (Genesis reports those of the step just taken) -- that changes nothing a
        later call can see.  Fresh device tensors on the current stream: n_contacts (B,) int32, flags (B,) uint8 (bit 0: more candidate
        points than the kernel holds, forces of the thinned manifold), and with `contacts` the list in the solver's contact order,
        rows >= n_contacts zeroed -- ids (B,48,4) int32 [geom_a, geom_b, link_a, link_b], pos_normal_pen (B,48,7) [position, normal
        a -> b, penetration], force (B,48,3) on link b (link a gets the opposite) -- and with `link_force` the net contact force per
        link (B,nbody,3), the world included.  The tensors are allocated per call, not reused: contact_sensor() hands a read out to
        several callers, and a reused buffer would change under them."""
        out = {"n_contacts": self.empty(dtype=torch.int32), "flags": self.empty(dtype=torch.uint8)}
        if contacts:
            out["ids"] = self.empty(self.MAX_CONTACT, 4, dtype=torch.int32)
            out["pos_normal_pen"] = self.empty(self.MAX_CONTACT, 7)
            out["force"] = self.empty(self.MAX_CONTACT, 3)
        if link_force:
            out["link_force"] = self.empty(self.nbody, 3)
        self._check(self.lib.mir_contact_forces(self.h, _ptr(out["n_contacts"]), _ptr(out["flags"]), _ptr(out.get("ids")), _ptr(out.get("pos_normal_pen")),
                                                _ptr(out.get("force")), _ptr(out.get("link_force")), self._stream()))
        self.contact_force_launches += 1
        return out

    def contact_sensor(self) -> dict:
        """contact_forces() of the current state, shared: one launch serves every getter of every entity view until the state moves
        (mir_get_state_version: steps, resets, state writes) or the PD targets are set (set_pd_targets).  The tensors are handed out as
        they are: treat them as read-only."""
        key = (self.state_version, self._targets_version)
        last = self._contact_sensor
        if last is None or last[0] != key:
            last = self._contact_sensor = (key, self.contact_forces())
        return last[1]

    def link_kinematics(self, links, local_points=None, env_idx=None, dof0: int = 0, n_dofs: Optional[int] = None, pos: bool = True,
                        quat: bool = True, vel: bool = True, jac: bool = True) -> dict:
        """mir_link_kinematics: poses, velocities and geometric Jacobians of the links `links` (body indices of the spec, repeats allowed)
        in ONE launch of a kernel of its own, for the envs `env_idx` (int64 device tensor, any order, repeats allowed; None: all envs).
        With p = the link's origin + R_link local_point (local_points (3,) or (n_links, 3); None: the origins), R rows and L links:
        pos (R,L,3) = p, quat (R,L,4) wxyz, vel (R,L,6) = world linear velocity of p and world angular velocity of the link,
        jac (R,L,6,n_dofs) = the columns of the scene dofs [dof0, dof0 + n_dofs) (n_dofs None: up to nv) of the map qvel -> vel.
        Only the outputs asked for are computed and returned: fresh device tensors on the current stream.  The read changes nothing."""
        nd = self.nv - int(dof0) if n_dofs is None else int(n_dofs)
        q = make_kin_query(links, local_points, dof0, nd)
        idx = None
        if env_idx is not None:
            idx = torch.as_tensor(env_idx, device=self.device).long().reshape(-1).contiguous()
        R, L = (self.num_envs if idx is None else int(idx.numel())), q.n_links
        new = lambda *shape: torch.empty((R, L, *shape), dtype=torch.float32, device=self.device)  # noqa: E731
        out = {}
        if pos:
            out["pos"] = new(3)
        if quat:
            out["quat"] = new(4)
        if vel:
            out["vel"] = new(6)
        if jac:
            out["jac"] = new(6, max(nd, 0))
        self._check(self.lib.mir_link_kinematics(self.h, C.byref(q), _ptr(idx), R, _ptr(out.get("pos")), _ptr(out.get("quat")), _ptr(out.get("vel")),
                                                 _ptr(out.get("jac")), self._stream()))
        self._launched("link_kinematics")
        return out

    def link_accelerations(self, links, local_points=None, quat_offsets=None, env_idx=None, qacc=None, acc: bool = True,
                           bias_acc: bool = False, imu: bool = False) -> dict:
        """mir_link_accelerations: world accelerations of the links `links` (body indices of the spec, repeats allowed) in ONE launch of a
        kernel of its own, for the envs `env_idx` (int64 device tensor, any order, repeats allowed; None: all envs).  With p = the link's
        origin + R_link local_point (local_points (3,) or (n_links, 3); None: the origins), R rows and L links:
        acc (R,L,6) = classical world linear acceleration of the material point p, then the link's world angular acceleration
        (J qacc + Jdot qvel with the J of link_kinematics); bias_acc (R,L,6) = the same at qacc = 0 (Jdot qvel); imu (R,L,6) = what an
        accelerometer and a gyro at p with the axes R_link R(quat_offsets) read: R_s^T (acc - gravity), R_s^T w (quat_offsets wxyz, (4,) or
        (n_links, 4); None: the link's axes).  `qacc` (R,nv), in the dof order of get_state(), is used as given; None: the acceleration
        the next step applies if the targets stay as they are (forward(), gathered to the rows; the convention of contact_forces) -- taken
        only when acc or imu is asked for.  Only the outputs asked for are computed and returned: fresh device tensors on the current
        stream.  The read changes nothing (with qacc=None: nothing that a bare forward() does not)."""
        q = make_acc_query(links, local_points, quat_offsets)
        idx = None
        if env_idx is not None:
            idx = torch.as_tensor(env_idx, device=self.device).long().reshape(-1).contiguous()
        R, L = (self.num_envs if idx is None else int(idx.numel())), q.n_links
        if acc or imu:
            if qacc is None:
                qacc = self.forward()[3]
                if idx is not None:
                    qacc = qacc.index_select(0, idx.clamp(0, self.num_envs - 1))   # (the kernel clamps the same way)
            qacc = torch.as_tensor(qacc, device=self.device).to(torch.float32).contiguous()
            if tuple(qacc.shape) != (R, self.nv):
                raise ValueError(f"qacc must be ({R}, {self.nv}), got {tuple(qacc.shape)}")
        else:
            qacc = None
        out = {}
        for name, want in (("acc", acc), ("bias_acc", bias_acc), ("imu", imu)):
            if want:
                out[name] = torch.empty((R, L, 6), dtype=torch.float32, device=self.device)
        self._check(self.lib.mir_link_accelerations(self.h, C.byref(q), _ptr(idx), R, _ptr(qacc), _ptr(out.get("acc")), _ptr(out.get("bias_acc")),
                                                    _ptr(out.get("imu")), self._stream()))
        if out and R > 0:
            self._launched("link_accelerations")
        return out

    def dynamics(self, env_idx=None, dof0: int = 0, n_dofs: Optional[int] = None, qpos=None, qvel=None, qacc=None, mass: bool = True,
                 bias: bool = True, gravity: bool = False, tau: bool = False, ctrl_force: bool = False) -> dict:
        """mir_dynamics: joint-space dynamics of the scene dofs [dof0, dof0 + n_dofs) (n_dofs None: up to nv) in ONE launch of a kernel
        of its own, for the envs `env_idx` (int64 device tensor, any order, repeats allowed; None: all envs).  With R rows and n dofs:
        mass (R,n,n) = the composite-rigid-body mass matrix with armature on the diagonal, bias (R,n) = Coriolis + centrifugal + gravity
        forces (M qacc + bias = applied torque), gravity (R,n) = bias at qvel = 0, tau (R,n) = the window of M qacc + bias for the
        full-length `qacc` (R,nv), ctrl_force (R,n) = the clamped PD torque of the current targets.  `qpos` (R,nq) / `qvel` (R,nv), in
        the layout of get_state(), replace the rows' current state for this evaluation only.  Only the outputs asked for are computed
        and returned: fresh device tensors on the current stream.  The read changes nothing."""
        nd = self.nv - int(dof0) if n_dofs is None else int(n_dofs)
        q = make_dyn_query(dof0, nd)
        idx = None
        if env_idx is not None:
            idx = torch.as_tensor(env_idx, device=self.device).long().reshape(-1).contiguous()
        R = self.num_envs if idx is None else int(idx.numel())

        def rows(t, width, name):
            if t is None:
                return None
            t = torch.as_tensor(t, device=self.device).to(torch.float32).contiguous()
            if tuple(t.shape) != (R, width):
                raise ValueError(f"{name} must be ({R}, {width}), got {tuple(t.shape)}")
            return t

        qpos, qvel, qacc = rows(qpos, self.nq, "qpos"), rows(qvel, self.nv, "qvel"), rows(qacc, self.nv, "qacc")
        if tau and qacc is None:
            raise ValueError("tau needs qacc")
        n = max(nd, 0)
        new = lambda *shape: torch.empty((R, *shape), dtype=torch.float32, device=self.device)  # noqa: E731
        out = {}
        if mass:
            out["mass"] = new(n, n)
        for name, want in (("bias", bias), ("gravity", gravity), ("tau", tau), ("ctrl_force", ctrl_force)):
            if want:
                out[name] = new(n)
        self._check(self.lib.mir_dynamics(self.h, C.byref(q), _ptr(idx), R, _ptr(qpos), _ptr(qvel), _ptr(qacc), _ptr(out.get("mass")),
                                          _ptr(out.get("bias")), _ptr(out.get("gravity")), _ptr(out.get("tau")), _ptr(out.get("ctrl_force")),
                                          self._stream()))
        if out and R > 0 and n > 0:
            self._launched("dynamics")
        return out

    def task_dynamics(self, links=(), local_points=None, env_idx=None, dof0: int = 0, n_dofs: Optional[int] = None, qpos=None, x=None,
                      damping: float = 0.0, minv: bool = False, solve: bool = False, lambda_inv: Optional[bool] = None,
                      lambda_: Optional[bool] = None, jbar: Optional[bool] = None) -> dict:
        """mir_task_dynamics: operational-space dynamics of the links `links` (body indices of the spec, repeats allowed; none for minv /
        solve alone) in ONE launch of a kernel of its own, for the envs `env_idx` (int64 device tensor, any order, repeats allowed; None:
        all envs).  With M the mass matrix of dynamics(), J the Jacobian of link_kinematics() at `local_points` ((3,) or (n_links, 3);
        None: the origins), R rows, L links and n the dofs [dof0, dof0 + n_dofs) (n_dofs None: up to nv):
        minv (R,n,n) = the window of M^-1, solve (R,n) = the window of M^-1 x for the full-length `x` (R,nv), lambda_inv (R,L,6,6) =
        J M^-1 J^T, lambda (R,L,6,6) = (J M^-1 J^T + damping^2 I)^-1, jbar (R,L,n,6) = the window rows of M^-1 J^T lambda.  The window
        selects what is written, never what is inverted.  Where the 6 x 6 matrix is singular to float32 (a relative Cholesky pivot
        <= 1e-5: a link with fewer than six dofs above it, an arm at a singularity) lambda and jbar of that row and link are NaN;
        damping > 0 is the remedy.  `qpos` (R,nq), in the layout of get_state(), replaces the rows' current qpos for this evaluation
        only.  Only the outputs asked for are computed and returned (lambda under the key "lambda"; lambda_inv / lambda_ / jbar None:
        asked for when there are links): fresh device tensors on the current stream.  The read changes nothing."""
        nd = self.nv - int(dof0) if n_dofs is None else int(n_dofs)
        lambda_inv, lambda_, jbar = (bool(len(links)) if w is None else bool(w) for w in (lambda_inv, lambda_, jbar))
        q = make_task_query(links, local_points, dof0, nd, damping)
        idx = None
        if env_idx is not None:
            idx = torch.as_tensor(env_idx, device=self.device).long().reshape(-1).contiguous()
        R, L = (self.num_envs if idx is None else int(idx.numel())), q.n_links

        def rows(t, width, name):
            if t is None:
                return None
            t = torch.as_tensor(t, device=self.device).to(torch.float32).contiguous()
            if tuple(t.shape) != (R, width):
                raise ValueError(f"{name} must be ({R}, {width}), got {tuple(t.shape)}")
            return t

        qpos, x = rows(qpos, self.nq, "qpos"), rows(x, self.nv, "x")
        if solve and x is None:
            raise ValueError("solve needs x")
        if (lambda_inv or lambda_ or jbar) and L == 0:
            raise ValueError("lambda_inv, lambda and jbar need a link")
        n = max(nd, 0)
        new = lambda *shape: torch.empty((R, *shape), dtype=torch.float32, device=self.device)  # noqa: E731
        out = {}
        if minv:
            out["minv"] = new(n, n)
        if solve:
            out["solve"] = new(n)
        if lambda_inv:
            out["lambda_inv"] = new(L, 6, 6)
        if lambda_:
            out["lambda"] = new(L, 6, 6)
        if jbar:
            out["jbar"] = new(L, n, 6)
        self._check(self.lib.mir_task_dynamics(self.h, C.byref(q), _ptr(idx), R, _ptr(qpos), _ptr(x), _ptr(out.get("minv")), _ptr(out.get("solve")),
                                               _ptr(out.get("lambda_inv")), _ptr(out.get("lambda")), _ptr(out.get("jbar")), self._stream()))
        if R > 0 and any(v.numel() for v in out.values()):
            self._launched("task_dynamics")
        return out

    def raycast(self, dirs, link: int = 0, pos_offset=(0.0, 0.0, 0.0), quat_offset=(1.0, 0.0, 0.0, 0.0), min_range: float = 0.0,
                max_range: float = 100.0, skip_geoms=(), env_idx=None, world_frame: bool = False, distance: bool = True,
                points: bool = True, geom: bool = False, normal: bool = False) -> dict:
        """mir_raycast: the range along the N rays `dirs` ((N,3) float32, sensor frame, any length; a device tensor is used as it is)
        of ONE sensor that rides on body `link` (0: the world) at `pos_offset` / `quat_offset` (wxyz) in the link's frame, for the envs
        `env_idx` (int64, any order, repeats allowed; None: all envs), in ONE launch of a kernel of its own.  Every geom not in
        `skip_geoms` (indices, or the bit mask) is tested; hulls as the polytope of their vertices; a solid that contains the origin
        is not seen.  distance (R,N) = clamp(range, min_range, max_range), max_range on a miss; points (R,N,3) = distance x the unit
        direction in the sensor's frame, or origin + that in world axes with `world_frame`; geom (R,N) int32, -1 on a miss; normal
        (R,N,3) unit outward normal in the axes of points, 0 on a miss.  Only the outputs asked for are computed and returned: fresh
        device tensors on the current stream.  The read changes nothing a later call can see."""
        if not isinstance(dirs, torch.Tensor):
            dirs = torch.as_tensor(np.ascontiguousarray(dirs, dtype=np.float32))
        d = dirs.to(device=self.device, dtype=torch.float32).contiguous()
        if d.dim() != 2 or d.shape[1] != 3 or d.shape[0] < 1:
            raise ValueError(f"dirs must be (N, 3) with N >= 1, got {tuple(d.shape)}")
        N = int(d.shape[0])
        q = make_ray_query(N, link, pos_offset, quat_offset, min_range, max_range, skip_geoms, world_frame)
        idx = None
        if env_idx is not None:
            idx = torch.as_tensor(env_idx, device=self.device).long().reshape(-1).contiguous()
        R = self.num_envs if idx is None else int(idx.numel())
        out = {}
        if distance:
            out["distance"] = torch.empty((R, N), dtype=torch.float32, device=self.device)
        if points:
            out["points"] = torch.empty((R, N, 3), dtype=torch.float32, device=self.device)
        if geom:
            out["geom"] = torch.empty((R, N), dtype=torch.int32, device=self.device)
        if normal:
            out["normal"] = torch.empty((R, N, 3), dtype=torch.float32, device=self.device)
        self._check(self.lib.mir_raycast(self.h, C.byref(q), _ptr(d), _ptr(idx), R, _ptr(out.get("distance")), _ptr(out.get("points")),
                                         _ptr(out.get("geom")), _ptr(out.get("normal")), self._stream()))
        self._launched("raycast")
        return out

    def _sphere_probes(self, probes, links, n_extra=None):
        """the sphere model of signed_distance, self_distance, plan_path and path_clearance -> (probes on the device, links as host int32
        or None).  n_extra: the call is self_distance(), whose probes are (N + n_extra, 4).  (Each call builds its query struct behind
        this and before _sphere_qrows(): the order of their ValueErrors.)"""
        if not isinstance(probes, torch.Tensor):
            probes = torch.as_tensor(np.ascontiguousarray(probes, dtype=np.float32))
        p = probes.to(device=self.device, dtype=torch.float32).contiguous()
        if p.dim() != 2 or p.shape[1] != 4 or p.shape[0] - int(n_extra or 0) < 1:
            raise ValueError(f"probes must be (N, 4) with N >= 1, got {tuple(p.shape)}" if n_extra is None else
                             f"probes must be (N + n_extra, 4) with N >= 1, got {tuple(p.shape)} with n_extra = {n_extra}")
        lk = None
        if links is not None:
            lk = np.ascontiguousarray(links.cpu().numpy() if isinstance(links, torch.Tensor) else links, dtype=np.int32).reshape(-1)
            if lk.shape[0] != p.shape[0]:
                raise ValueError(f"links must be ({p.shape[0]},), got {lk.shape}")
        return p, lk

    def _sphere_qrows(self, env_idx, qpos, qpos_name: str = "qpos"):
        """... and their rows -> (the row list on the device or None, R, the qpos rows (R, nq) on the device or None)"""
        idx = None if env_idx is None else torch.as_tensor(env_idx, device=self.device).long().reshape(-1).contiguous()
        R = self.num_envs if idx is None else int(idx.numel())
        if qpos is not None:
            qpos = torch.as_tensor(qpos, device=self.device).to(torch.float32).contiguous()
            if tuple(qpos.shape) != (R, self.nq):
                raise ValueError(f"{qpos_name} must be ({R}, {self.nq}), got {tuple(qpos.shape)}")
        return idx, R, qpos

    def signed_distance(self, probes, links=None, env_idx=None, qpos=None, max_distance: float = 1.0, skip_geoms=0, geom: bool = False,
                        closest: bool = False, normal: bool = False, row_min: bool = False) -> dict:
        """mir_signed_distance: the signed distance from the N probe spheres `probes` ((N,4) float32: centre in the frame of the probe's
        link, radius; a device tensor is used as it is) to the nearest geom, for the envs `env_idx` (int64, any order, repeats allowed;
        None: all envs), in ONE launch of a kernel of its own.  `links` (N,) host integers: the body each probe rides on (0: the world;
        None: all in the world).  Every geom not in `skip_geoms` (indices, or the bit mask) is tested, each as its exact shape.
        `qpos` (R,nq), in the layout of get_state(), is evaluated instead of the rows' current state, for this call only.
        distance (R,N) = distance to the surface minus the probe's radius, negative inside, max_distance on a miss; geom (R,N) int32,
        -1 on a miss; closest (R,N,3) = the nearest surface point in world axes (the probe centre on a miss); normal (R,N,3) = the unit
        outward gradient, 0 on a miss; row_min: adds row_min (R,) and row_argmin (R,) int32, the lowest distance of a row and its probe.
        distance and what was asked for are returned: fresh device tensors on the current stream.  The call changes nothing a later
        call can see."""
        p, lk = self._sphere_probes(probes, links)
        N = int(p.shape[0])
        q = make_dist_query(N, max_distance, skip_geoms)
        idx, R, qpos = self._sphere_qrows(env_idx, qpos)
        new = self._row_alloc(R)
        out = {"distance": new(N)}
        if geom:
            out["geom"] = new(N, dtype=torch.int32)
        if closest:
            out["closest"] = new(N, 3)
        if normal:
            out["normal"] = new(N, 3)
        if row_min:
            out["row_min"], out["row_argmin"] = new(), new(dtype=torch.int32)
        self._check(self.lib.mir_signed_distance(self.h, C.byref(q), _ptr(p), None if lk is None else lk.ctypes.data_as(C.c_void_p), _ptr(idx), R,
                                                 _ptr(qpos), _ptr(out["distance"]), _ptr(out.get("geom")), _ptr(out.get("closest")),
                                                 _ptr(out.get("normal")), _ptr(out.get("row_min")), _ptr(out.get("row_argmin")), self._stream()))
        if R > 0:
            self._launched("distance")
        return out

    def self_distance(self, probes, links, link_mask, env_idx=None, qpos=None, max_distance: float = 1.0, n_extra: int = 0,
                      other: bool = False, row_min: bool = False) -> dict:
        """mir_self_distance: the sphere model `probes` (N + E, 4) / `links` (N + E,) (as in signed_distance(); the last `n_extra` are
        the self-only spheres, which this call treats like the others) against ITSELF, for the envs `env_idx` (None: all), in ONE
        launch.  `link_mask` (32,) words: bit b of word a = the spheres on body a are tested against those on body b (symmetric, zero
        diagonal).  distance (R, N + E) = per sphere the lowest |ci - cj| - ri - rj over the spheres it is tested against, max_distance
        when none is that near; other (R, N + E) int32 = that sphere, -1: none; row_min: adds row_min (R,) and row_pair (R, 2) int32,
        the lowest distance of the row and its pair (i < j; (-1, -1): none).  `qpos` (R, nq) is evaluated instead of the rows' current
        state.  Fresh device tensors on the current stream; the call changes nothing a later call can see."""
        p, lk = self._sphere_probes(probes, links, n_extra=n_extra)
        NS = int(p.shape[0])
        sq = make_self_query(link_mask, n_extra, 0.0, max_distance)
        idx, R, qpos = self._sphere_qrows(env_idx, qpos)
        new = self._row_alloc(R)
        out = {"distance": new(NS)}
        if other:
            out["other"] = new(NS, dtype=torch.int32)
        if row_min:
            out["row_min"], out["row_pair"] = new(), new(2, dtype=torch.int32)
        self._check(self.lib.mir_self_distance(self.h, C.byref(sq), NS - int(n_extra), _ptr(p), None if lk is None else lk.ctypes.data_as(C.c_void_p),
                                               _ptr(idx), R, _ptr(qpos), _ptr(out["distance"]), _ptr(out.get("other")), _ptr(out.get("row_min")),
                                               _ptr(out.get("row_pair")), self._stream()))
        if R > 0:
            self._launched("self")
        return out

    @staticmethod
    def _self_query(self_model, n_total):
        """self_model = dict(link_mask (32,), n_extra, self_margin, max_distance) -> (MirSelfQuery, N: the probes of the scene test)"""
        sq = make_self_query(self_model["link_mask"], self_model.get("n_extra", 0), self_model.get("self_margin", 0.0), self_model.get("max_distance", 1.0))
        return sq, n_total - int(sq.n_extra)

    def _plan_front(self, probes, links, dof_qadr, env_idx, qpos_start):
        """the arguments mir_plan_path and mir_path_clearance share -> (probes on the device, links, dof addresses, row list, R, start rows)"""
        p, lk = self._sphere_probes(probes, links)
        qa = np.ascontiguousarray(dof_qadr, dtype=np.int32).reshape(-1)
        return (p, lk, qa, *self._sphere_qrows(env_idx, qpos_start, "qpos_start"))

    def _carry_query(self, carry, R):
        """carry = dict(body, link, grasp=None) -> (MirCarryQuery, the grasp rows (R, 7) on the device or None, grasp_used (R, 7))"""
        cq = make_carry_query(carry["body"], carry["link"])
        grasp = carry.get("grasp")
        if grasp is not None:
            grasp = torch.as_tensor(grasp, device=self.device).to(torch.float32).contiguous()
            if tuple(grasp.shape) != (R, 7):
                raise ValueError(f"grasp must be ({R}, 7): position xyz and quaternion wxyz per row, got {tuple(grasp.shape)}")
        return cq, grasp, torch.empty((R, 7), dtype=torch.float32, device=self.device)

    def plan_path(self, probes, links, dof_qadr, qpos_goal, env_idx=None, qpos_start=None, num_waypoints: int = 100, max_nodes: int = 256,
                  max_iterations: int = 2000, smooth_passes: int = 64, ignore_collision: bool = False, seed: int = 0, resolution: float = 0.05,
                  step: float = 0.3, margin: float = 0.0, max_distance: float = 1.0, skip_geoms=0, self_model=None, carry=None) -> dict:
        """mir_plan_path: for the envs `env_idx` (None: all), ONE launch plans a collision-checked path for the planned dofs `dof_qadr`
        (qpos addresses of D limited scalar joints) from `qpos_start` ((R, nq) full rows in the layout of get_state(); None: the current
        state) to `qpos_goal` (R, D): RRT-Connect, shortcut smoothing, resampling (include/mirigid.h has the algorithm).  `probes` (N, 4)
        / `links` (N,) are the sphere model as in signed_distance(); every geom not in `skip_geoms` is an obstacle and must not ride on a
        planned joint.  -> dict of fresh device tensors: path (R, W, D), status (R,) int32 (spec.PLAN_STATUS), poly (R, 128, D) the
        polyline behind the waypoints, n_poly (R,), stats (R, 4): iterations, nodes of the two trees, configurations checked.  A row
        that fails holds its start W times.  The call changes nothing a later call can see.
        `self_model` = dict(link_mask (32,) words, n_extra, self_margin, max_distance): mir_plan_path_self -- a configuration must
        also keep `self_margin` between the spheres of the links the mask enables; the last `n_extra` probes take part in that test
        only; statuses 7 and 8 (START / GOAL_IN_SELF_COLLISION).
        `carry` = dict(body, link, grasp=None): mir_plan_path_carry -- the free body `body` follows the body `link` by a rigid grasp
        transform per row, `grasp` (R, 7) = its position xyz and quaternion wxyz in the link's frame (None: the kernel takes it from
        the start row), and the probes whose link is `body` ride on it; the body's own geoms must be in `skip_geoms`.  With or
        without `self_model`.  The result gains grasp (R, 7): the transform each row used."""
        s = _SphereCall(self, probes, links, dof_qadr, env_idx, qpos_start, self_model)
        R, D, new = s.R, s.D, s.new
        goal = torch.as_tensor(qpos_goal, device=self.device).to(torch.float32).contiguous()
        if tuple(goal.shape) != (R, D):
            raise ValueError(f"qpos_goal must be ({R}, {D}), got {tuple(goal.shape)}")
        s.collision(carry, True, num_waypoints=num_waypoints, max_nodes=max_nodes, max_iterations=max_iterations, smooth_passes=smooth_passes,
                    ignore_collision=ignore_collision, seed=seed, resolution=resolution, step=step, margin=margin, max_distance=max_distance,
                    skip_geoms=skip_geoms)
        W = max(int(num_waypoints), 0)
        out = {"path": new(W, D), "status": new(dtype=torch.int32), "poly": new(PLAN_MAX_POLY, D), "n_poly": new(dtype=torch.int32),
               "stats": new(4, dtype=torch.int32)}
        fn, head, form = s.symbol("mir_plan_path")
        if form == "_carry":
            out["grasp"] = s.grasp_used
        self._check(fn(*head, *s.grasp_in, _ptr(goal), _ptr(out["path"]), _ptr(out["status"]), _ptr(out["poly"]), _ptr(out["n_poly"]),
                       _ptr(out["stats"]), *s.grasp_out, self._stream()))
        if R > 0:
            self._launched("plan")
        return out

    def plan_path_goals(self, probes, links, dof_qadr, qpos_goals, n_goals=None, env_idx=None, qpos_start=None, num_waypoints: int = 100,
                        max_nodes: int = 256, max_iterations: int = 2000, smooth_passes: int = 64, ignore_collision: bool = False, seed: int = 0,
                        resolution: float = 0.05, step: float = 0.3, margin: float = 0.0, max_distance: float = 1.0, skip_geoms=0,
                        self_model=None, carry=None) -> dict:
        """mir_plan_path_goals: plan_path() to a SET of goal configurations per row, in ONE launch.  `qpos_goals` (R, G, D), G = 1 ..
        spec.PLAN_MAX_GOALS; `n_goals` (R,) integers, None: G for every row -- the entries at or behind a row's count are never read.
        Every goal is judged (limits, then the collision tests of the call); the direct edge is tried to the valid ones, nearest to the
        start first; otherwise RRT-Connect runs with the goal tree started from all valid goals, and the plan ends at whichever goal the
        trees meet through (include/mirigid.h has the rule).  Everything else, `self_model` and `carry` included, as plan_path().
        -> the dict of plan_path() plus goal_index (R,) int32: the goal the plan ends at, -1 for a row without a plan, and goal_status
        (R, G) int32: spec.PLAN_STATUS per goal, -1 behind the row's count (and for every goal of a row whose start is refused).  A row
        without a valid goal has status NO_VALID_GOAL (spec.PLAN_GOAL_STATUS names the row statuses).  With one valid goal per row the result is that of plan_path() bit for bit."""
        s = _SphereCall(self, probes, links, dof_qadr, env_idx, qpos_start, self_model)
        R, D, new = s.R, s.D, s.new
        goals = torch.as_tensor(qpos_goals, device=self.device).to(torch.float32).contiguous()
        if goals.dim() != 3 or goals.shape[0] != R or goals.shape[2] != D:
            raise ValueError(f"qpos_goals must be ({R}, G, {D}), got {tuple(goals.shape)}")
        NG = int(goals.shape[1])
        gq = make_goal_query(NG)
        if n_goals is not None:
            n_goals = torch.as_tensor(n_goals, device=self.device).to(torch.int32).contiguous()
            if tuple(n_goals.shape) != (R,):
                raise ValueError(f"n_goals must be ({R},), got {tuple(n_goals.shape)}")
        s.collision(carry, True, num_waypoints=num_waypoints, max_nodes=max_nodes, max_iterations=max_iterations, smooth_passes=smooth_passes,
                    ignore_collision=ignore_collision, seed=seed, resolution=resolution, step=step, margin=margin, max_distance=max_distance,
                    skip_geoms=skip_geoms)
        W, i32 = max(int(num_waypoints), 0), torch.int32
        out = {"path": new(W, D), "status": new(dtype=i32), "poly": new(PLAN_MAX_POLY, D), "n_poly": new(dtype=i32), "stats": new(4, dtype=i32),
               "goal_index": new(dtype=i32), "goal_status": new(NG, dtype=i32)}
        if s.cq is not None:
            out["grasp"] = s.grasp_used
        head = s.head()  # (h, pq, sq, cq, ...: the goal query stands behind the carry query)
        self._check(self.lib.mir_plan_path_goals(*head[:4], C.byref(gq), *head[4:], *(s.grasp_in or (None,)), _ptr(goals), _ptr(n_goals),
                                                 _ptr(out["path"]), _ptr(out["status"]), _ptr(out["poly"]), _ptr(out["n_poly"]), _ptr(out["stats"]),
                                                 *(s.grasp_out or (None,)), _ptr(out["goal_index"]), _ptr(out["goal_status"]), self._stream()))
        if R > 0:
            self._launched("plan")
        return out

    def plan_path_pose(self, probes, links, dof_qadr, link_body: int, target_pos, target_quat=None, max_goals: int = 4, max_samples: int = 16,
                       dedup: float = 0.0, env_idx=None, qpos_start=None, num_waypoints: int = 100, max_nodes: int = 256,
                       max_iterations: int = 2000, smooth_passes: int = 64, ignore_collision: bool = False, seed: int = 0,
                       resolution: float = 0.05, step: float = 0.3, margin: float = 0.0, max_distance: float = 1.0, skip_geoms=0,
                       self_model=None, carry=None, **ik_options) -> dict:
        """mir_plan_path_pose: plan_path_goals() whose goal set is made inside the launch -- up to `max_goals` inverse-kinematics
        solutions of the pose `target_pos` (R, 3) / `target_quat` ((R, 4) wxyz; None: position only) of the body `link_body`, from up
        to `max_samples` seeds (the start, then random draws inside the joint limits, deterministic in `seed`), each kept when it
        converged (`ik_options`: those of inverse_kinematics()), lies inside the limits, is clear by the collision tests of the call
        and differs from every kept one by `dedup` (0: `resolution`) in some joint; then the goal-set planner on the kept ones, with no
        host decision in between (include/mirigid.h has the rule).  Everything else as plan_path_goals().
        -> its dict plus goals (R, G, D): the kept configurations, zeros behind them, n_goals (R,) int32 and goal_stats (R, 4) int32:
        samples tried, samples converged, converged but in collision or outside the limits, IK iterations.  A row that keeps no goal has
        status NO_VALID_GOAL; a target that is not finite, spec.CART_NOT_FINITE."""
        s = _SphereCall(self, probes, links, dof_qadr, env_idx, qpos_start, self_model)
        R, D, new = s.R, s.D, s.new
        tp = torch.as_tensor(target_pos, device=self.device).to(torch.float32).contiguous()
        if tuple(tp.shape) != (R, 3):
            raise ValueError(f"target_pos must be ({R}, 3), got {tuple(tp.shape)}")
        tq = None
        if target_quat is not None:
            tq = torch.as_tensor(target_quat, device=self.device).to(torch.float32).contiguous()
            if tuple(tq.shape) != (R, 4):
                raise ValueError(f"target_quat must be ({R}, 4), got {tuple(tq.shape)}")
        NG = int(max_goals)
        gq = make_pose_goal_query(link_body, NG, max_samples, dedup)
        s.collision(carry, True, num_waypoints=num_waypoints, max_nodes=max_nodes, max_iterations=max_iterations, smooth_passes=smooth_passes,
                    ignore_collision=ignore_collision, seed=seed, resolution=resolution, step=step, margin=margin, max_distance=max_distance,
                    skip_geoms=skip_geoms)
        o = self._ik_options(ik_options)
        W, i32, G_ = max(int(num_waypoints), 0), torch.int32, max(NG, 0)
        out = {"path": new(W, D), "status": new(dtype=i32), "poly": new(PLAN_MAX_POLY, D), "n_poly": new(dtype=i32), "stats": new(4, dtype=i32),
               "goal_index": new(dtype=i32), "goal_status": new(G_, dtype=i32), "goals": new(G_, D), "n_goals": new(dtype=i32),
               "goal_stats": new(4, dtype=i32)}
        if s.cq is not None:
            out["grasp"] = s.grasp_used
        head = s.head()
        self._check(self.lib.mir_plan_path_pose(*head[:4], C.byref(gq), *head[4:], *(s.grasp_in or (None,)), _ptr(tp), _ptr(tq), C.byref(o),
                                                _ptr(out["path"]), _ptr(out["status"]), _ptr(out["poly"]), _ptr(out["n_poly"]), _ptr(out["stats"]),
                                                *(s.grasp_out or (None,)), _ptr(out["goal_index"]), _ptr(out["goal_status"]), _ptr(out["goals"]),
                                                _ptr(out["n_goals"]), _ptr(out["goal_stats"]), self._stream()))
        if R > 0:
            self._launched("plan")
        return out

    def path_clearance(self, probes, links, dof_qadr, paths, env_idx=None, qpos_start=None, resolution: float = 0.05, margin: float = 0.0,
                       max_distance: float = 1.0, skip_geoms=0, self_model=None, carry=None) -> dict:
        """mir_path_clearance: the swept check of the trajectories `paths` (R, K, D) over the planned dofs `dof_qadr`, in ONE launch:
        every configuration the edge rule of mir_plan_path samples on every segment (at most `resolution` apart in every joint) is
        evaluated like signed_distance(row_min=True) on the sphere model.  -> seg_min (R, K-1), row_min (R,), row_first_blocked (R,)
        int32: the first segment whose minimum is < margin, -1: none.  Everything else as plan_path().  With `self_model`
        (mir_path_clearance_self): also seg_self_min (R, K-1) and row_self_min (R,), and row_first_blocked counts either test.  With
        `carry` (as in plan_path(): mir_path_clearance_carry) the carried body's probes ride along, and the result gains grasp (R, 7)."""
        s = _SphereCall(self, probes, links, dof_qadr, env_idx, qpos_start, self_model)
        R, new = s.R, s.new
        paths, K = self._rows_kd(paths, "paths", R, s.D, kmin=2)
        s.collision(carry, True, resolution=resolution, margin=margin, max_distance=max_distance, skip_geoms=skip_geoms)
        out = {"seg_min": new(K - 1), "row_min": new(), "row_first_blocked": new(dtype=torch.int32)}
        if s.sq is not None:
            out["seg_self_min"], out["row_self_min"] = new(K - 1), new()
        fn, head, form = s.symbol("mir_path_clearance")
        if form == "_carry":
            out["grasp"] = s.grasp_used
        so = lambda k: (_ptr(out.get(k)),) if form else ()  # noqa: E731  (the plain entry point has no self outputs)
        self._check(fn(*head, *s.grasp_in, _ptr(paths), K, _ptr(out["seg_min"]), *so("seg_self_min"), _ptr(out["row_min"]), *so("row_self_min"),
                       _ptr(out["row_first_blocked"]), *s.grasp_out, self._stream()))
        if R > 0:
            self._launched("plan")
        return out

    def certify_path(self, probes, links, dof_qadr, paths, env_idx=None, qpos_start=None, margin: float = 0.0, tol: float = 0.002,
                     guard: float = 1e-5, max_depth: int = 12, max_evaluations: int = 4096, bracket: bool = False, max_leaves: int = 0,
                     max_distance: float = 1.0, skip_geoms=0, ignore_collision: bool = False, self_model=None, carry=None, grasp=None) -> dict:
        """mir_certify_path: the CONTINUOUS minimum clearance of the trajectories `paths` (R, K, D) over the planned dofs `dof_qadr`,
        bracketed per segment in ONE launch.  Where path_clearance() judges samples of a segment, this call judges all of it: the signed
        distance is 1-Lipschitz in a sphere's centre and a centre moves no faster than the kinematic chain allows, so one evaluation
        bounds the clearance on a whole interval, which is bisected where the bound does not decide (include/mirigid.h has the rule).
        `tol`: the width a bracket is closed to; `guard`: subtracted from every bound for the float32 error of an evaluation; `max_depth`
        (0 .. 20) and `max_evaluations` per row bound the work; `bracket`: close every bracket to `tol` instead of stopping at "clear of
        `margin`"; `max_leaves`: the accepted leaves kept per row.  Everything else as path_clearance().
        `self_model` and `carry` (the dicts of path_clearance(); `grasp` (R, 7) may also be given here in place of carry["grasp"]):
        mir_certify_path_self / mir_certify_path_carry -- the self clearance (the lowest distance of an enabled pair of spheres, capped
        at self_model["max_distance"]) is bracketed over the whole of every segment too, by a bound on the RELATIVE speed of two spheres
        (only the joints below the lowest common ancestor of their links count), and the carried body's spheres ride along in both
        tests.  The result gains seg_self_lower, seg_self_upper (R, K-1), row_self_lower, row_self_upper (R,) (+inf without a self
        model) and grasp (R, 7) (NaN without a carried body); a status then speaks for both tests.
        -> dict of fresh device tensors: seg_lower, seg_upper (R, K-1), seg_status (R, K-1) int32 (spec.CERT_STATUS), row_lower,
        row_upper (R,), row_status, row_first (R,) int32 (the first segment that is not CLEAR, -1: none), stats (R, 4) int32:
        evaluations, leaves, deepest level, segments finished; with max_leaves > 0 also leaves (R, max_leaves, 3) int32: segment, level,
        index, -1 behind the row's count.  The call changes nothing a later call can see."""
        s = _SphereCall(self, probes, links, dof_qadr, env_idx, qpos_start)
        R, new, i32 = s.R, s.new, torch.int32
        paths, K = self._rows_kd(paths, "paths", R, s.D, kmin=2)
        q = make_cert_query(K, tol, guard, max_depth, max_evaluations, bracket, max_leaves)
        s.self_model(self_model)   # (behind the two above: the order of this method's errors)
        s.collision(ignore_collision=ignore_collision, margin=margin, max_distance=max_distance, skip_geoms=skip_geoms)
        out = {"seg_lower": new(K - 1), "seg_upper": new(K - 1), "seg_status": new(K - 1, dtype=i32), "row_lower": new(), "row_upper": new(),
               "row_status": new(dtype=i32), "row_first": new(dtype=i32), "stats": new(4, dtype=i32)}
        if int(max_leaves) > 0:
            out["leaves"] = torch.full((R, int(max_leaves), 3), -1, dtype=i32, device=self.device)
        if self_model is not None or carry is not None or grasp is not None:
            if grasp is not None:
                if carry is None:
                    raise ValueError("grasp belongs to carry, which is None")
                carry = {**carry, "grasp": grasp}
            inf = lambda *shape: torch.full((R, *shape), float("inf"), dtype=torch.float32, device=self.device)  # noqa: E731
            mk = new if s.sq is not None else inf
            out.update(seg_self_lower=mk(K - 1), seg_self_upper=mk(K - 1), row_self_lower=mk(), row_self_upper=mk())
            s.carry(carry, True)
            out["grasp"] = s.grasp_used if carry is not None else torch.full((R, 7), float("nan"), dtype=torch.float32, device=self.device)
        if R > 0:   # (without rows there is nothing to point at)
            fn, head, form = s.symbol("mir_certify_path", q)
            # (the plain entry point has no self outputs; without a self model the other two get none either: the +inf stay)
            so = lambda k: (_ptr(out[k]) if s.sq is not None else None,) if form else ()  # noqa: E731
            self._check(fn(*head, *s.grasp_in, _ptr(paths), _ptr(out["seg_lower"]), _ptr(out["seg_upper"]), *so("seg_self_lower"),
                           *so("seg_self_upper"), _ptr(out["seg_status"]), _ptr(out["row_lower"]), _ptr(out["row_upper"]), *so("row_self_lower"),
                           *so("row_self_upper"), _ptr(out["row_status"]), _ptr(out["row_first"]), *s.grasp_out, _ptr(out.get("leaves")),
                           _ptr(out["stats"]), self._stream()))
            self._launched("cert")
        return out

    def cartesian_path(self, probes, links, dof_qadr, link_body: int, target_pos, target_quat=None, env_idx=None, qpos_start=None,
                       max_pos_step: float = 0.01, max_rot_step: float = 0.05, jump_threshold: float = 0.5, max_points: int = 256,
                       num_waypoints: int = 0, ignore_collision: bool = False, resolution: float = 0.05, margin: float = 0.0,
                       max_distance: float = 1.0, skip_geoms=0, self_model=None, carry=None, **ik_options) -> dict:
        """mir_cartesian_path: for the envs `env_idx` (None: all), ONE launch takes the body `link_body` from where it is at
        `qpos_start` ((R, nq) full rows; None: the current state) along the straight segments to `target_pos` (R, K, 3) -- with
        `target_quat` (R, K, 4) wxyz the orientation is interpolated along the shorter arc, without it it is free -- by inverse
        kinematics at samples at most `max_pos_step` m and `max_rot_step` rad apart, each seeded with the one before; a sample whose IK
        does not converge, that moves a planned dof by more than `jump_threshold`, or whose edge from the sample before is not clear
        (the sphere model, `resolution`, `margin`, `skip_geoms`, `self_model` and `carry` = dict(body, link) exactly as in
        path_clearance(); the grasp is taken from the start row) ends the row, which keeps what it achieved (include/mirigid.h has the
        rule).  Only the planned dofs `dof_qadr` on the chain to the link move.  `ik_options`: those of inverse_kinematics().
        -> dict of fresh device tensors: points (R, P, D) with P = max_points (the start, the accepted samples, then the last one
        repeated), n_points (R,) int32, fraction (R,) = accepted samples / all samples, status (R,) int32 (spec.CART_STATUS), stats
        (R, 4) int32: IK iterations, configurations checked, samples S, the segment that failed or -1; with num_waypoints = W >= 2 also
        path (R, W, D): the points resampled at equal steps of their index.  The call changes nothing a later call can see."""
        s = _SphereCall(self, probes, links, dof_qadr, env_idx, qpos_start, self_model)
        R, D, new = s.R, s.D, s.new
        tp, K = self._rows_kd(target_pos, "target_pos", R, 3, kmin=1)
        tq = None
        if target_quat is not None:
            tq = torch.as_tensor(target_quat, device=self.device).to(torch.float32).contiguous()
            if tuple(tq.shape) != (R, K, 4):
                raise ValueError(f"target_quat must be ({R}, {K}, 4), got {tuple(tq.shape)}")
        P, W = int(max_points), int(num_waypoints)
        q = make_cart_query(link_body, K, P, W, max_pos_step, max_rot_step, jump_threshold)
        s.collision(carry, False, ignore_collision=ignore_collision, resolution=resolution, margin=margin, max_distance=max_distance,
                    skip_geoms=skip_geoms)
        o = self._ik_options(ik_options)
        out = {"points": new(max(P, 0), D), "n_points": new(dtype=torch.int32), "fraction": new(), "status": new(dtype=torch.int32),
               "stats": new(4, dtype=torch.int32)}
        if W > 0:
            out["path"] = new(W, D)
        if R > 0:   # (without rows there is nothing to point at)
            self._check(self.lib.mir_cartesian_path(*s.head(q), _ptr(tp), _ptr(tq), C.byref(o), _ptr(out["points"]), _ptr(out["n_points"]),
                                                    _ptr(out["fraction"]), _ptr(out["status"]), _ptr(out.get("path")), _ptr(out["stats"]), self._stream()))
            self._launched("cart")
        return out

    def blend_path(self, probes, links, dof_qadr, poly, n_poly=None, env_idx=None, qpos_start=None, max_deviation: float = 0.05,
                   blend_points: int = 8, max_shrinks: int = 4, max_points=None, num_waypoints: int = 0, ignore_collision: bool = False,
                   resolution: float = 0.05, margin: float = 0.0, max_distance: float = 1.0, skip_geoms=0, self_model=None, carry=None) -> dict:
        """mir_blend_path: for the envs `env_idx` (None: all), ONE launch rounds the interior corners of the joint-space polylines `poly`
        (R, K, D) -- K <= 128 nodes over the planned dofs `dof_qadr`, as plan_path()["poly"] holds them, `n_poly` (R,) the count of valid
        leading nodes (None: K); repeated nodes are dropped -- by quadratic Bezier blends that stay within `max_deviation` (L2 over the
        dofs) of their corner, `blend_points` chords each.  Every blend is checked like an edge of plan_path() (the sphere model,
        `resolution`, `margin`, `skip_geoms`, `self_model` and `carry` = dict(body, link) exactly as in path_clearance(); the grasp is
        taken from the start row, `qpos_start` (R, nq) or the current state); a blocked blend is halved up to `max_shrinks` times and
        then left sharp (include/mirigid.h has the rule).  The straight remainders of the input's segments are not checked again.
        -> dict of fresh device tensors: points (R, P, D) with P = `max_points` (None: the worst case 2 + (K - 2)(blend_points + 1); the
        smoothed path, then its last point repeated), n_points (R,) int32, status (R,) int32 (spec.BLEND_STATUS), blend_len (R, 128): the
        accepted half-length at each input node, stats (R, 4) int32: nodes kept, corners blended, corners left sharp, configurations
        checked; with num_waypoints = W >= 2 also path (R, W, D): the points resampled at equal arc length.  A row that fails holds its
        first node everywhere.  The call changes nothing a later call can see."""
        s = _SphereCall(self, probes, links, dof_qadr, env_idx, qpos_start, self_model)
        R, D, new = s.R, s.D, s.new
        poly, K = self._rows_kd(poly, "poly", R, D)
        if n_poly is not None:
            n_poly = torch.as_tensor(n_poly, device=self.device).to(torch.int32).contiguous()
            if tuple(n_poly.shape) != (R,):
                raise ValueError(f"n_poly must be ({R},), got {tuple(n_poly.shape)}")
        W = int(num_waypoints)
        q = make_blend_query(K, max_deviation, blend_points, max_shrinks, max_points, W)
        P = int(q.max_points)
        s.collision(carry, False, ignore_collision=ignore_collision, resolution=resolution, margin=margin, max_distance=max_distance,
                    skip_geoms=skip_geoms)
        out = {"points": new(max(P, 0), D), "n_points": new(dtype=torch.int32), "status": new(dtype=torch.int32), "blend_len": new(PLAN_MAX_POLY),
               "stats": new(4, dtype=torch.int32)}
        if W > 0:
            out["path"] = new(W, D)
        if R > 0:   # (without rows there is nothing to point at)
            self._check(self.lib.mir_blend_path(*s.head(q), _ptr(poly), _ptr(n_poly), _ptr(out["points"]), _ptr(out["n_points"]), _ptr(out["status"]),
                                                _ptr(out.get("path")), _ptr(out["blend_len"]), _ptr(out["stats"]), self._stream()))
            self._launched("blend")
        return out

    def optimize_path(self, probes, links, dof_qadr, paths, env_idx=None, qpos_start=None, smooth_weight=None, obstacle_weight=None,
                      activation=None, step=None, max_iterations=None, max_halvings=None, ftol=None, ignore_collision: bool = False,
                      resolution: float = 0.05, margin: float = 0.0, max_distance: float = 1.0, skip_geoms=0, self_model=None, carry=None,
                      grad0: bool = False) -> dict:
        """mir_optimize_path: for the envs `env_idx` (None: all), ONE launch takes each row's joint path `paths` (R, K, D) -- 3 <= K <= 128
        waypoints over the planned dofs `dof_qadr`, the layout plan_path()["path"] and blend_path()["path"] have -- as a seed and moves
        its interior waypoints by covariant gradient descent (CHOMP's update) with a backtracking line search on U = `smooth_weight` S +
        `obstacle_weight` O: S the discrete integral of |q'|^2, O the sum over the interior waypoints and the spheres of a cost that is
        zero from `activation` metres beyond `margin` outwards, quadratic in that band and linear inside the margin (include/mirigid.h
        has the rule).  `step`: the first step length of every iteration, halved up to `max_halvings` times while U does not fall;
        `max_iterations`; `ftol`: the relative decrease of U below which a row has converged.  None: spec.OPT_DEFAULTS.  The result is
        swept like an edge of plan_path() (the sphere model, `resolution`, `margin`, `skip_geoms`, `self_model` and `carry` =
        dict(body, link) exactly as in path_clearance(); the grasp is taken from the start row, `qpos_start` (R, nq) or the current
        state): a row whose result does not pass returns its input, bit for bit.  The ends never move.
        -> dict of fresh device tensors: path (R, K, D), status (R,) int32 (spec.OPT_STATUS), cost (R, 4): S and O of the input, S and O
        of what the descent reached, stats (R, 6) int32: iterations, accepted steps, halvings, configurations evaluated in the descent,
        configurations checked in the sweep, stop (spec.OPT_STOP), min_d (R,): the lowest distance beyond the margin of a sphere at an
        interior waypoint of `path`; with `grad0` also grad0 (R, K, D): the gradient of U at the input (a test hook).  The call changes
        nothing a later call can see."""
        s = _SphereCall(self, probes, links, dof_qadr, env_idx, qpos_start, self_model)
        R, D, new = s.R, s.D, s.new
        paths, K = self._rows_kd(paths, "paths", R, D)
        q = make_opt_query(K, smooth_weight, obstacle_weight, activation, step, max_iterations, max_halvings, ftol)
        s.collision(carry, False, ignore_collision=ignore_collision, resolution=resolution, margin=margin, max_distance=max_distance,
                    skip_geoms=skip_geoms)
        out = {"path": new(K, D), "status": new(dtype=torch.int32), "cost": new(4), "stats": new(6, dtype=torch.int32), "min_d": new()}
        if grad0:
            out["grad0"] = new(K, D)
        if R > 0:   # (without rows there is nothing to point at)
            self._check(self.lib.mir_optimize_path(*s.head(q), _ptr(paths), K, _ptr(out["path"]), _ptr(out["status"]), _ptr(out["cost"]),
                                                   _ptr(out["stats"]), _ptr(out["min_d"]), _ptr(out.get("grad0")), self._stream()))
            self._launched("opt")
        return out

    def retime_path(self, paths, vmax, amax, dt, num_samples: int = 0, max_path_speed=None, extra=None, velocity: bool = False) -> dict:
        """mir_retime_path: the joint paths `paths` (R, K, D) -- K waypoints of D <= 16 dofs per row, as plan_path()["path"] holds them --
        as time-optimal trajectories within `vmax` and `amax` (a scalar or D values, shared by the rows), in ONE launch (include/mirigid.h
        has the algorithm: TOPP-RA on the caller's waypoints, repeated waypoints dropped).  `dt`: the sample period; `num_samples` = T:
        the samples written per row (0: none); `max_path_speed` in waypoints per second (None: 1 / dt, at most one waypoint per
        sample); `extra` = (ea, eb, elo, ehi), each (R, K, E): E more rows elo <= ea u + eb x <= ehi per waypoint (torque limits).
        -> dict of fresh device tensors on the current stream: x, t (R, K) squared path speed and time at the caller's waypoints,
        duration (R,), status (R,) int32 (spec.RETIME_STATUS), n_samples (R,) int32 = ceil(duration / dt) + 1, and with T > 0 samples
        (R, T, D) -- targets at n dt, the end configuration from the duration on -- and, with `velocity`, sample_vel (R, T, D).  A row
        with n_samples > T is TRUNCATED (x, t, duration valid); a row that fails otherwise holds its start T times.  The call reads no
        state and changes nothing a later call can see."""
        paths = torch.as_tensor(paths, device=self.device).to(torch.float32).contiguous()
        if paths.dim() != 3:
            raise ValueError(f"paths must be (R, K, D), got {tuple(paths.shape)}")
        R, K, D = (int(v) for v in paths.shape)
        ex, E = [None] * 4, 0
        if extra is not None:
            ex = [torch.as_tensor(e, device=self.device).to(torch.float32).contiguous() for e in extra]
            if len(ex) != 4 or any(e.dim() != 3 or tuple(e.shape) != (R, K, int(ex[0].shape[-1])) for e in ex):
                raise ValueError(f"extra must be four ({R}, {K}, E) tensors (ea, eb, elo, ehi), got {[tuple(e.shape) for e in ex]}")
            E = int(ex[0].shape[2])
            if E == 0:
                ex = [None] * 4
        T = int(num_samples)
        q = make_retime_query(D, K, vmax, amax, dt, T, max_path_speed, E)
        new = self._row_alloc(R)
        out = {"x": new(K), "t": new(K), "duration": new(), "status": new(dtype=torch.int32), "n_samples": new(dtype=torch.int32)}
        if T > 0:
            out["samples"] = new(T, D)
            if velocity:
                out["sample_vel"] = new(T, D)
        if R > 0:   # (without rows there is nothing to point at)
            self._check(self.lib.mir_retime_path(self.h, C.byref(q), R, _ptr(paths), *(_ptr(e) for e in ex), _ptr(out["x"]), _ptr(out["t"]),
                                                 _ptr(out["duration"]), _ptr(out["status"]), _ptr(out["n_samples"]), _ptr(out.get("samples")),
                                                 _ptr(out.get("sample_vel")), self._stream()))
            self._launched("retime")
        return out

    def render(self, cam: MirCameraSpec, vis: MirVisualSpec, mode: int = 0, env_offset: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """RGB8 images of the current state (mir_render): (B,H,W,3) per-env, or (H,W,3) in global mode."""
        shape = (cam.height, cam.width, 3) if mode == 1 else (self.num_envs, cam.height, cam.width, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous uint8 tensor of shape {shape}")
        off = None
        if env_offset is not None:
            off = self._f32(env_offset, 3)
        self._check(self.lib.mir_render(self.h, C.byref(cam), C.byref(vis), int(mode), _ptr(off), _ptr(out), self._stream()))
        return out

    @property
    def spec_active(self) -> bool:
        """True when this scene runs the scene-specialised instantiation of the 16-lane kernel (mir_debug_spec_active)."""
        return bool(self.lib.mir_debug_spec_active(self.h))

    def early_mask_stats(self, reset: bool = False):
        """(workgroup-launches that sent their terminated bytes from inside the solver loop, workgroup-launches whose early bytes
        differed from the integrated state: must be 0 -- the library also fails the next call with MIR_E_MASK) -- mir_debug_early_mask_stats."""
        out = (C.c_uint32 * 2)()
        self._check(self.lib.mir_debug_early_mask_stats(self.h, out, 1 if reset else 0, self._stream()))
        return int(out[0]), int(out[1])

    def set_exact_contacts(self, on=True) -> None:
        """mir_set_exact_contacts: from now on the begin / end step path defers every env whose narrowphase finds more contact
        points than the 16-lane kernel keeps (16) and steps it with 48 points, never thinned below that -- on the list instantiation of
        the 16-lane kernel (three contacts per lane), on the wave-per-env kernel what exceeds that too; the other envs are computed as
        before.  step() / step_fused() then wait for their step; step_packed() / rollout*() are refused.
        on="all" (tests): EVERY env of every step takes the deferred envs' route -- the twin a deferred env is compared with."""
        self._check(self.lib.mir_set_exact_contacts(self.h, C.byref(self.spec), 2 if on == "all" else (1 if on else 0)))

    def exact_route(self) -> dict:
        """mir_get_exact_route: deferred env-steps handed to the list instantiation / env-steps stepped by the wave-per-env kernel /
        heavy steps / two-launch steps of overflow runs."""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.mir_get_exact_route(self.h, out))
        return {"list_env_steps": int(out[0]), "wave_env_steps": int(out[1]), "heavy_steps": int(out[2]), "big_steps": int(out[3])}

    @property
    def exact_contacts(self) -> bool:
        return bool(self.lib.mir_get_exact_contacts(self.h))

    def exact_stats(self, reset: bool = False) -> dict:
        """mir_get_exact_stats: steps closed by step_end, steps that had deferred envs, deferred env-steps, most deferred envs in a step."""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.mir_get_exact_stats(self.h, out, 1 if reset else 0))
        return {"steps": int(out[0]), "overflow_steps": int(out[1]), "overflow_env_steps": int(out[2]), "overflow_envs_max": int(out[3])}

    @property
    def early_mask(self) -> bool:
        """True while mir_step_begin launches may send their terminated bytes early (mir_get_early_mask)."""
        return bool(self.lib.mir_get_early_mask(self.h))

    @property
    def state_version(self) -> int:
        """mir_get_state_version: advances with every call that moves the bodies (steps, resets, state writes)."""
        return int(self.lib.mir_get_state_version(self.h))

    def debug_render_path(self, generic: bool = False, strip_rows: int = 0) -> None:
        """mir_debug_render_path: force the generic pixel kernel / override the strip height for the following renders."""
        self._check(self.lib.mir_debug_render_path(self.h, 1 if generic else 0, int(strip_rows)))

    def render_cams(self, cam: MirCameraSpec, vis: MirVisualSpec, cam_pos, cam_lookat, cam_up=None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(B,H,W,3) RGB8 images, env i seen from its own camera cam_pos[i] -> cam_lookat[i] (mir_render_cams)."""
        shape = (self.num_envs, cam.height, cam.width, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        p, l = self._f32(cam_pos, 3), self._f32(cam_lookat, 3)
        u = None if cam_up is None else self._f32(cam_up, 3)
        self._check(self.lib.mir_render_cams(self.h, C.byref(cam), C.byref(vis), _ptr(p), _ptr(l), _ptr(u), _ptr(out), self._stream()))
        return out

    def render_outputs(self, cam: MirCameraSpec, vis: MirVisualSpec, mode: int = 0, env_offset: Optional[torch.Tensor] = None,
                       cam_pos=None, cam_lookat=None, cam_up=None, rgb: bool = True, depth: bool = False, segmentation: bool = False,
                       normal: bool = False, seg_level: str = "link", out=None):
        """(rgb, depth, segmentation, normal) device tensors of the current state, Genesis's order (mir_render_outputs); None for a
        channel not asked for.  Shapes (B,H,W[,3]) per env, (H,W[,3]) with mode=1.  rgb: uint8, what render() / render_cams() draw;
        depth: float32 planar camera-z metres, 0 = sky; segmentation: int32 body ("link") or geom ("geom") index, -1 = sky; normal:
        uint8 world-frame normal as round((n + 1) / 2 * 255), sky 0 0 0.  cam_pos / cam_lookat (B,3): per-env cameras as in
        render_cams() (mode 0 only).  out: optional 4-tuple of tensors (or None) to write into."""
        if seg_level not in SEG_LEVELS:
            raise ValueError(f"seg_level must be one of {sorted(SEG_LEVELS)}, got {seg_level!r}")
        if cam_pos is not None and mode != 0:
            raise ValueError("per-env cameras (cam_pos) need mode=0")
        if (cam_pos is None) != (cam_lookat is None):
            raise ValueError("cam_pos and cam_lookat go together")
        base = (cam.height, cam.width) if mode == 1 else (self.num_envs, cam.height, cam.width)
        given = tuple(out) if out is not None else (None,) * 4
        if len(given) != 4:
            raise ValueError("out must be a 4-tuple (rgb, depth, segmentation, normal)")

        def buf(k, want, shape, dtype):
            if not want:
                return None
            t = given[k]
            if t is None:
                return torch.empty(shape, dtype=dtype, device=self.device)
            if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
                raise ValueError(f"out[{k}] must be a contiguous {dtype} tensor of shape {shape}")
            return t

        r = buf(0, rgb, base + (3,), torch.uint8)
        d = buf(1, depth, base, torch.float32)
        sg = buf(2, segmentation, base, torch.int32)
        n = buf(3, normal, base + (3,), torch.uint8)
        if r is None and d is None and sg is None and n is None:
            raise ValueError("render_outputs: no channel asked for")
        off = None if env_offset is None or cam_pos is not None else self._f32(env_offset, 3)
        p = None if cam_pos is None else self._f32(cam_pos, 3)
        l = None if cam_lookat is None else self._f32(cam_lookat, 3)
        u = None if cam_up is None else self._f32(cam_up, 3)
        o = MirRenderOutputs(C.sizeof(MirRenderOutputs), SEG_LEVELS[seg_level], _ptr(r), _ptr(d), _ptr(sg), _ptr(n))
        self._check(self.lib.mir_render_outputs(self.h, C.byref(cam), C.byref(vis), int(mode), _ptr(off), _ptr(p), _ptr(l), _ptr(u),
                                                C.byref(o), self._stream()))
        return r, d, sg, n

    def _ik_options(self, opts):
        """MirIkOptions of a call: the defaults with `opts` over them (the object for no opts is made once and kept)"""
        o = self.__dict__.get("_ik_default")
        if opts or o is None:
            o = MirIkOptions(**{**IK_DEFAULTS, **opts})
            if not opts:
                self._ik_default = o
        return o

    @staticmethod
    def _ik_rows(env_idx, n, flags, col0, ncols):
        """MirIkRows: n rows for the envs `env_idx` (an int64 device tensor, or None: row k = env k)"""
        return MirIkRows(None if env_idx is None else env_idx.data_ptr(), n, int(flags), int(col0), int(ncols))

    def inverse_kinematics(self, link_body: int, pos, quat=None, init_qpos=None, return_error: bool = False, **opts):
        """Batched damped-least-squares IK (mir_inverse_kinematics): (B, n_arm) joint positions that bring body
        `link_body` to pos (B,3) / quat (B,4 wxyz, optional).  Seed = init_qpos or the scene's current joint positions."""
        p = self._f32(pos, 3)
        q = None if quat is None else self._f32(quat, 4)
        init = None if init_qpos is None else self._f32(init_qpos, self.n_arm)
        o = self._ik_options(opts)
        out, err = self.empty(self.n_arm), self.empty(2)
        self._check(self.lib.mir_inverse_kinematics(self.h, int(link_body), _ptr(p), _ptr(q), _ptr(init), C.byref(o), _ptr(out), _ptr(err),
                                                    self._stream()))
        return (out, err) if return_error else out

    def inverse_kinematics_rows(self, link_body: int, pos, quat, init_qpos, env_idx, flags: int, init_col0: int = 0, init_ncols: int = 0,
                                return_error: bool = False, **opts):
        """mir_inverse_kinematics_rows: the solver for the rows `env_idx` (int64 device tensor, or None: every env) in ONE launch.
        pos / quat / init_qpos: contiguous float32 device tensors addressed as `flags` say (spec.IK_*); -> (n_rows, n_arm)[, (n_rows, 2)]."""
        n = self.num_envs if env_idx is None else int(env_idx.numel())
        o = self._ik_options(opts)
        rows = self._ik_rows(env_idx, n, flags, init_col0, init_ncols)
        out = torch.empty((n, self.n_arm), dtype=torch.float32, device=self.device)
        err = torch.empty((n, 2), dtype=torch.float32, device=self.device) if return_error else None
        self._check(self.lib.mir_inverse_kinematics_rows(self.h, int(link_body), C.byref(rows), _ptr(pos), _ptr(quat), _ptr(init_qpos), C.byref(o),
                                                         _ptr(out), _ptr(err), self._stream()))
        return (out, err) if return_error else out

    def inverse_kinematics_multilink(self, links, poss, quats=None, init_qpos=None, env_idx=None, flags: int = 0, init_col0: int = 0,
                                     init_ncols: int = 0, pos_mask=(True, True, True), rot_mask=(True, True, True), dof_mask=None,
                                     max_samples: int = 1, seed: int = 0, return_error: bool = False, return_info: bool = False, **opts):
        """mir_inverse_kinematics_multilink: damped-least-squares IK for up to four links at once (body indices `links`), with axis masks
        shared by the links, a mask over the n_arm joint columns that may move (None: every joint on a chain) and `max_samples` restarts,
        for the rows `env_idx` (int64 device tensor, or None: every env) in ONE launch of a kernel of its own.  poss (n or B, L, 3),
        quats (n or B, L, 4 | L, 4 with IK_QUAT_ONE | None), init_qpos: float32 tensors addressed as `flags` say (spec.IK_*), made
        contiguous here.  -> (n, n_arm)[, err (n, L, 2)][, info dict: iters (n) int32 summed over the samples, sample (n) int32].
        The scene state is read and never written."""
        q = make_ik_multi(links, pos_mask, rot_mask, dof_mask, max_samples, seed, self.n_arm)
        L = q.n_links
        idx = None if env_idx is None else torch.as_tensor(env_idx, device=self.device).long().reshape(-1).contiguous()
        n = self.num_envs if idx is None else int(idx.numel())
        q.rows = self._ik_rows(idx, n, flags, init_col0, init_ncols)

        def dev(t, width, name, by_env, one=False):
            if t is None:
                return None
            t = torch.as_tensor(t, device=self.device).to(torch.float32).contiguous()
            want = 1 if one else (self.num_envs if by_env else n)
            if t.numel() != want * width:
                raise ValueError(f"{name} must hold {want} x {width} values, got {tuple(t.shape)}")
            return t

        p = dev(poss, L * 3, "poss", flags & IK_POS_BY_ENV)
        if p is None:
            raise ValueError("inverse_kinematics_multilink needs target positions")
        qq = dev(quats, L * 4, "quats", flags & IK_QUAT_BY_ENV, bool(flags & IK_QUAT_ONE))
        iq = dev(init_qpos, init_ncols or self.n_arm, "init_qpos", flags & IK_INIT_BY_ENV)
        o = self._ik_options(opts)
        out = torch.empty((n, self.n_arm), dtype=torch.float32, device=self.device)
        err = torch.empty((n, L, 2), dtype=torch.float32, device=self.device) if return_error else None
        iters = torch.empty((n,), dtype=torch.int32, device=self.device) if return_info else None
        sample = torch.empty((n,), dtype=torch.int32, device=self.device) if return_info else None
        if n > 0:   # (no rows: nothing to launch, and an empty tensor has no address to pass)
            self._check(self.lib.mir_inverse_kinematics_multilink(self.h, C.byref(q), _ptr(p), _ptr(qq), _ptr(iq), C.byref(o), _ptr(out), _ptr(err),
                                                                  _ptr(iters), _ptr(sample), self._stream()))
            self._launched("ik_multilink")
        res = (out,) + ((err,) if return_error else ()) + (({"iters": iters, "sample": sample},) if return_info else ())
        return res if len(res) > 1 else out
