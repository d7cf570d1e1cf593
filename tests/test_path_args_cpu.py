"""The pure Python helpers the sphere-model path methods share, against stubs with device = cpu (no library is loaded, no kernel runs):
MirScene._rows_kd, the (R, K >= kmin, D) check of `paths` / `poly` / `target_pos`; EntityView._path_rows, the path normaliser of the
(K, R, n) layout plan_path() returns and of blend_path's (R, K, n); EntityView._drop_env_axis.  The messages are the ones the methods
raised before they shared a helper, written out here."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gym_genesis.backend.lib import MirScene
from gym_genesis.tasks.views import EntityView

CPU = torch.device("cpu")
SCENE = SimpleNamespace(device=CPU)
D = 3


def entity(unbatched: bool):
    return SimpleNamespace(_mir=SimpleNamespace(device=CPU), _qcols=list(range(D)), unbatched=unbatched)


# ---- MirScene._rows_kd(t, name, R, D, kmin): paths of path_clearance / certify_path (K >= 2), paths of optimize_path and poly of blend_path
# (any K), target_pos of cartesian_path (K >= 1, D = 3)
@pytest.mark.parametrize("name, kmin, R, K", [("paths", 2, 1, 2), ("paths", 2, 4, 5), ("paths", 0, 1, 0), ("poly", 0, 2, 1), ("target_pos", 1, 1, 1)])
def test_rows_kd_accepts(name, kmin, R, K):
    src = np.arange(R * K * D, dtype=np.float64).reshape(R, K, D)
    t, k = MirScene._rows_kd(SCENE, src, name, R, D, kmin)
    assert k == K and tuple(t.shape) == (R, K, D) and t.dtype == torch.float32 and t.is_contiguous() and t.device == CPU
    assert np.array_equal(t.numpy(), src.astype(np.float32))
    # (a transposed view comes back contiguous)
    t2, _ = MirScene._rows_kd(SCENE, torch.zeros((D, K, R)).permute(2, 1, 0), name, R, D, kmin)
    assert tuple(t2.shape) == (R, K, D) and t2.is_contiguous()


@pytest.mark.parametrize("name, kmin, R, shape, message", [
    ("paths", 2, 1, (1, 1, 3), "paths must be (1, K >= 2, 3), got (1, 1, 3)"),          # K = kmin - 1
    ("paths", 2, 4, (4, 5, 2), "paths must be (4, K >= 2, 3), got (4, 5, 2)"),          # wrong D
    ("paths", 2, 4, (3, 5, 3), "paths must be (4, K >= 2, 3), got (3, 5, 3)"),          # wrong R
    ("paths", 2, 1, (5, 3), "paths must be (1, K >= 2, 3), got (5, 3)"),                # 2-D
    ("paths", 0, 2, (2, 4, 4), "paths must be (2, K, 3), got (2, 4, 4)"),               # optimize_path: no bound on K here
    ("poly", 0, 2, (4, 3), "poly must be (2, K, 3), got (4, 3)"),
    ("poly", 0, 1, (1, 4, 2), "poly must be (1, K, 3), got (1, 4, 2)"),
    ("target_pos", 1, 1, (1, 0, 3), "target_pos must be (1, K >= 1, 3), got (1, 0, 3)"),  # K = kmin - 1
    ("target_pos", 1, 2, (2, 3), "target_pos must be (2, K >= 1, 3), got (2, 3)"),
])
def test_rows_kd_refuses(name, kmin, R, shape, message):
    with pytest.raises(ValueError) as e:
        MirScene._rows_kd(SCENE, np.zeros(shape, np.float32), name, R, D, kmin)
    assert str(e.value) == message


# ---- EntityView._path_rows(path, R, kmin, name, axis, letter="K") -> (R, K, n)
@pytest.mark.parametrize("unbatched", [False, True])
@pytest.mark.parametrize("axis, kmin, K", [(0, 2, 2), (0, 2, 5), (0, 3, 3), (1, 0, 1), (1, 0, 4)])
def test_path_rows_accepts(unbatched, axis, kmin, K):
    for R in ((1,) if unbatched else (1, 3)):
        rows = np.arange(R * K * D, dtype=np.float64).reshape(R, K, D)          # what must come back
        given = rows if axis else rows.transpose(1, 0, 2)
        out = EntityView._path_rows(entity(unbatched), given, R, kmin, "path", axis)
        assert tuple(out.shape) == (R, K, D) and out.dtype == torch.float32 and out.is_contiguous()
        assert np.array_equal(out.numpy(), rows.astype(np.float32))
        if unbatched:   # (the env axis may be left out)
            out = EntityView._path_rows(entity(True), rows[0], 1, kmin, "path", axis)
            assert tuple(out.shape) == (1, K, D) and np.array_equal(out.numpy(), rows.astype(np.float32))


@pytest.mark.parametrize("unbatched, R, kmin, name, axis, letter, shape, message", [
    (False, 1, 2, "path", 0, "K", (1, 1, 3), "path must be (K >= 2, 1, 3), got (1, 1, 3)"),      # K = kmin - 1, R = 1
    (True, 1, 2, "path", 0, "K", (1, 3), "path must be (K >= 2, 1, 3), got (1, 1, 3)"),          # the same without the env axis
    (False, 1, 2, "path", 0, "K", (4, 3), "path must be (K >= 2, 1, 3), got (4, 3)"),            # 2-D on a batched scene
    (False, 4, 2, "path", 0, "K", (5, 4, 2), "path must be (K >= 2, 4, 3), got (5, 4, 2)"),      # wrong n
    (False, 4, 2, "path", 0, "K", (4, 5, 3), "path must be (K >= 2, 4, 3), got (4, 5, 3)"),      # (R, K, n) where (K, R, n) is due
    (True, 1, 2, "path", 0, "K", (5, 2), "path must be (K >= 2, 1, 3), got (5, 1, 2)"),
    (False, 2, 3, "path", 0, "W", (2, 2, 3), "path must be (W >= 3, 2, 3), got (2, 2, 3)"),      # optimize_path: K = kmin - 1
    (True, 1, 3, "path", 0, "W", (2, 3), "path must be (W >= 3, 1, 3), got (2, 1, 3)"),
    (False, 2, 0, "poly", 1, "K", (4, 3), "poly must be (2, K, 3), got (4, 3)"),                 # blend_path: 2-D on a batched scene
    (False, 2, 0, "poly", 1, "K", (4, 2, 3), "poly must be (2, K, 3), got (4, 2, 3)"),           # (K, R, n) where (R, K, n) is due
    (True, 1, 0, "poly", 1, "K", (4, 2), "poly must be (1, K, 3), got (1, 4, 2)"),               # wrong n, the env axis left out
])
def test_path_rows_refuses(unbatched, R, kmin, name, axis, letter, shape, message):
    with pytest.raises(ValueError) as e:
        EntityView._path_rows(entity(unbatched), np.zeros(shape, np.float32), R, kmin, name, axis, letter)
    assert str(e.value) == message


# ---- EntityView._drop_env_axis(detail, axis1=("path",))
def test_drop_env_axis():
    K = 4
    detail = {"path": torch.arange(K * D, dtype=torch.float32).reshape(K, 1, D), "status": torch.tensor([7], dtype=torch.int32),
              "stats": torch.arange(4, dtype=torch.int32).reshape(1, 4), "samples": torch.arange(K * D, dtype=torch.float32).reshape(K, 1, D)}
    same = EntityView._drop_env_axis(entity(False), detail)
    assert same is detail                                   # a batched task: the dict as it is
    one = EntityView._drop_env_axis(entity(True), detail)
    assert list(one) == list(detail)
    assert tuple(one["path"].shape) == (K, D) and torch.equal(one["path"], detail["path"][:, 0])
    assert one["status"].shape == () and int(one["status"]) == 7 and one["status"].dtype == torch.int32
    assert tuple(one["stats"].shape) == (4,) and torch.equal(one["stats"], detail["stats"][0])
    assert tuple(one["samples"].shape) == (1, D)            # (not named: axis 0 goes)
    two = EntityView._drop_env_axis(entity(True), detail, ("path", "samples"))
    assert tuple(two["samples"].shape) == (K, D) and tuple(two["path"].shape) == (K, D)
    none = EntityView._drop_env_axis(entity(True), {"clearance": torch.tensor([0.5]), "seg_min": torch.zeros(1, 3)}, ())
    assert none["clearance"].shape == () and tuple(none["seg_min"].shape) == (3,)
