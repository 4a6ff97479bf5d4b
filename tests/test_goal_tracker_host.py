"""CPU: what geometry.GoalTracker and the pnvo_nav_* entry points refuse before anything reaches a device.  A tracker on a CPU device
can be built and checks its arguments like one on the GPU; its launches have no CPU path."""
import ctypes as C

import numpy as np
import pytest
import torch

from pointnav_vo_amd import _lib
from pointnav_vo_amd.geometry import GoalTracker


def tracker(E=4, **kw):
    return GoalTracker(E, "cpu", **kw)


def test_state_tensors_have_the_documented_shapes_and_types():
    t = tracker(5)
    assert (t.goal.shape, t.goal.dtype) == ((5, 3), torch.float64)
    assert (t.rot.shape, t.rot.dtype) == ((5, 4), torch.float64)
    assert (t.pos.shape, t.pos.dtype) == ((5, 3), torch.float64)
    assert (t.polar.shape, t.polar.dtype) == ((5, 2), torch.float32)
    assert torch.equal(t.rot, torch.tensor([[0.0, 0.0, 0.0, 1.0]] * 5, dtype=torch.float64))      # the identity rotation
    g = tracker(5, track_pose=False)
    assert g.rot is None and g.pos is None and g.goal.shape == (5, 3)
    with pytest.raises(RuntimeError):
        g.global_state()
    for bad in (0, -2, 2.5):
        with pytest.raises(ValueError):
            GoalTracker(bad, "cpu")


@pytest.mark.parametrize("idx, what", [([0, 1, 1], "distinct"), ([0, 1, 4], "outside"), ([-1, 1, 2], "outside"),
                                       ([0, 1], "indices for 3 rows"), ([0, 1.0, 2], "not an integer"), (7, "sequence")])
def test_update_refuses_bad_indices(idx, what):
    t = tracker()
    with pytest.raises(ValueError, match=what):
        t.update(torch.zeros(3, 3), idx)


def test_update_refuses_bad_deltas():
    t = tracker()
    for bad in (torch.zeros(4, 2), torch.zeros(4, 3, 1), torch.zeros(12), torch.zeros(4, 3, dtype=torch.float64), np.zeros((4, 3), np.float32)):
        with pytest.raises(ValueError):
            t.update(bad)
    with pytest.raises(ValueError, match="pass env_indices"):
        t.update(torch.zeros(3, 3))                                   # three rows for four environments and no indices
    with pytest.raises(ValueError, match="CUDA"):
        t.update(torch.zeros(4, 3))                                   # right shape and type, but on the host
    with pytest.raises(ValueError, match="CUDA"):
        t.update(torch.zeros(2, 3), [3, 0])


def test_reset_refuses_bad_arguments():
    t = tracker()
    goals, pos, rot = np.zeros((2, 3)), np.zeros((2, 3)), np.tile([0.0, 0.0, 0.0, 1.0], (2, 1))
    with pytest.raises(ValueError, match="distinct"):
        t.reset([1, 1], goals, pos, rot)
    with pytest.raises(ValueError, match="outside"):
        t.reset([1, 4], goals, pos, rot)
    with pytest.raises(ValueError, match="goal_positions"):
        t.reset([1, 2], np.zeros((3, 3)), pos, rot)
    with pytest.raises(ValueError, match="start_positions"):
        t.reset([1, 2], goals, np.zeros((2, 2)), rot)
    with pytest.raises(ValueError, match="start_rotations"):
        t.reset([1, 2], goals, pos, np.zeros((2, 3)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # well-formed: refused because nothing runs on a CPU
        t.reset([1, 2], goals, pos, rot)
    assert not t.goal.any() and not t.polar.any()                     # and nothing was written


def test_nav_entry_points_return_error_codes_for_bad_arguments():
    lib = _lib.lib
    # stand-ins for device pointers: every refusal below happens before a launch, nothing is dereferenced
    buf = np.zeros(64, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.pnvo_nav_update(None, 3, None, 1, p, p, p, p, None) == -1
    assert b"pnvo_nav_update" in lib.pnvo_last_error(None)
    assert lib.pnvo_nav_update(p, 3, None, 1, None, p, p, p, None) == -1
    assert lib.pnvo_nav_update(p, 3, None, 1, p, p, p, None, None) == -1
    assert lib.pnvo_nav_update(p, 3, None, 1, p, None, p, p, None) == -1          # rot without pos
    assert lib.pnvo_nav_update(p, 3, None, 1, p, p, None, p, None) == -1          # pos without rot
    assert lib.pnvo_nav_update(p, 3, None, -1, p, p, p, p, None) == -1
    assert lib.pnvo_nav_update(p, 3, None, 0, p, p, p, p, None) == 0              # nothing to do: no launch
    assert lib.pnvo_nav_update(p, 3, None, 0, p, None, None, p, None) == 0        # goal only
    assert lib.pnvo_nav_reset(None, p, p, p, None, 1, p, p, p, p, None) == -1
    assert b"pnvo_nav_reset" in lib.pnvo_last_error(None)
    assert lib.pnvo_nav_reset(p, None, p, p, None, 1, p, p, p, p, None) == -1
    assert lib.pnvo_nav_reset(p, p, p, p, None, 1, None, p, p, p, None) == -1
    assert lib.pnvo_nav_reset(p, p, p, p, None, 1, p, p, p, None, None) == -1
    assert lib.pnvo_nav_reset(p, p, p, p, None, 1, p, None, p, p, None) == -1     # rot without pos
    assert lib.pnvo_nav_reset(p, p, None, p, None, 1, p, p, p, p, None) == -1     # a tracked pose without a start rotation
    assert lib.pnvo_nav_reset(p, p, p, p, None, -3, p, p, p, p, None) == -1
    assert lib.pnvo_nav_reset(p, p, p, p, None, 0, p, p, p, p, None) == 0
    assert lib.pnvo_nav_reset(p, p, None, None, None, 0, p, None, None, p, None) == 0
