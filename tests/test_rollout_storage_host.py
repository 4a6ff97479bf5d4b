"""CPU: the surface of pointnav_vo_amd.rollout_storage.RolloutStorage that needs no GPU — the reference's attributes (names, shapes,
dtypes), the `sensors=` extension, the refusals (Box action space, CPU-resident storage) and the argument checks of the five
pnvo_rollout_* entry points."""
import ctypes as C

import pytest
import torch

from pointnav_vo_amd import _lib
from pointnav_vo_amd.rollout_storage import RolloutStorage

GOAL = "pointgoal_with_gps_compass"


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class ActionSpace:                                       # the reference tests action_space.__class__.__name__ == "ActionSpace"
    def __init__(self, n):
        self.n = n


SPACE = Space({"rgb": Box((6, 9, 3)), "depth": Box((6, 9, 1)), GOAL: Box((2,))})
T, N, L, H = 5, 3, 4, 8


def make(**kw):
    return RolloutStorage(T, N, SPACE, ActionSpace(4), H, L, **kw)


def test_constructor_attributes_are_the_references():
    r = make()
    want = {
        "recurrent_hidden_states": ((T + 1, L, N, H), torch.float32),
        "rewards": ((T, N, 1), torch.float32),
        "action_log_probs": ((T, N, 1), torch.float32),
        "value_preds": ((T + 1, N, 1), torch.float32),
        "returns": ((T + 1, N, 1), torch.float32),
        "masks": ((T + 1, N, 1), torch.float32),
        "actions": ((T, N, 1), torch.int64),
        "prev_actions": ((T + 1, N, 1), torch.int64),
    }
    for name, (shape, dtype) in want.items():
        t = getattr(r, name)
        assert type(t) is torch.Tensor and tuple(t.shape) == shape and t.dtype == dtype, (name, t.shape, t.dtype)
        assert t.device.type == "cpu" and not t.any()
    assert list(r.observations) == ["rgb", "depth", GOAL]
    for s, box in SPACE.spaces.items():
        t = r.observations[s]
        assert tuple(t.shape) == (T + 1, N) + box.shape and t.dtype == torch.float32 and not t.any()
    assert r.num_steps == T and r.step == 0
    # the positional signature of the reference, num_recurrent_layers defaulting to 1
    assert tuple(RolloutStorage(T, N, SPACE, ActionSpace(4), H).recurrent_hidden_states.shape) == (T + 1, 1, N, H)
    assert r.to("cpu") is None                           # as the reference's .to


def test_sensors_restricts_the_stored_dict():
    r = make(sensors=["depth", GOAL])
    assert list(r.observations) == ["depth", GOAL]
    assert tuple(r.observations["depth"].shape) == (T + 1, N, 6, 9, 1)
    with pytest.raises(TypeError):
        RolloutStorage(T, N, SPACE, ActionSpace(4), H, L, ["depth"])      # keyword-only
    with pytest.raises(KeyError):
        make(sensors=["semantic"])


def test_box_action_space_is_refused():
    with pytest.raises(NotImplementedError):
        RolloutStorage(T, N, SPACE, Box((2,)), H, L)


def test_cpu_resident_storage_refuses_the_four_methods():
    r = make()
    obs = {s: torch.zeros(N, *b.shape) for s, b in SPACE.spaces.items()}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.insert(obs, torch.zeros(L, N, H), torch.zeros(N, 1, dtype=torch.int64), torch.zeros(N, 1), torch.zeros(N, 1),
                 torch.zeros(N, 1), torch.ones(N, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.after_update()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.compute_returns(torch.zeros(N, 1), True, 0.99, 0.95)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.recurrent_generator(torch.zeros(T, N, 1), 1)
    assert r.step == 0


def test_entry_points_return_err_arg_on_null_and_non_positive_arguments():
    lib = _lib.lib
    assert lib.pnvo_rollout_insert(*[None] * 7, T, N, L * N * H, 0, *[None] * 7) == -1
    assert b"pnvo_rollout_insert" in lib.pnvo_last_error(None)
    assert lib.pnvo_rollout_after_update(None, None, None, T, N, L * N * H, 1, None) == -1
    assert lib.pnvo_rollout_compute_returns(*[None] * 5, T, N, T, 1, 0.99, 0.94, None) == -1
    assert b"pnvo_rollout_compute_returns" in lib.pnvo_last_error(None)
    assert lib.pnvo_rollout_gather(*[None] * 9, N, L, H, T, 0, N, *[None] * 9) == -1
    assert lib.pnvo_rollout_gather_frames(None, None, N, 54, T, 0, N, None, None) == -1
    # non-null (host) pointers, bad sizes: refused before anything is launched
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.pnvo_rollout_insert(*[p] * 7, T, 0, L * N * H, 0, *[p] * 6, None) == -1
    assert lib.pnvo_rollout_insert(*[p] * 7, T, N, L * N * H, T, *[p] * 6, None) == -1          # a full storage
    assert b"full" in lib.pnvo_last_error(None)
    assert lib.pnvo_rollout_after_update(p, p, p, T, N, 0, 1, None) == -1
    assert lib.pnvo_rollout_after_update(p, p, p, T, N, L * N * H, T + 1, None) == -1
    assert lib.pnvo_rollout_compute_returns(*[p] * 5, 0, N, 0, 1, 0.99, 0.94, None) == -1
    assert lib.pnvo_rollout_compute_returns(*[p] * 5, T, N, T + 1, 1, 0.99, 0.94, None) == -1
    assert lib.pnvo_rollout_gather(*[p] * 9, N, L, H, 0, 0, N, *[p] * 8, None) == -1
    assert lib.pnvo_rollout_gather(*[p] * 9, N, L, H, T, 1, N, *[p] * 8, None) == -1            # start + n_mb > N
    assert lib.pnvo_rollout_gather_frames(p, p, N, 0, T, 0, N, p, None) == -1
    assert lib.pnvo_rollout_gather_frames(p, p, N, 54, T, -1, N, p, None) == -1
