"""CPU: the baseline navigation policy's module (names, shapes, order, initialisation, refusals) and the float64 restatement the GPU
tests compare with (tests/baseline_policy_reference.py) against the outputs recorded from the imported reference
(tests/golden/baseline_policy_*.npz, written by tests/golden/gen_golden_baseline_policy.py)."""
import numpy as np
import pytest
import torch

import baseline_policy_reference as R
from conftest import load_golden
from pointnav_vo_amd import PointNavBaselinePolicy, baseline_policy


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class Act:
    def __init__(self, n=4):
        self.n = n


def space(H, W, vis):
    d = {R.GOAL: Box((2,))}
    if "rgb" in vis:
        d["rgb"] = Box((H, W, 3))
    if "depth" in vis:
        d["depth"] = Box((H, W, 1))
    return Space(d)


def build(case):
    c = R.CASES[case]
    return PointNavBaselinePolicy(space(c["H"], c["W"], c["vis"]), Act(R.N_ACTIONS), R.GOAL, c["hidden"])


def recorded_spec(rec):
    return [(str(n), tuple(int(d) for d in str(s).split(","))) for n, s in zip(rec["sd_names"], rec["sd_shapes"])]


@pytest.mark.parametrize("case", list(R.CASES))
def test_state_dict_has_the_reference_names_shapes_and_order(case):
    rec = load_golden(f"baseline_policy_{case}.npz")
    want = recorded_spec(rec)
    assert [(n, tuple(s)) for n, s in R.spec(case)] == want
    pol = build(case)
    assert [(k, tuple(v.shape)) for k, v in pol.state_dict().items()] == want
    blind = not R.CASES[case]["vis"]
    assert pol.net.is_blind == blind and pol.net.visual_encoder.is_blind == blind
    assert any(n.startswith(R.CNN) for n, _ in want) != blind
    assert pol.net.output_size == R.CASES[case]["hidden"] and pol.net.num_recurrent_layers == 1
    assert int(rec["weight_seed"]) == R.CASES[case]["wseed"] and int(rec["input_seed"]) == R.CASES[case]["iseed"]


def test_initialisation_follows_layer_init():
    torch.manual_seed(0)
    sd = build("rgbd_85x53").state_dict()
    for k, v in sd.items():
        if "bias" in k:
            assert not v.any(), k                                                   # every bias starts at zero
    w = sd[R.CNN + "6.weight"]                                                       # kaiming-normal: std^2 = 2 / ((1 + a^2) fan_in), a = sqrt(2)
    assert abs(float(w.std()) / np.sqrt(2.0 / (3.0 * w.shape[1])) - 1.0) < 0.05
    for k, gain in ((R.RNN + "weight_hh_l0", 1.0), ("action_distribution.linear.weight", 0.01), ("critic.fc.weight", 1.0)):
        m = sd[k].double()
        g = m @ m.T if m.shape[0] <= m.shape[1] else m.T @ m                        # orthogonal rows (or columns), scaled by the gain
        torch.testing.assert_close(g, gain * gain * torch.eye(g.shape[0], dtype=torch.float64), atol=1e-5, rtol=0)


@pytest.mark.parametrize("case", list(R.CASES))
def test_float64_restatement_reproduces_the_reference(case):
    rec = load_golden(f"baseline_policy_{case}.npz")
    steps = R.rollout(case)
    assert len(steps) == int(rec["steps"]) == R.CASES[case]["steps"]
    for t, o in enumerate(steps):
        for k in R.OUTPUTS:
            key = f"{'logits_raw' if k == 'logits' else k}64/{t}"
            if k == "embed" and not R.CASES[case]["vis"]:
                assert key not in rec and k not in o
                continue
            assert o[k].shape == rec[key].shape, (case, t, k)
            assert R.rel_err(o[k], rec[key]) < 1e-9, (case, t, k, R.rel_err(o[k], rec[key]))
        np.testing.assert_array_equal(o["logits"].argmax(-1)[:, None], rec[f"action64/{t}"])


def test_float32_restatement_stays_under_a_quarter_of_the_tolerance():
    """The seeds' condition: a float32 framework on the same weights and inputs is within TOL / 4 of the float64 outputs on every compared
    tensor, and no compared tensor's scale is below 1e-2 (a seed that fails is replaced, the tolerance is not widened)."""
    for (case, k), (err, scale) in R.float32_error_table().items():
        assert err < R.TOL / 4, (case, k, err)
        assert scale >= 1e-2, (case, k, scale)
    p = R.pool()
    for k in R.OUTPUTS:
        assert np.abs(p["want"][k]).max() >= 1e-2, k


def test_pool_positions_cover_distinct_samples():
    for B in (1, 5, 67, 130):
        pos = R.positions(B)
        assert pos.min() >= 0 and pos.max() < R.POOL["P"]
        assert len(set(pos[:R.POOL["P"]].tolist())) == min(B, R.POOL["P"])
    assert len({int(R.positions(B)[0]) for B in (1, 5, 67, 130)}) == 4


def test_cpu_policy_refuses():
    c = R.CASES["rgbd_85x53"]
    pol = build("rgbd_85x53")
    rgb, depth, goal, mask = R.inputs("rgbd_85x53")[0]
    obs = {"rgb": torch.from_numpy(rgb), "depth": torch.from_numpy(depth), R.GOAL: torch.from_numpy(goal)}
    hidden = torch.zeros(1, c["B"], c["hidden"])
    pa, mk = torch.zeros(c["B"], 1, dtype=torch.int64), torch.from_numpy(mask).view(-1, 1)
    for call in (lambda: pol.act(obs, hidden, pa, mk), lambda: pol.get_value(obs, hidden, pa, mk), lambda: pol.net(obs, hidden, pa, mk),
                 lambda: pol.net.visual_encoder(obs)):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call()
    with pytest.raises(NotImplementedError, match="PPO update"):
        pol.evaluate_actions(obs, hidden, pa, mk, pa)
    with pytest.raises(NotImplementedError):
        pol.forward(obs)
    with pytest.raises(ValueError, match=">= 36"):
        PointNavBaselinePolicy(space(35, 85, ("rgb", "depth")), Act(), R.GOAL, 128)
    with pytest.raises(ValueError, match=">= 36"):
        PointNavBaselinePolicy(space(53, 35, ("depth",)), Act(), R.GOAL, 128)
    PointNavBaselinePolicy(space(36, 36, ("depth",)), Act(), R.GOAL, 128)           # the smallest frame is accepted
    with pytest.raises(ValueError, match="multiples of 8"):
        PointNavBaselinePolicy(space(53, 85, ("depth",)), Act(), R.GOAL, hidden_size=516)


def test_conv_map_sizes_follow_floor():
    assert baseline_policy.simple_cnn_dims(53, 85) == [(12, 20), (5, 9), (3, 7)]
    assert baseline_policy.simple_cnn_dims(64, 64) == [(15, 15), (6, 6), (4, 4)]
    assert baseline_policy.simple_cnn_dims(192, 341) == [(47, 84), (22, 41), (20, 39)]
    assert baseline_policy.simple_cnn_dims(36, 36) == [(8, 8), (3, 3), (1, 1)]
    assert baseline_policy.simple_cnn_dims(256, 256)[-1] == (28, 28)


def test_library_refuses_bad_configurations_without_a_gpu():
    """pnvo_baseline_create checks its configuration before it touches the device."""
    import ctypes as C

    from pointnav_vo_amd import _lib
    ok = dict(width=85, height=53, rgb_channels=3, depth_channels=1, hidden=128, n_actions=4, goal_dim=2)
    for bad in (dict(height=35), dict(width=35), dict(hidden=516), dict(hidden=0), dict(n_actions=0), dict(n_actions=33), dict(goal_dim=0),
                dict(goal_dim=9), dict(rgb_channels=1), dict(depth_channels=2)):
        cc = baseline_policy.pnvo_baseline_config(**dict(ok, **bad))
        h = C.c_void_p()
        assert _lib.lib.pnvo_baseline_create(C.byref(cc), 0, C.byref(h)) == -1, bad
        assert b"baseline" in _lib.lib.pnvo_last_error(None)
    assert _lib.lib.pnvo_baseline_destroy(None) == 0
    assert _lib.lib.pnvo_baseline_act(None, None, 0, None, None, None, None, 1, None, None, None, None, None) == -1
