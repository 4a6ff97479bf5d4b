"""GPU (-m gpu): the HIP baseline navigation policy (pnvo_baseline_* through the nn.Module mirror) against the outputs recorded from the
imported reference PointNavBaselinePolicy (tests/golden/baseline_policy_*.npz) and against the float64 restatement of
tests/baseline_policy_reference.py.  Tolerance: 2e-4 of each tensor's scale (tests/test_gpu_policy.py's `close`), per output per step.
Frame sizes: no pixel count is a multiple of 16 and the stride remainders are non-zero (85x53 -> maps 12x20, 5x9, 3x7, F = 672)."""
import ctypes as C

import numpy as np
import pytest
import torch

import baseline_policy_reference as R
from conftest import load_golden
from pointnav_vo_amd import PointNavBaselinePolicy, _lib, baseline_policy
from test_baseline_policy_host import Act, space

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def make_policy(c, sd):
    pol = PointNavBaselinePolicy(space(c["H"], c["W"], c["vis"]), Act(R.N_ACTIONS), R.GOAL, c["hidden"])
    assert list(pol.state_dict().keys()) == list(sd.keys())
    pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return pol.to(DEV).eval()


def observations(rgb, depth, goal, rgb_float=False):
    obs = {R.GOAL: torch.from_numpy(np.ascontiguousarray(goal)).to(DEV)}
    if rgb is not None:
        t = torch.from_numpy(np.ascontiguousarray(rgb))
        obs["rgb"] = (t.float() if rgb_float else t).to(DEV)
    if depth is not None:
        obs["depth"] = torch.from_numpy(np.ascontiguousarray(depth)).to(DEV)
    return obs


def step(pol, obs, hidden, mask):
    """(features, hidden, logits, value) as float64 ndarrays plus the device state."""
    B = hidden.shape[1]
    pa, mk = torch.zeros(B, 1, dtype=torch.int64, device=DEV), torch.from_numpy(np.ascontiguousarray(mask)).view(B, 1).to(DEV)
    feats, hnew, logits, value = pol.features_and_logits(obs, hidden, pa, mk)
    torch.cuda.synchronize()
    out = dict(features=feats, hidden=hnew, logits=logits, value=value)
    return {k: v.cpu().numpy() for k, v in out.items()}, hnew, (pa, mk)


def check(got, want, what):
    err = R.rel_err(got, want)
    print(f"{what}: {err:.2e} of scale")
    assert np.isfinite(got).all() and got.shape == want.shape and err < R.TOL, (what, err)


def run_case(case, rgb_float=False):
    """The case's steps against its fixture; -> the outputs of every step (for bit comparisons)."""
    rec, c = load_golden(f"baseline_policy_{case}.npz"), R.CASES[case]
    pol = make_policy(c, R.state_dict(case))
    assert pol.net.is_blind == (not c["vis"]) and pol.net.num_recurrent_layers == 1 and pol.net.output_size == c["hidden"]
    hidden = torch.zeros(1, c["B"], c["hidden"], device=DEV)
    outs = []
    for t, (rgb, depth, goal, mask) in enumerate(R.inputs(case)):
        obs = observations(rgb, depth, goal, rgb_float)
        o, hnew, (pa, mk) = step(pol, obs, hidden, mask)
        for k in ("features", "hidden", "logits", "value"):
            check(o[k], rec[f"{'logits_raw' if k == 'logits' else k}64/{t}"], f"{case} step {t} {k}")
        if c["vis"]:
            o["embed"] = pol.net.visual_encoder(obs).cpu().numpy()
            check(o["embed"], rec[f"embed64/{t}"], f"{case} step {t} embed")
        value, action, logp, h2 = pol.act(obs, hidden, pa, mk, deterministic=True)
        assert torch.equal(h2, hnew) and np.array_equal(value.cpu().numpy(), o["value"])
        assert torch.equal(pol.get_value(obs, hidden, pa, mk), value)               # bit for bit
        feats, h3 = pol.net(obs, hidden, pa, mk)
        assert torch.equal(h3, hnew) and np.array_equal(feats.cpu().numpy(), o["features"])
        np.testing.assert_array_equal(action.cpu().numpy(), rec[f"action64/{t}"])
        assert tuple(value.shape) == (c["B"], 1) and tuple(action.shape) == (c["B"], 1) and action.dtype == torch.int64
        assert tuple(h2.shape) == (1, c["B"], c["hidden"]) and tuple(logp.shape) == (c["B"], 1)
        outs.append(o)
        hidden = hnew
    return outs


def test_rgbd_steps_match_the_reference():
    """Four consecutive steps of two environments, environment 1 reset at step 2."""
    assert R.CASES["rgbd_85x53"]["steps"] == 4
    run_case("rgbd_85x53")


def test_depth_only_matches_the_reference():
    run_case("depth_64x64")


def test_rgb_only_matches_the_reference_and_uint8_equals_float32():
    a, b = run_case("rgb_85x53"), run_case("rgb_85x53", rgb_float=True)
    for t, (oa, ob) in enumerate(zip(a, b)):
        for k in oa:
            assert np.array_equal(oa[k], ob[k]), (t, k)


def test_rgbd_uint8_equals_float32():
    c = R.CASES["rgbd_85x53"]
    pol = make_policy(c, R.state_dict("rgbd_85x53"))
    rgb, depth, goal, mask = R.inputs("rgbd_85x53")[1]
    hidden = torch.full((1, c["B"], c["hidden"]), 0.25, device=DEV)
    a = step(pol, observations(rgb, depth, goal), hidden, mask)[0]
    b = step(pol, observations(rgb, depth, goal, rgb_float=True), hidden, mask)[0]
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_full_size_frames_match_the_reference():
    """341 x 192 rgb-d, B = 3, hidden 512: the split-K Linear at F = 24 960."""
    run_case("rgbd_341x192")


@pytest.mark.parametrize("H,W,vis,hidden,B", [(36, 36, ("depth",), 24, 3), (37, 39, ("rgb", "depth"), 40, 1)])
def test_smallest_frames_and_hidden_sizes_off_the_linear_tile(H, W, vis, hidden, B):
    """36 x 36 leaves conv3 ONE output pixel (F = 32: two 16-float steps for the Linear's four waves, fewer pixels than a conv tile);
    hidden sizes that are multiples of 8 but not of the Linear's 16-unit block.  Two steps against the float64 restatement."""
    c = dict(H=H, W=W, vis=vis, B=B, steps=2, hidden=hidden, wseed=51, iseed=52)
    sd = R.state_dict(c)
    pol = make_policy(c, sd)
    hidden_t, hidden_np = torch.zeros(1, B, hidden, device=DEV), np.zeros((1, B, hidden))
    for t, (rgb, depth, goal, mask) in enumerate(R.inputs(c)):
        obs = observations(rgb, depth, goal)
        o, hidden_t, _ = step(pol, obs, hidden_t, mask)
        o["embed"] = pol.net.visual_encoder(obs).cpu().numpy()
        want = R.policy_step(sd, rgb, depth, goal, mask, hidden_np)
        for k in R.OUTPUTS:
            assert np.abs(want[k]).max() >= 1e-2, (t, k)
            check(o[k], want[k], f"{W}x{H} hidden {hidden} step {t} {k}")
        hidden_np = want["hidden"]


def pool_batch(p, idx):
    obs = observations(p["rgb"][idx], p["depth"][idx], p["goal"][idx])
    return obs, torch.from_numpy(np.ascontiguousarray(p["hidden"][:, idx])).to(DEV), p["mask"][idx]


def test_batch_independence_and_determinism():
    """Batches of 1, 5, 67 and 130 drawn from a pool of 31 samples (the GRU kernel's 64-row chunk, the Linear's 32-row workgroup and 16-row
    tile, the convs' 64-pixel tiles crossing sample boundaries): every position within tolerance of the float64 restatement of its own
    sample, two runs bit-identical, and a sample's bits the same at every position of every batch."""
    p = R.pool()
    pol = make_policy(R.POOL, p["sd"])
    bits = {}
    for B in (1, 5, 67, 130):
        idx = R.positions(B)
        obs, hidden, mask = pool_batch(p, idx)
        o1 = step(pol, obs, hidden, mask)[0]
        o1["embed"] = pol.net.visual_encoder(obs).cpu().numpy()
        o2 = step(pol, obs, hidden, mask)[0]
        o2["embed"] = pol.net.visual_encoder(obs).cpu().numpy()
        for k in R.OUTPUTS:
            assert np.array_equal(o1[k], o2[k]), (B, k)
            got = o1[k][0] if k == "hidden" else o1[k]
            want = p["want"][k][0] if k == "hidden" else p["want"][k]
            check(got, want[idx], f"B={B} {k}")
            for pos, i in enumerate(idx):
                row = got[pos].tobytes()
                assert bits.setdefault((k, int(i)), row) == row, (B, k, pos, int(i))


def test_blind_policy():
    import gc
    c = R.CASES["blind"]
    outs = run_case("blind")
    assert all("embed" not in o for o in outs)
    gc.collect()
    before = _lib.lib.pnvo_device_bytes_live()
    pol = make_policy(c, R.state_dict("blind"))
    assert pol.net.is_blind and pol.net.visual_encoder.is_blind
    _, _, goal, mask = R.inputs("blind")[0]
    step(pol, observations(None, None, goal), torch.zeros(1, c["B"], c["hidden"], device=DEV), mask)
    # no encoder: its weights and workspace do not exist (the handle holds the GRU with its padded input weight, the heads and one
    # four-float input row per environment; a buffer is never smaller than 16 bytes)
    n = sum(int(np.prod(s)) for _, s in R.spec("blind")) + 3 * c["hidden"] * 2 + c["B"] * 4
    assert 0 < _lib.lib.pnvo_device_bytes_live() - before <= 4 * n + 16 * 16
    with pytest.raises(RuntimeError, match="blind"):
        pol.net.visual_encoder({})


def test_sampling():
    c = R.CASES["rgbd_85x53"]
    pol = make_policy(c, R.state_dict("rgbd_85x53"))
    rgb, depth, goal, mask = R.inputs("rgbd_85x53")[1]
    obs = observations(rgb, depth, goal)
    hidden = torch.zeros(1, c["B"], c["hidden"], device=DEV)
    o, _, (pa, mk) = step(pol, obs, hidden, mask)
    torch.manual_seed(3)
    for _ in range(4):
        value, action, logp, hnew = pol.act(obs, hidden, pa, mk, deterministic=False)
        assert action.dtype == torch.int64 and action.min() >= 0 and action.max() < R.N_ACTIONS
        want = torch.log_softmax(torch.from_numpy(o["logits"]).to(DEV), dim=-1).gather(-1, action)
        assert (logp - want).abs().max() <= 1e-6 and np.array_equal(value.cpu().numpy(), o["value"])
    with pytest.raises(NotImplementedError, match="PPO update"):
        pol.evaluate_actions(obs, hidden, pa, mk, action)


def raw_handle(cfg, sd=None, drop=()):
    cc = baseline_policy.pnvo_baseline_config(**cfg)
    h = C.c_void_p()
    rc = _lib.lib.pnvo_baseline_create(C.byref(cc), 0, C.byref(h))
    if rc != 0 or sd is None:
        return rc, h
    tensors = [(k, torch.from_numpy(np.array(v))) for k, v in sd.items() if k not in drop]
    blob, toc = _lib.pack_tensors(tensors)
    return _lib.lib.pnvo_baseline_load_weights(h, blob.ctypes.data_as(C.c_void_p), blob.size, toc, len(tensors)), h


def test_refusals_by_error_code_with_nothing_launched():
    c = R.CASES["depth_64x64"]
    cfg = dict(width=c["W"], height=c["H"], rgb_channels=0, depth_channels=1, hidden=c["hidden"], n_actions=R.N_ACTIONS, goal_dim=2)
    rc, _ = raw_handle(dict(cfg, height=35))
    assert rc == -1 and b">= 36" in _lib.lib.pnvo_last_error(None)                  # PNVO_ERR_ARG
    sd = R.state_dict("depth_64x64")
    rc, h = raw_handle(cfg, sd, drop=(R.CNN + "6.weight",))
    assert rc == -4 and b"cnn.6.weight" in _lib.lib.pnvo_last_error(None)           # PNVO_ERR_WEIGHTS
    B, Hd = c["B"], c["hidden"]
    _, depth, goal, mask = R.inputs("depth_64x64")[0]
    d, g, m = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (depth, goal, mask))
    state = torch.full((2, B, Hd), 7.0, device=DEV)
    out = torch.full((B, Hd + R.N_ACTIONS + 1), 7.0, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    act = lambda depth_p, hin, hout: _lib.lib.pnvo_baseline_act(h, None, 0, depth_p, p(g), p(m), hin, B, hout, p(out), None, None, None)
    assert act(p(d), p(state[0]), p(state[1])) == -3                                # PNVO_ERR_STATE: the weights were refused
    assert _lib.lib.pnvo_baseline_destroy(h) == 0
    rc, h = raw_handle(cfg, sd)
    assert rc == 0
    assert act(p(d), p(state[0]), p(state[0])) == -1 and b"overlap" in _lib.lib.pnvo_last_error(None)
    assert act(p(d), p(state[0]), C.c_void_p(state[0].data_ptr() + 4 * (B * Hd - 4))) == -1      # the last 16 bytes shared
    assert act(None, p(state[0]), p(state[1])) == -1 and b"visual types" in _lib.lib.pnvo_last_error(None)
    assert _lib.lib.pnvo_baseline_act(h, p(d), 0, p(d), p(g), p(m), p(state[0]), B, p(state[1]), None, None, None, None) == -1   # rgb on a depth handle
    assert _lib.lib.pnvo_baseline_encode(h, None, 0, None, B, p(out), None) == -1
    torch.cuda.synchronize()
    assert bool((state == 7.0).all()) and bool((out == 7.0).all())                  # nothing ran
    assert act(p(d), p(state[0]), p(state[1])) == 0                                 # and the handle still serves a good call
    torch.cuda.synchronize()
    assert bool((state[0] == 7.0).all()) and bool(torch.isfinite(state[1]).all()) and not bool((state[1] == 7.0).any())
    assert _lib.lib.pnvo_baseline_destroy(h) == 0


def test_weight_reload_follows_the_new_parameters():
    c = R.CASES["rgbd_85x53"]
    pol = make_policy(c, R.state_dict("rgbd_85x53"))
    rgb, depth, goal, mask = R.inputs("rgbd_85x53")[1]
    obs = observations(rgb, depth, goal)
    hidden_np = R.rollout("rgbd_85x53")[0]["hidden"]
    hidden = torch.from_numpy(hidden_np).float().to(DEV)
    first = step(pol, obs, hidden, mask)[0]
    sd2 = R.state_dict("rgbd_85x53", seed=77)
    pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd2.items()})
    second = step(pol, obs, hidden, mask)[0]
    want = R.policy_step(sd2, rgb, depth, goal, mask, hidden_np.astype(np.float32))
    for k in ("features", "hidden", "logits", "value"):
        check(second[k], want[k], f"reloaded {k}")
        assert not R.close(first[k], want[k]), k                                    # the first weights give something else
    check(pol.net.visual_encoder(obs).cpu().numpy(), want["embed"], "reloaded embed")
