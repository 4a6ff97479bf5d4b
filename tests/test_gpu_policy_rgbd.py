"""GPU (-m gpu): the act path of the navigation policy with rgb / rgb-d input and RunningMeanAndVar (pnvo_policy_act_rgbd,
pnvo_policy_encode_rgbd: policy_input_kernel + the float32 stem with its whitening pair written on the device) against the reference
policy's recorded float64 outputs (tests/golden/policy_rgbd_128x96_h128_b2.npz) and, where no fixture exists, against the float64
model of tests/rgbd_policy_reference.py, which tests/test_policy_rgbd_host.py pins to those recordings.

Criterion: the project's (tests/test_gpu_policy.py): 2e-4 of each tensor's scale over features, every [B, hidden] block of the
state, logits and value; the deterministic action equals the model's arg-max wherever its top two logits are apart by the rule of
tests/test_gpu_policy_regimes.py (more than 1e-3 of the largest logit magnitude).

Statistics.  _count is exact.  _mean and _var: oracle.torch_train_ref.running_stats_update run in float32 on the CPU, on the frames
and starting buffers of the fixture's training-mode steps (cases b, c, d), deviates from the recorded float64 statistics by at most
1.403e-07 (_mean, case d) and 7.640e-08 (_var, case b step 1) of the tensor's largest magnitude; STAT_TOL = 10 x that, the rule that
gave GRAD_TOL of tests/test_gpu_ppo.py: what a float32 framework itself loses.  On the 192 x 341 frames of the odd-width case the same
measurement gives 5.2e-08 / 2.5e-08, below those figures: the same STAT_TOL is applied there.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import rgbd_policy_reference as Q
from conftest import load_golden
from pointnav_vo_amd import _lib, synth
from pointnav_vo_amd.obs_transforms import ResizeCenterCropper
from pointnav_vo_amd.policy import RMV_PREFIX, PointNavResNetPolicy

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TOL = 2e-4
STAT_TOL = {"_mean": 1.403e-6, "_var": 7.64e-7}
GOAL = Q.GOAL
H, W, HIDDEN, LAYERS, N_ACT, B = 96, 128, 128, 2, 4, 2
# case -> (vis_types, rnn_type, zero-initialised statistics, training flag of each step): tests/golden/gen_golden_policy_rgbd.py
CASES = {"a": (["rgb", "depth"], "LSTM", False, [False] * 4), "b": (["rgb", "depth"], "GRU", True, [True] * 3),
         "c": (["rgb"], "LSTM", False, [False, True]), "d": (["depth"], "LSTM", True, [True])}


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class Act:
    def __init__(self, n):
        self.n = n


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("policy_rgbd_128x96_h128_b2.npz")


def make_policy(vis, rnn, sd=None, seed=5, zero_stats=False, h=H, w=W, normalize=True, obs_transform=None, frame=None):
    fh, fw = frame or (h, w)
    space = Space({"depth": Box((fh, fw, 1)), "rgb": Box((fh, fw, 3)), GOAL: Box((2,))})
    pol = PointNavResNetPolicy(observation_space=space, action_space=Act(N_ACT), hidden_size=HIDDEN, rnn_type=rnn,
                               num_recurrent_layers=LAYERS, backbone="resnet18", goal_sensor_uuid=GOAL,
                               normalize_visual_inputs=normalize, obs_transform=obs_transform, vis_types=vis)
    if sd is None:
        sd = synth.make_state_dict(Q.spec(H=h, W=w, hidden=HIDDEN, A=N_ACT, L=LAYERS, rnn=rnn, vis=vis, normalize=normalize), seed=seed)
    if zero_stats:
        sd = {k: (np.zeros_like(v) if k.startswith(RMV_PREFIX) else v) for k, v in sd.items()}
    assert list(pol.state_dict().keys()) == list(sd.keys())
    pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return pol.to(DEV), sd


def buffers(pol):
    rmv = pol.net.visual_encoder.running_mean_and_var
    return {"_mean": rmv._mean, "_var": rmv._var, "_count": rmv._count}


def stats_numpy(pol):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy().copy() for k, v in buffers(pol).items()}


def set_stats(pol, stats):
    for k, v in buffers(pol).items():
        v.copy_(torch.as_tensor(np.asarray(stats[k], np.float32)).reshape(v.shape))


def to_obs(vis, rgb, depth, goal, rgb_float=False):
    obs = {GOAL: torch.from_numpy(goal).to(DEV)}
    if "rgb" in vis:
        t = torch.from_numpy(rgb)
        obs["rgb"] = (t.float() if rgb_float else t).to(DEV)
    if "depth" in vis:
        obs["depth"] = torch.from_numpy(depth).to(DEV)
    return obs


def run_step(pol, vis, step, hidden, rgb_float=False):
    """ONE forward (in training mode every forward updates the statistics) -> numpy outputs, the new state on the device."""
    rgb, depth, goal, prev, mask = step
    n = len(goal)
    pa, mk = torch.from_numpy(prev).view(n, 1).to(DEV), torch.from_numpy(mask).view(n, 1).to(DEV)
    feats, hnew, logits, value = pol.features_and_logits(to_obs(vis, rgb, depth, goal, rgb_float), hidden, pa, mk)
    torch.cuda.synchronize()
    return dict(features=feats.cpu().numpy(), hidden=hnew.cpu().numpy(), logits=logits.cpu().numpy(), value=value.cpu().numpy()), hnew


def rel(got, want):
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64).reshape(want.shape) - want).max() / (np.abs(want).max() + 1e-6)


def assert_outputs(got, want, what):
    for k in ("features", "logits", "value"):
        e = rel(got[k], want[k])
        print(f"{what} {k}: {e:.2e} of scale")
        assert e < TOL, (what, k, e)
    assert got["hidden"].shape == np.shape(want["hidden"])
    for l in range(got["hidden"].shape[0]):
        e = rel(got["hidden"][l], want["hidden"][l])
        assert e < TOL, (what, "hidden", l, e)


def assert_stats(got, want, what):
    assert float(got["_count"]) == float(want["_count"]), (what, got["_count"], want["_count"])
    for k, tol in STAT_TOL.items():
        w = np.asarray(want[k], np.float64)
        e = np.abs(got[k].astype(np.float64).reshape(w.shape) - w).max() / np.abs(w).max()
        print(f"{what} {k}: {e:.2e} of the largest magnitude (STAT_TOL {tol:.2e})")
        assert e <= tol, (what, k, e)


def clear_rows(logits):
    lg = np.asarray(logits, np.float64)
    top2 = np.sort(lg, axis=-1)[:, -2:]
    return (top2[:, 1] - top2[:, 0]) > 1e-3 * (np.abs(lg).max() + 1e-12)


def states(rnn):
    return LAYERS * (2 if rnn == "LSTM" else 1)


# ------------------------------------------------------------------------------------------------ 1. the reference's recordings
@pytest.mark.parametrize("case", list(CASES))
def test_case_matches_the_reference_policy(case):
    vis, rnn, zero, training = CASES[case]
    g = golden()
    pol, _ = make_policy(vis, rnn, seed=int(g[f"{case}/weight_seed"]), zero_stats=zero)
    ptrs = [b.data_ptr() for b in buffers(pol).values()]
    hidden = torch.zeros(states(rnn), B, HIDDEN, device=DEV)
    steps = synth.make_policy_rgbd_inputs(H, W, B, len(training), int(g[f"{case}/input_seed"]), N_ACT)
    n_clear = 0
    for t, step in enumerate(steps):
        pol.train(training[t])
        before = stats_numpy(pol)
        hin = hidden
        got, hidden = run_step(pol, vis, step, hin)
        want = {k: g[f"{case}/{gk}/{t}"] for k, gk in (("features", "features64"), ("hidden", "hidden64"), ("logits", "logits_raw64"),
                                                       ("value", "value64"))}
        assert_outputs(got, want, (case, t))
        after = stats_numpy(pol)
        if training[t]:
            assert_stats(after, {k: g[f"{case}/{gk}/{t}"] for k, gk in (("_mean", "mean64"), ("_var", "var64"), ("_count", "count64"))}, (case, t))
        else:                                              # .eval(): read, never written
            assert all(np.array_equal(after[k], before[k]) for k in before), (case, t)
            rgb, depth, goal, prev, mask = step
            _, action, logp, h2 = pol.act(to_obs(vis, rgb, depth, goal), hin, torch.from_numpy(prev).view(B, 1).to(DEV),
                                          torch.from_numpy(mask).view(B, 1).to(DEV), deterministic=True)
            assert torch.equal(h2, hidden)
            clear = clear_rows(want["logits"])
            n_clear += int(clear.sum())
            np.testing.assert_array_equal(action.cpu().numpy()[:, 0][clear], np.asarray(want["logits"]).argmax(-1)[clear])
    assert [b.data_ptr() for b in buffers(pol).values()] == ptrs                 # updated in place
    assert case != "a" or n_clear >= 6, n_clear                                  # (most of case a's 8 rows have a clear arg-max)


# ------------------------------------------------------------------------------------------------ 2. bits
def test_uint8_and_float32_rgb_and_repeated_calls_give_equal_bits():
    """Training mode from the same starting buffers: uint8 rgb, the same call again, and float32 rgb holding the same values give
    the same outputs and the same statistics, bit for bit (every reduction has a fixed order; uint8 converts exactly)."""
    vis, rnn = ["rgb", "depth"], "GRU"
    pol, sd = make_policy(vis, rnn, seed=12)
    pol.train()
    step = synth.make_policy_rgbd_inputs(H, W, 3, 1, 77, N_ACT)[0]
    hidden = torch.from_numpy(synth.uniform(77, "h0", (states(rnn), 3, HIDDEN), -1.0, 1.0).astype(np.float32)).to(DEV)
    start = {k: np.asarray(sd[RMV_PREFIX + k]) for k in Q.STATS}
    start["_count"] = np.float32(3.0)                      # a light history: the batch moves the statistics visibly
    runs = []
    for rgb_float in (False, False, True):
        set_stats(pol, start)
        got, _ = run_step(pol, vis, step, hidden, rgb_float)
        runs.append((got, stats_numpy(pol)))
    assert not np.array_equal(runs[0][1]["_mean"], start["_mean"]) and float(runs[0][1]["_count"]) == 6.0
    for got, st in runs[1:]:
        for k in got:
            np.testing.assert_array_equal(got[k], runs[0][0][k], err_msg=k)
        for k in st:
            np.testing.assert_array_equal(st[k], runs[0][1][k], err_msg=k)


def test_eval_leaves_the_buffers_unchanged_and_training_then_eval_uses_the_updated_statistics():
    vis, rnn = ["rgb", "depth"], "LSTM"
    pol, sd = make_policy(vis, rnn, seed=11)
    sd = dict(sd)
    sd[RMV_PREFIX + "_count"] = np.array(2.0, np.float32)  # a light history: one batch moves the statistics a long way
    set_stats(pol, {k: sd[RMV_PREFIX + k] for k in Q.STATS})
    steps = synth.make_policy_rgbd_inputs(H, W, B, 2, 78, N_ACT)
    hid0 = np.zeros((states(rnn), B, HIDDEN), np.float32)
    hidden = torch.from_numpy(hid0).to(DEV)
    # .eval(): act, get_value, the encoder on its own, several times — the three buffers keep their bits
    pol.eval()
    before = stats_numpy(pol)
    rgb, depth, goal, prev, mask = steps[0]
    obs, pa, mk = to_obs(vis, rgb, depth, goal), torch.from_numpy(prev).view(B, 1).to(DEV), torch.from_numpy(mask).view(B, 1).to(DEV)
    for _ in range(2):
        pol.act(obs, hidden, pa, mk)
        pol.get_value(obs, hidden, pa, mk)
        pol.net.visual_encoder(obs)
    after = stats_numpy(pol)
    assert all(np.array_equal(after[k], before[k]) for k in before)
    # one act in training mode (what PPOTrainer's collection does), then .eval(): the next act whitens with the updated statistics
    pol.train()
    pol.act(obs, hidden, pa, mk)
    pol.eval()
    updated = stats_numpy(pol)
    ref_train = Q.policy_step(sd, {"rgb": rgb, "depth": depth}, goal, prev, mask, hid0, rnn, True)
    assert_stats(updated, ref_train["stats"], "after the training-mode act")
    assert np.abs(updated["_mean"] - before["_mean"]).max() > 0.05
    got, _ = run_step(pol, vis, steps[1], hidden)
    assert all(np.array_equal(stats_numpy(pol)[k], updated[k]) for k in updated)
    rgb1, depth1, goal1, prev1, mask1 = steps[1]
    want_new = Q.policy_step(Q.with_stats(sd, ref_train["stats"]), {"rgb": rgb1, "depth": depth1}, goal1, prev1, mask1, hid0, rnn, False)
    want_old = Q.policy_step(sd, {"rgb": rgb1, "depth": depth1}, goal1, prev1, mask1, hid0, rnn, False)
    assert_outputs(got, want_new, "eval after training")
    assert rel(got["features"], want_old["features"]) > 10 * TOL          # stale statistics in the handle would show


def test_encoder_output_fed_back_as_visual_features_reproduces_act():
    vis, rnn = ["rgb"], "GRU"
    pol, _ = make_policy(vis, rnn, seed=13)
    rgb, depth, goal, prev, mask = synth.make_policy_rgbd_inputs(H, W, B, 1, 79, N_ACT)[0]
    hidden = torch.from_numpy(synth.uniform(79, "h0", (states(rnn), B, HIDDEN), -1.0, 1.0).astype(np.float32)).to(DEV)
    obs, pa, mk = to_obs(vis, rgb, depth, goal), torch.from_numpy(prev).view(B, 1).to(DEV), torch.from_numpy(mask).view(B, 1).to(DEV)
    pol.eval()
    direct = pol.features_and_logits(obs, hidden, pa, mk)
    feats = pol.net.visual_encoder(obs)
    assert tuple(feats.shape) == (B,) + tuple(pol.net.visual_encoder.output_shape) and float(feats.min()) >= 0.0
    fed = pol.features_and_logits({"visual_features": feats, GOAL: obs[GOAL]}, hidden, pa, mk)
    torch.cuda.synchronize()
    for a, b, k in zip(fed, direct, ("features", "hidden", "logits", "value")):
        assert rel(a.cpu().numpy(), b.cpu().numpy()) < TOL, k
    # training mode: the encoder call merges its batch once; the call that takes the features never touches the statistics
    pol.train()
    c0 = float(stats_numpy(pol)["_count"])
    feats = pol.net.visual_encoder(obs)
    st = stats_numpy(pol)
    assert float(st["_count"]) == c0 + B
    fed = pol.features_and_logits({"visual_features": feats, GOAL: obs[GOAL]}, hidden, pa, mk)
    assert all(np.array_equal(stats_numpy(pol)[k], st[k]) for k in st)
    pol.eval()
    direct = pol.features_and_logits(obs, hidden, pa, mk)
    torch.cuda.synchronize()
    for a, b, k in zip(fed, direct, ("features", "hidden", "logits", "value")):
        assert rel(a.cpu().numpy(), b.cpu().numpy()) < TOL, k


# ------------------------------------------------------------------------------------------------ 3. other frame sizes
def test_default_frame_with_an_odd_width_matches_fp64():
    """192 x 341: the pool drops the last column, a row of uint8 rgb starts at any byte and a row of float32 frames at any float."""
    h, w, vis, rnn = 192, 341, ["rgb", "depth"], "LSTM"
    pol, sd = make_policy(vis, rnn, seed=14, h=h, w=w)
    sd = dict(sd)
    sd[RMV_PREFIX + "_count"] = np.array(4.0, np.float32)
    set_stats(pol, {k: sd[RMV_PREFIX + k] for k in Q.STATS})
    step = synth.make_policy_rgbd_inputs(h, w, B, 1, 80, N_ACT)[0]
    rgb, depth, goal, prev, mask = step
    hid0 = synth.uniform(80, "h0", (states(rnn), B, HIDDEN), -1.0, 1.0).astype(np.float32)
    want = Q.policy_step(sd, {"rgb": rgb, "depth": depth}, goal, prev, mask, hid0, rnn, True)
    pol.train()
    outs = []
    for rgb_float in (False, True):
        set_stats(pol, {k: sd[RMV_PREFIX + k] for k in Q.STATS})
        got, _ = run_step(pol, vis, step, torch.from_numpy(hid0).to(DEV), rgb_float)
        assert_outputs(got, want, ("341x192", "float32 rgb" if rgb_float else "uint8 rgb"))
        st = stats_numpy(pol)
        assert_stats(st, want["stats"], "341x192")
        outs.append((got, st))
    for k in outs[0][0]:
        np.testing.assert_array_equal(outs[0][0][k], outs[1][0][k], err_msg=k)
    for k in outs[0][1]:
        np.testing.assert_array_equal(outs[0][1][k], outs[1][1][k], err_msg=k)


def test_resize_crop_from_a_larger_rgbd_frame_matches_fp64():
    """RL.OBS_TRANSFORM = resize_crop per sensor in front of the concatenation (resnet_policy.py:164-167): 150 x 210 -> 96 x 128."""
    hs, ws, vis, rnn = 150, 210, ["rgb", "depth"], "GRU"
    pol, sd = make_policy(vis, rnn, seed=15, obs_transform=ResizeCenterCropper((W, H)), frame=(hs, ws))
    step = synth.make_policy_rgbd_inputs(hs, ws, B, 1, 81, N_ACT)[0]
    rgb, depth, goal, prev, mask = step
    hid0 = synth.uniform(81, "h0", (states(rnn), B, HIDDEN), -1.0, 1.0).astype(np.float32)
    want = Q.policy_step(sd, {"rgb": rgb, "depth": depth}, goal, prev, mask, hid0, rnn, False, transform=("resize_crop", (W, H)))
    pol.eval()
    got, _ = run_step(pol, vis, step, torch.from_numpy(hid0).to(DEV))
    assert_outputs(got, want, "resize_crop")
    got_f, _ = run_step(pol, vis, step, torch.from_numpy(hid0).to(DEV), rgb_float=True)
    for k in got:
        np.testing.assert_array_equal(got[k], got_f[k], err_msg=k)


# ------------------------------------------------------------------------------------------------ 4. the input stage on its own
@pytest.mark.parametrize("vis", [["rgb", "depth"], ["rgb"], ["depth"]])
def test_input_stage_pools_pads_and_sums(vis):
    """policy_input_kernel on a 65 x 70 frame (an odd height, 35 pooled columns: a ragged last group of three; several workgroups) against
    torch on the CPU: the pooled tensor with its zero channels, and the fused moments against the two-launch form and float64."""
    h, w, n = 65, 70, 3
    pol, _ = make_policy(vis, "LSTM", seed=16, h=h, w=w)
    pol._ensure(DEV)
    step = synth.make_policy_rgbd_inputs(h, w, n, 1, 82, N_ACT)[0]
    rgb, depth = step[0], step[1]
    Cn = (3 if "rgb" in vis else 0) + (1 if "depth" in vis else 0)
    x64 = Q.pooled_input({k: v for k, v in (("rgb", rgb), ("depth", depth)) if k in vis}, torch.float64)
    x32 = Q.pooled_input({k: v for k, v in (("rgb", rgb), ("depth", depth)) if k in vis}, torch.float32).permute(0, 2, 3, 1).numpy()
    center = np.linspace(0.1, 0.4, Cn).astype(np.float32)
    d = x64.permute(0, 2, 3, 1).reshape(-1, Cn) - torch.from_numpy(center).double()
    want_m12 = torch.cat([d.mean(0), (d * d).mean(0)]).numpy()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    ctr = torch.from_numpy(center).to(DEV)
    dep = torch.from_numpy(depth).to(DEV) if "depth" in vis else None
    results = []
    for rgb_float in (False, True):
        img = None
        if "rgb" in vis:
            img = torch.from_numpy(rgb).to(DEV)
            img = img.float() if rgb_float else img
        for mode in (0, 1, 2):
            pooled = torch.full((n, h // 2, w // 2, 2 * Cn), 7.0, device=DEV)
            m12 = torch.zeros(2 * Cn, device=DEV, dtype=torch.float64)
            with torch.cuda.device(DEV):
                _lib.check(_lib.lib.pnvo_policy_input_stage(pol._handle, p(img), int(not rgb_float), p(dep), p(ctr), mode, n, p(pooled), p(m12),
                                                            C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
            torch.cuda.synchronize()
            results.append((pooled.cpu().numpy(), m12.cpu().numpy(), mode))
    base = results[0][0]
    assert not base[..., Cn:].any()                                             # the zero channels
    np.testing.assert_allclose(base[..., :Cn], x32, rtol=0, atol=2e-7)          # (torch's own float32 pool: the same operations)
    for pooled, m12, mode in results:
        np.testing.assert_array_equal(pooled, base)                             # every mode, uint8 and float32 rgb: the same bits
        if mode:
            np.testing.assert_allclose(m12, want_m12, rtol=2e-6, atol=1e-9)     # float32 pooled values, float64 sums
    fused = [m for _, m, mode in results if mode == 1]
    np.testing.assert_array_equal(fused[0], fused[1])
    np.testing.assert_allclose(fused[0], [m for _, m, mode in results if mode == 2][0], rtol=1e-12, atol=1e-15)


def test_depth_only_entry_points_refuse_an_rgbd_handle():
    pol, _ = make_policy(["rgb", "depth"], "LSTM", seed=17)
    pol._ensure(DEV)
    depth = torch.zeros(B, H, W, 1, device=DEV)
    out = torch.zeros((B,) + tuple(pol.net.visual_encoder.output_shape), device=DEV)
    rc = _lib.lib.pnvo_policy_encode(pol._handle, C.c_void_p(depth.data_ptr()), B, C.c_void_p(out.data_ptr()), None)
    assert rc == -3 and "pnvo_policy_encode_rgbd" in _lib.lib.pnvo_last_error(None).decode()      # PNVO_ERR_STATE
    rc = _lib.lib.pnvo_policy_encode_rgbd(pol._handle, None, 0, C.c_void_p(depth.data_ptr()), None, None, None, 0, B,
                                          C.c_void_p(out.data_ptr()), None)
    assert rc == -1 and "rgb missing" in _lib.lib.pnvo_last_error(None).decode()                  # PNVO_ERR_ARG, nothing launched
    torch.cuda.synchronize()
    assert not out.any()
