"""GPU (-m gpu): the act path of the GRU navigation policy (pnvo_policy_act -> gru_layer_kernel through the nn.Module mirror) against
the torch float64 model of tests/gru_reference.py, which tests/test_policy_gru_host.py pins to the reference policy itself.

Criterion: the project's (tests/test_gpu_policy.py): 2e-4 of each tensor's scale over features, every [B, hidden] block of the
[L, B, hidden] state, logits and value; the deterministic action equals the model's arg-max wherever the model's top two logits are
apart by the rule of tests/test_gpu_policy_regimes.py (more than 1e-3 of the largest logit magnitude).  The input seeds below were
chosen on the CPU, from the float64 model alone, so that at least three quarters of the rows of every case are clear; each test asserts
that share before it compares.

Shapes (frames 96 x 128 unless noted): the smallest at which each path of the kernel can go wrong —
  h128   hidden 128, 2 layers, B = 3, two consecutive steps: non-zero incoming state, masks that differ inside a step
  h264   hidden 264, 1 layer, B = 2: 66 float4 per row, a second, ragged pass of the lane loop
  b65    hidden 128, 3 layers, 3 actions, B = 65: a second 64-row chunk
  full   192 x 341, hidden 512, 2 layers, B = 9: the default sizes
The inputs make every environment distinct (its own frame, goal, incoming state in [-1, 1]); previous actions take every value with
mask 1 and with mask 0."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gru_reference as G
from pointnav_vo_amd import _lib, synth
from pointnav_vo_amd.policy import PointNavResNetPolicy, policy_state_dict_spec

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TOL = 2e-4
GOAL = "pointgoal_with_gps_compass"
# name -> (H, W, hidden, layers, actions, B, steps, input seed)
CASES = {"h128": (96, 128, 128, 2, 4, 3, 2, 101), "h264": (96, 128, 264, 1, 4, 2, 1, 102), "b65": (96, 128, 128, 3, 3, 65, 1, 103),
         "full": (192, 341, 512, 2, 4, 9, 1, 104)}


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class Act:
    def __init__(self, n):
        self.n = n


def make_policy(H, W, hidden, layers, n_actions, rnn_type="GRU", seed=5):
    space = Space({"depth": Box((H, W, 1)), "rgb": Box((H, W, 3)), GOAL: Box((2,))})
    pol = PointNavResNetPolicy(observation_space=space, action_space=Act(n_actions), hidden_size=hidden, rnn_type=rnn_type,
                               num_recurrent_layers=layers, backbone="resnet18", goal_sensor_uuid=GOAL,
                               normalize_visual_inputs=False, obs_transform=None, vis_types=["depth"])
    sd = synth.make_state_dict(policy_state_dict_spec(width=W, height=H, hidden=hidden, n_actions=n_actions, rnn_layers=layers,
                                                      rnn_type=rnn_type), seed=seed)
    assert list(pol.state_dict().keys()) == list(sd.keys())
    pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return pol.to(DEV).eval(), sd


def make_hidden(blocks, B, Hd, seed):
    return synth.uniform(seed, "h0", (blocks, B, Hd), -1.0, 1.0).astype(np.float32)


def make_step(H, W, B, n_actions, seed, t):
    """Step t: a distinct frame and goal per environment; mask 0 at b % 3 == 1 and b == 64 (step 0) or at b % 3 == 0 (later steps);
    previous actions run through every value among the masked and among the unmasked environments."""
    depth = synth.uniform(seed, f"depth{t}", (B, H, W, 1), 0.0, 1.0).astype(np.float32)
    goal = np.stack([synth.uniform(seed, f"rho{t}", (B,), 0.2, 6.0), synth.uniform(seed, f"phi{t}", (B,), -3.0, 3.0)],
                    axis=-1).astype(np.float32)
    b = np.arange(B)
    zero = (b % 3 == 1) | (b == 64) if t == 0 else (b % 3 == 0)
    prev = np.empty(B, np.int64)
    for sel in (zero, ~zero):
        idx = np.flatnonzero(sel)
        prev[idx] = (np.arange(len(idx)) + t) % n_actions
    return depth, goal, prev, np.where(zero, 0.0, 1.0).astype(np.float32)


def close(got, want, tol=TOL):
    scale = np.abs(want).max() + 1e-6
    return np.abs(got - want).max() / scale < tol


def clear_rows(logits):
    lg = np.asarray(logits, np.float64)
    top2 = np.sort(lg, axis=-1)[:, -2:]
    return (top2[:, 1] - top2[:, 0]) > 1e-3 * (np.abs(lg).max() + 1e-12)


@functools.lru_cache(maxsize=None)
def weights(name):
    H, W, Hd, L, A = CASES[name][:5]
    return synth.make_state_dict(G.spec(H=H, W=W, hidden=Hd, A=A, L=L), seed=5)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 model's steps of a case, each fed its own previous state: computed once, shared, read-only."""
    H, W, Hd, L, A, B, steps, seed = CASES[name]
    hid = make_hidden(L, B, Hd, seed).astype(np.float64)
    out = []
    for t in range(steps):
        o = G.policy_step(weights(name), *make_step(H, W, B, A, seed, t), hid)
        out.append(o)
        hid = o["hidden"]
    return out


def run_gpu(pol, inputs, hidden):
    depth, goal, prev, mask = inputs
    B = depth.shape[0]
    obs = {"depth": torch.from_numpy(depth).to(DEV), GOAL: torch.from_numpy(goal).to(DEV)}
    pa, mk = torch.from_numpy(prev).view(B, 1).to(DEV), torch.from_numpy(mask).view(B, 1).to(DEV)
    feats, hnew, logits, value = pol.features_and_logits(obs, hidden, pa, mk)
    v2, action, logp, h2 = pol.act(obs, hidden, pa, mk, deterministic=True)
    torch.cuda.synchronize()
    assert torch.equal(h2, hnew) and torch.equal(v2, value)
    assert tuple(action.shape) == (B, 1) and action.dtype == torch.int64 and tuple(logp.shape) == (B, 1)
    out = dict(features=feats.cpu().numpy(), hidden=hnew.cpu().numpy(), logits=logits.cpu().numpy(), value=value.cpu().numpy(),
               action=action.cpu().numpy()[:, 0], logp=logp.cpu().numpy()[:, 0])
    return out, hnew


def assert_matches(got, o, L, what):
    assert got["hidden"].shape == o["hidden"].shape and got["hidden"].shape[0] == L, (what, got["hidden"].shape)
    assert close(got["features"], o["features"]), (what, "features")
    for l in range(L):
        assert close(got["hidden"][l], o["hidden"][l]), (what, "h", l)
    assert close(got["logits"], o["logits"]), (what, "logits")
    assert close(got["value"], o["value"]), (what, "value")
    clear = clear_rows(o["logits"])
    assert clear.mean() >= 0.75, (what, "the seed leaves too few rows with a clear arg-max", clear.mean())
    np.testing.assert_array_equal(got["action"][clear], np.asarray(o["logits"]).argmax(-1)[clear], err_msg=str(what))
    lg = np.asarray(o["logits"], np.float64)
    m = lg.max(-1, keepdims=True)
    want_logp = (lg - m - np.log(np.exp(lg - m).sum(-1, keepdims=True)))[np.arange(lg.shape[0]), got["action"]]
    np.testing.assert_allclose(got["logp"], want_logp, rtol=0, atol=2e-4, err_msg=str(what))


def run_case(name, pol=None):
    H, W, Hd, L, A, B, steps, seed = CASES[name]
    if pol is None:
        pol, sd = make_policy(H, W, Hd, L, A)
        assert all(np.array_equal(sd[k], weights(name)[k]) for k in sd)
    assert pol.num_recurrent_layers == pol.net.num_recurrent_layers == L
    hidden = torch.from_numpy(make_hidden(L, B, Hd, seed)).to(DEV)
    first = None
    for t in range(steps):
        inputs = make_step(H, W, B, A, seed, t)
        hin = hidden
        got, hidden = run_gpu(pol, inputs, hin)
        assert_matches(got, reference(name)[t], L, (name, t))
        first = first or (inputs, hin, got)
    return pol, first


# ------------------------------------------------------------------------------------------------------------ the LSTM beside it
@functools.lru_cache(maxsize=None)
def lstm_inputs():
    H, W, Hd, L, A, B = 96, 128, 128, 2, 4, 3
    return make_step(H, W, B, A, 55, 1), np.concatenate([make_hidden(L, B, Hd, 55), 3.0 * make_hidden(L, B, Hd, 56)])


def run_lstm():
    pol, _ = make_policy(96, 128, 128, 2, 4, rnn_type="LSTM")
    inputs, hid = lstm_inputs()
    got, _ = run_gpu(pol, inputs, torch.from_numpy(hid).to(DEV))
    return pol, got


@pytest.fixture(scope="module", autouse=True)
def lstm_before():
    """An LSTM policy built and run before this module creates its first GRU handle (in the suite's default order no earlier module
    creates one either)."""
    return run_lstm()


# ---------------------------------------------------------------------------------------------------------------------- tests
def test_two_steps_with_state_and_mixed_masks_match_fp64():
    H, W, Hd, L, A, B, steps, seed = CASES["h128"]
    masks = [make_step(H, W, B, A, seed, t)[3] for t in range(steps)]
    assert all(0 < m.sum() < B for m in masks) and make_hidden(L, B, Hd, seed).all(axis=-1).all()
    pol, (inputs, hin, got) = run_case("h128")
    # an environment whose mask is 0 gets exactly what it gets from a zeroed incoming state
    mask = inputs[3]
    hz = hin * torch.from_numpy(mask).to(DEV)[None, :, None]
    assert not torch.equal(hz, hin)
    got_z, _ = run_gpu(pol, inputs, hz)
    for k in ("features", "hidden", "logits", "value", "action", "logp"):
        np.testing.assert_array_equal(got_z[k], got[k], err_msg=k)
    # and the state of an unmasked environment does matter
    got_0, _ = run_gpu(pol, inputs, torch.zeros_like(hin))
    keep = mask == 1
    assert not np.array_equal(got_0["hidden"][:, keep], got["hidden"][:, keep])
    np.testing.assert_array_equal(got_0["hidden"][:, ~keep], got["hidden"][:, ~keep])


def test_ragged_second_pass_of_the_lane_loop_matches_fp64():
    assert (CASES["h264"][2] // 4) == 66                     # 64 lanes + 2: the second pass is ragged
    run_case("h264")


def test_second_chunk_of_environments_matches_fp64_and_is_distinguishable():
    L = CASES["b65"][3]
    _, (inputs, _, got) = run_case("b65")
    assert inputs[3][64] == 0 and inputs[3][0] == 1
    want = reference("b65")[0]["hidden"]
    swapped = want.copy()
    swapped[:, [0, 64]] = want[:, [64, 0]]                    # environments b and b + 64 traded: the comparison must notice
    assert not all(close(got["hidden"][l], swapped[l]) for l in range(L))
    lg = reference("b65")[0]["logits"].copy()
    lg[[0, 64]] = lg[[64, 0]]
    assert not close(got["logits"], lg)


def test_default_sizes_match_fp64():
    run_case("full")


def _act_raw(pol, inputs, hin_ptr, hout_ptr, feats, logits, value):
    depth, goal, prev, mask = (torch.from_numpy(a).to(DEV) for a in inputs)
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(DEV):
        stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        rc = _lib.lib.pnvo_policy_act(pol._handle, p(depth), p(goal), p(prev), p(mask), C.c_void_p(hin_ptr), int(depth.shape[0]),
                                      C.c_void_p(hout_ptr), p(feats), p(logits), p(value), stream)
    torch.cuda.synchronize()
    return rc


def test_overlapping_state_buffers_are_refused_and_adjacent_ones_served():
    """hidden_out == hidden_in and hidden_out one [B, hidden] block behind hidden_in are refused with PNVO_ERR_ARG and nothing is
    written; disjoint buffers of L * B * hidden floats each (half the LSTM's) right behind one another are served."""
    H, W, Hd, L, A, B, _, seed = CASES["h128"]
    pol, _ = make_policy(H, W, Hd, L, A)
    pol._ensure(DEV)
    n = L * B * Hd
    hid = make_hidden(L, B, Hd, seed)
    inputs = make_step(H, W, B, A, seed, 0)
    for off in (0, B * Hd):
        buf = torch.zeros(2 * n + B * Hd, device=DEV)
        buf[:n] = torch.from_numpy(hid.reshape(-1)).to(DEV)
        feats, logits, value = (torch.full(s, 7.0, device=DEV) for s in ((B, Hd), (B, A), (B, 1)))
        before = buf.clone()
        torch.cuda.synchronize()
        rc = _act_raw(pol, inputs, buf.data_ptr(), buf.data_ptr() + 4 * off, feats, logits, value)
        assert rc == -1, (off, rc)                             # PNVO_ERR_ARG
        assert "overlap" in _lib.lib.pnvo_last_error(None).decode(), off
        assert torch.equal(buf, before) and (feats == 7).all() and (logits == 7).all() and (value == 7).all(), off
    o = reference("h128")[0]
    for first_in in (True, False):
        buf = torch.zeros(2 * n, device=DEV)
        hin, hout = (buf[:n], buf[n:]) if first_in else (buf[n:], buf[:n])
        hin.copy_(torch.from_numpy(hid.reshape(-1)))
        feats, logits, value = (torch.empty(s, device=DEV) for s in ((B, Hd), (B, A), (B, 1)))
        rc = _act_raw(pol, inputs, hin.data_ptr(), hout.data_ptr(), feats, logits, value)
        assert rc == 0, _lib.lib.pnvo_last_error(None).decode()
        assert torch.equal(hin.cpu(), torch.from_numpy(hid.reshape(-1)))
        got = hout.view(L, B, Hd).cpu().numpy()
        assert all(close(got[l], o["hidden"][l]) for l in range(L)), first_in
        assert close(feats.cpu().numpy(), o["features"]) and close(logits.cpu().numpy(), o["logits"])
        assert close(value.cpu().numpy(), o["value"])


def test_unknown_rnn_type_is_refused_by_the_library():
    class cfg(C.Structure):
        _fields_ = [(n, C.c_int32) for n in ("width", "height", "baseplanes", "hidden", "n_actions", "rnn_layers", "flat_size", "rnn_type")]
    h = C.c_void_p()
    rc = _lib.lib.pnvo_policy_create(C.byref(cfg(128, 96, 32, 128, 4, 2, 2048, 7)), 0, C.byref(h))
    assert rc == -1 and h.value is None
    assert "rnn_type 7" in _lib.lib.pnvo_last_error(None).decode()


def test_an_lstm_policy_beside_gru_policies_is_unaffected(lstm_before):
    """The two types share no state: an LSTM policy run before the first GRU handle of this module, the same policy run again after
    GRU policies have acted, and a second LSTM policy built after them give the same bits."""
    pol_a, before = lstm_before
    gru, _ = run_case("h128")                                  # a GRU handle exists and has acted (whatever ran before this test)
    inputs, hid = lstm_inputs()
    again, _ = run_gpu(pol_a, inputs, torch.from_numpy(hid).to(DEV))
    pol_b, after = run_lstm()
    assert gru._handle is not None and pol_a._handle.value != pol_b._handle.value
    assert before["hidden"].shape == (4, 3, 128) and np.isfinite(before["hidden"]).all()
    for k in before:
        np.testing.assert_array_equal(again[k], before[k], err_msg=k)
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
