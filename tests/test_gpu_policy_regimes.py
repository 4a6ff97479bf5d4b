"""GPU (-m gpu): the HIP navigation policy (pnvo_policy_act through the nn.Module mirror) against the fp64 policy oracle
outside the default nav-loop shape: batches that cross every kernel threshold of the encoder and the LSTM's 64-sample chunks,
a workspace reused across shrinking and growing batches, non-default hidden sizes / layer counts / action counts / base widths,
an odd frame height, and the C ABI's refusal of aliased hidden-state buffers.

Every step compares all four outputs (features, the [2L,B,Hd] hidden state block by block, logits, value) with the criterion of
tests/test_gpu_policy.py (2e-4 of the tensor's scale), the deterministic action with the oracle's arg-max wherever the oracle's top
two logits are apart, and the action's log-probability with the oracle's log_softmax.  The inputs make every environment distinct:
its own depth frame, goal and non-zero incoming state (h in [-1, 1], c in [-3, 3]), masks that differ inside one step and
previous actions that take every value with mask 1 and with mask 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import policy_oracle
from pointnav_vo_amd import _lib, synth
from pointnav_vo_amd.policy import PointNavResNetPolicy, policy_state_dict_spec

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TOL = 2e-4


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class Act:
    def __init__(self, n):
        self.n = n


def make_policy(H, W, hidden=512, layers=2, n_actions=4, baseplanes=32, seed=5):
    space = Space({"depth": Box((H, W, 1)), "rgb": Box((H, W, 3)), "pointgoal_with_gps_compass": Box((2,))})
    pol = PointNavResNetPolicy(observation_space=space, action_space=Act(n_actions), hidden_size=hidden, rnn_type="LSTM",
                               num_recurrent_layers=layers, resnet_baseplanes=baseplanes, backbone="resnet18",
                               goal_sensor_uuid="pointgoal_with_gps_compass", normalize_visual_inputs=False, obs_transform=None,
                               vis_types=["depth"])
    spec = policy_state_dict_spec(width=W, height=H, baseplanes=baseplanes, hidden=hidden, n_actions=n_actions, rnn_layers=layers)
    sd = synth.make_state_dict(spec, seed=seed)
    assert list(pol.state_dict().keys()) == list(sd.keys())
    pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return pol.to(DEV).eval(), sd


def make_hidden(L, B, Hd, seed):
    """A non-zero incoming state: h of every layer in [-1, 1], c in [-3, 3] (so that c_prev * mask matters)."""
    h = synth.uniform(seed, "h0", (L, B, Hd), -1.0, 1.0)
    c = synth.uniform(seed, "c0", (L, B, Hd), -3.0, 3.0)
    return np.concatenate([h, c]).astype(np.float32)


def make_step(H, W, B, n_actions, seed, t):
    """Inputs of step t: a distinct depth frame and goal per environment; masks 0 at b % 5 == 0 and at b = 64 (step 0) or at
    b % 7 == 3 (later steps); previous actions that run through every action value among the masked and the unmasked environments."""
    depth = synth.uniform(seed, f"depth{t}", (B, H, W, 1), 0.0, 1.0).astype(np.float32)
    goal = np.stack([synth.uniform(seed, f"rho{t}", (B,), 0.2, 6.0), synth.uniform(seed, f"phi{t}", (B,), -3.0, 3.0)],
                    axis=-1).astype(np.float32)
    b = np.arange(B)
    zero = (b % 5 == 0) | (b == 64) if t == 0 else (b % 7 == 3)
    mask = np.where(zero, 0.0, 1.0).astype(np.float32)
    prev = np.empty(B, np.int64)
    for sel in (zero, ~zero):
        idx = np.flatnonzero(sel)
        prev[idx] = (np.arange(len(idx)) + t) % n_actions
    return depth, goal, prev, mask


def close(got, want, tol=TOL):
    scale = np.abs(want).max() + 1e-6
    return np.abs(got - want).max() / scale < tol


def log_softmax(x):
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def run_gpu(pol, inputs, hidden):
    """features_and_logits and act(deterministic=True) on the same inputs -> numpy outputs (and the hidden state on the device)."""
    depth, goal, prev, mask = inputs
    B = depth.shape[0]
    obs = {"depth": torch.from_numpy(depth).to(DEV), "pointgoal_with_gps_compass": torch.from_numpy(goal).to(DEV)}
    pa, mk = torch.from_numpy(prev).view(B, 1).to(DEV), torch.from_numpy(mask).view(B, 1).to(DEV)
    feats, hnew, logits, value = pol.features_and_logits(obs, hidden, pa, mk)
    v2, action, logp, h2 = pol.act(obs, hidden, pa, mk, deterministic=True)
    torch.cuda.synchronize()
    assert torch.equal(h2, hnew) and torch.equal(v2, value)          # act() is deterministic given the inputs
    assert tuple(action.shape) == (B, 1) and action.dtype == torch.int64 and tuple(logp.shape) == (B, 1)
    out = dict(features=feats.cpu().numpy(), hidden=hnew.cpu().numpy(), logits=logits.cpu().numpy(), value=value.cpu().numpy(),
               action=action.cpu().numpy()[:, 0], logp=logp.cpu().numpy()[:, 0])
    return out, hnew


def assert_matches(got, o, L, what):
    """got: run_gpu's outputs; o: policy_oracle.policy_step's (fp64)."""
    assert close(got["features"], o["features"]), (what, "features")
    for l in range(L):
        assert close(got["hidden"][l], o["hidden"][l]), (what, "h", l)
        assert close(got["hidden"][L + l], o["hidden"][L + l]), (what, "c", l)
    assert close(got["logits"], o["logits"]), (what, "logits")
    assert close(got["value"], o["value"]), (what, "value")
    lg = np.asarray(o["logits"], np.float64)
    B, n = lg.shape
    if n > 1:
        top2 = np.sort(lg, axis=-1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) > 1e-3 * (np.abs(lg).max() + 1e-12)
        np.testing.assert_array_equal(got["action"][clear], lg.argmax(-1)[clear], err_msg=str(what))
    want_logp = log_softmax(lg)[np.arange(B), got["action"]]
    np.testing.assert_allclose(got["logp"], want_logp, rtol=0, atol=2e-4, err_msg=str(what))


def run_steps(pol, sd, H, W, B, L, Hd, n_actions, baseplanes, seed, steps=2):
    """`steps` consecutive steps: the GPU carries its own hidden output, the oracle its own."""
    hid_o = make_hidden(L, B, Hd, seed).astype(np.float64)
    hidden = torch.from_numpy(hid_o.astype(np.float32)).to(DEV)
    for t in range(steps):
        inputs = make_step(H, W, B, n_actions, seed, t)
        got, hidden = run_gpu(pol, inputs, hidden)
        o = policy_oracle.policy_step(sd, *inputs, hid_o, baseplanes=baseplanes)
        assert_matches(got, o, L, (B, t))
        hid_o = o["hidden"]
    return got, o


# ---------------------------------------------------------------------------------------------------------- (a) batch regimes
# 8 / 9: the persistent encoder kernel's limit; 16 / 17: the encoder handle's max_batch hint; 32: the benchmarked nav loop;
# 48 / 49: fc_rows; 64 / 65 / 130: the LSTM's 64-sample chunks (a second and a third chunk)
@pytest.mark.parametrize("B", [1, 7, 8, 9, 16, 17, 32, 48, 49, 64, 65, 130])
def test_policy_batch_regimes_match_the_oracle(B):
    H, W = 192, 341
    pol, sd = make_policy(H, W)
    run_steps(pol, sd, H, W, B, 2, 512, 4, 32, seed=100 + B)


# ------------------------------------------------------------------------------------------------------- (b) sensitivity guard
def test_chunks_are_distinguishable_and_masked_state_is_ignored():
    """At B = 130 the comparison would fail if environments b and b + 64 (one LSTM chunk apart) traded places, so a wrong chunk
    offset cannot pass; and an environment whose mask is 0 gets exactly what it gets from a zeroed incoming state."""
    H, W, B, L, Hd = 192, 341, 130, 2, 512
    pol, sd = make_policy(H, W)
    seed = 7
    hid = make_hidden(L, B, Hd, seed)
    inputs = make_step(H, W, B, 4, seed, 0)
    got, _ = run_gpu(pol, inputs, torch.from_numpy(hid).to(DEV))
    o = policy_oracle.policy_step(sd, *inputs, hid.astype(np.float64))
    assert_matches(got, o, L, "guard")
    want = o["hidden"]
    for b in range(64):
        swapped = want.copy()
        swapped[:, [b, b + 64]] = want[:, [b + 64, b]]
        assert not all(close(got["hidden"][k], swapped[k]) for k in range(2 * L)), b
    # the masked environments' incoming state zeroed: every output bit-identical
    mask = inputs[3]
    assert (mask == 0).sum() > 2 and mask[64] == 0
    hz = hid * mask[None, :, None]
    got_z, _ = run_gpu(pol, inputs, torch.from_numpy(hz).to(DEV))
    for k in ("features", "hidden", "logits", "value", "action", "logp"):
        np.testing.assert_array_equal(got_z[k], got[k], err_msg=k)


# -------------------------------------------------------------------------------------------------------- (c) workspace reuse
def test_workspace_reused_across_batches():
    """One policy object, batches 130, 5, 65, 1, 130: the workspace grows only at the first call; every call matches the oracle, and the
    two calls at 130 on identical inputs are bit-identical."""
    H, W, L, Hd = 192, 341, 2, 512
    pol, sd = make_policy(H, W)
    first = None
    for i, B in enumerate((130, 5, 65, 1, 130)):
        seed = 40 + (0 if B == 130 else i)
        hid = make_hidden(L, B, Hd, seed)
        inputs = make_step(H, W, B, 4, seed, 0)
        got, _ = run_gpu(pol, inputs, torch.from_numpy(hid).to(DEV))
        o = policy_oracle.policy_step(sd, *inputs, hid.astype(np.float64))
        assert_matches(got, o, L, (i, B))
        if B == 130:
            if first is None:
                first = got
            else:
                for k in got:
                    np.testing.assert_array_equal(got[k], first[k], err_msg=k)
    assert first is not None


# ------------------------------------------------------------------------------------------------------- (d) configurations
# (hidden_size, num_recurrent_layers, action_space.n, resnet_baseplanes)
CONFIGS = [
    (512, 1, 4, 32), (512, 3, 4, 32), (512, 4, 4, 32),
    (256, 2, 4, 32), (128, 2, 4, 32),          # Hd / 4 below the 64 lanes of a wave
    (512, 2, 3, 32),                           # n_actions + 1 = 4 head rows: exactly one heads workgroup
    (512, 2, 8, 32),                           # 9 head rows: three workgroups
    (516, 2, 4, 32),                           # hidden not a multiple of 32
    (512, 2, 4, 64),
]
DEFAULT = (512, 2, 4, 32)


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "h%d_l%d_a%d_bp%d" % c)
def test_policy_configurations_match_the_oracle_or_are_refused(cfg):
    """A configuration either matches the oracle or is refused (at construction or at the first act) with an error that names the
    unsupported value; it never returns numbers wrongly.  Every hidden size the visual encoder takes (multiples of 8: 128 and 256
    among them, the values the reference's config keys take in practice) must be served, with 1 to 4 layers, 3 or 8 actions and
    base width 64.  Today only hidden_size 516 is refused (pnvo_policy_create)."""
    Hd, L, n_actions, bp = cfg
    H, W = 192, 341
    odd = [v for v, d in zip(cfg, DEFAULT) if v != d]
    must_serve = Hd % 8 == 0
    try:
        pol, sd = make_policy(H, W, hidden=Hd, layers=L, n_actions=n_actions, baseplanes=bp)
        pol._ensure(DEV)                                   # pnvo_policy_create + load_weights: what the first act does
    except (_lib.PnvoError, NotImplementedError) as e:
        assert not must_serve, f"{cfg} must be served: {e}"
        assert any(str(v) in str(e) for v in odd), f"the refusal of {cfg} does not name the unsupported value: {e}"
        return
    for B in (5, 9, 65):
        run_steps(pol, sd, H, W, B, L, Hd, n_actions, bp, seed=200 + B)


# ------------------------------------------------------------------------------------------------------------ (e) odd height
@pytest.mark.parametrize("B", [3, 9])
def test_odd_frame_height_matches_the_oracle(B):
    """193 x 341: avg_pool2d(2) drops the last row, so the encoder sees the default's 96 x 170 map and only the pooling's frame
    stride differs from an even height."""
    H, W = 193, 341
    pol, sd = make_policy(H, W)
    run_steps(pol, sd, H, W, B, 2, 512, 4, 32, seed=300 + B)


# --------------------------------------------------------------------------------------------- (f) aliased hidden buffers
def _act_raw(pol, inputs, hin_ptr, hout_ptr, feats, logits, value):
    depth, goal, prev, mask = (torch.from_numpy(a).to(DEV) for a in inputs)
    B = depth.shape[0]
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(DEV):
        stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        rc = _lib.lib.pnvo_policy_act(pol._handle, p(depth), p(goal), p(prev), p(mask), C.c_void_p(hin_ptr), int(B),
                                      C.c_void_p(hout_ptr), p(feats), p(logits), p(value), stream)
    torch.cuda.synchronize()
    return rc


def test_aliased_hidden_buffers_are_refused():
    """pnvo_policy_act refuses hidden_out == hidden_in and a partial overlap (the LSTM writes a layer's state while other workgroups
    still read it) with PNVO_ERR_ARG and launches nothing; adjacent, disjoint buffers are served and match the oracle."""
    H, W, B, L, Hd = 96, 128, 9, 2, 512
    pol, sd = make_policy(H, W)
    pol._ensure(DEV)
    n = 2 * L * B * Hd
    hid = make_hidden(L, B, Hd, 11)
    inputs = make_step(H, W, B, 4, 11, 0)
    ERR_ARG = -1
    for off in (0, B * Hd):                                   # hidden_out == hidden_in; hidden_out = hidden_in + B*Hd floats
        buf = torch.zeros(2 * n + B * Hd, device=DEV)
        buf[:n] = torch.from_numpy(hid.reshape(-1)).to(DEV)
        feats = torch.full((B, Hd), 7.0, device=DEV)
        logits = torch.full((B, 4), 7.0, device=DEV)
        value = torch.full((B, 1), 7.0, device=DEV)
        before = buf.clone()
        torch.cuda.synchronize()
        rc = _act_raw(pol, inputs, buf.data_ptr(), buf.data_ptr() + 4 * off, feats, logits, value)
        assert rc == ERR_ARG, (off, rc)
        assert "overlap" in _lib.lib.pnvo_last_error(None).decode(), off
        assert torch.equal(buf, before) and (feats == 7).all() and (logits == 7).all() and (value == 7).all(), off
    o = policy_oracle.policy_step(sd, *inputs, hid.astype(np.float64))
    for first_in in (True, False):                            # hidden_out right behind hidden_in, and right in front of it
        buf = torch.zeros(2 * n, device=DEV)
        hin, hout = (buf[:n], buf[n:]) if first_in else (buf[n:], buf[:n])
        hin.copy_(torch.from_numpy(hid.reshape(-1)))
        feats, logits, value = (torch.empty(s, device=DEV) for s in ((B, Hd), (B, 4), (B, 1)))
        rc = _act_raw(pol, inputs, hin.data_ptr(), hout.data_ptr(), feats, logits, value)
        assert rc == 0, _lib.lib.pnvo_last_error(None).decode()
        assert torch.equal(hin.cpu(), torch.from_numpy(hid.reshape(-1)))
        got = hout.view(2 * L, B, Hd).cpu().numpy()
        for k in range(2 * L):
            assert close(got[k], o["hidden"][k]), (first_in, k)
        assert close(feats.cpu().numpy(), o["features"]) and close(logits.cpu().numpy(), o["logits"])
        assert close(value.cpu().numpy(), o["value"])
