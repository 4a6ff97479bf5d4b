"""GPU (-m gpu): frozen-encoder training of the HIP navigation policy (RL.DDPPO.train_encoder False: ddppo_trainer.py:158-161,257-271).

`policy.net.visual_encoder(observations)` (pnvo_policy_encode) against the fp64 oracle's compression tap; `act`, `features_and_logits`
and `evaluate_actions` fed with observations["visual_features"] and no "depth" (pnvo_policy_act_features /
pnvo_policy_evaluate_features) against the recorded fp64 values of the two policy fixtures, oracle.policy_oracle.policy_step,
tests/ppo_reference.py and tests/gru_reference.py; the PPO step against ppo_reference.clip_and_adam with the encoder frozen; and one
PPO.update from a RolloutStorage that holds features only beside a twin updated from frames with a frozen encoder.

Tolerances are the project's own: activations 2e-5 of max|ref|, forward tensors 2e-4 of scale
(tests/test_gpu_policy.py::close), losses 1e-4 * max(1, |x|), gradients 1e-4 relative L2 per tensor (GRAD_TOL of tests/test_gpu_ppo.py),
parameters after a step atol 2e-6.

Shapes: 128x96 frames give output_shape (512, 2, 2), F = 2048; 341x192 gives (114, 3, 6), F = 2052 (odd width through the pool, C not a
multiple of 32: the channel padding is dropped on the way out); 300x192 gives (137, 3, 5), F = 2055 (odd: visual_fc's weight rows are
not 16-byte aligned).  visual_fc runs on its row kernel up to 48 rows and on the matrix-core GEMM above."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gru_reference as G
import ppo_reference as R
from conftest import load_golden
from oracle import oracle, policy_oracle
from pointnav_vo_amd import _lib, synth
from pointnav_vo_amd.obs_transforms import ResizeCenterCropper, transformed_size
from pointnav_vo_amd.policy import PointNavResNetPolicy, policy_state_dict_spec
from pointnav_vo_amd.ppo import PPO, PolicyTrainStep
from pointnav_vo_amd.rollout_storage import RolloutStorage

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GOAL, FEAT, ENC = R.GOAL, "visual_features", R.ENC
ACT_TOL, TOL, GRAD_TOL = 2e-5, 2e-4, 1.0e-4
LR, EPS, MAX_GRAD_NORM = 2.5e-4, 1e-5, 0.2               # configs/rl/ddppo_pointnav.yaml

# one more case for the reference functions of tests/ppo_reference.py: 300x192 frames (F = 2055), one layer, T = 2, N = 2, a non-zero
# state carried into environment 1 at step 0
R.CASES.setdefault("S", dict(H=192, W=300, hidden=128, L=1, A=4, T=2, N=2, masks={0: [0, 1]}, wseed=14, iseed=35))
R.LOSS_SEED.setdefault("S", 3)
G.LOSS_SEED.setdefault("S", 3)


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class Act:
    def __init__(self, n):
        self.n = n


class ActionSpace(Act):
    pass


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_policy(H, W, sd, *, hidden, layers, n_actions=4, rnn_type="LSTM", obs_transform=None, frame=None):
    fh, fw = frame or (H, W)
    space = Space({"depth": Box((fh, fw, 1)), "rgb": Box((fh, fw, 3)), GOAL: Box((2,))})
    pol = PointNavResNetPolicy(observation_space=space, action_space=Act(n_actions), hidden_size=hidden, rnn_type=rnn_type,
                               num_recurrent_layers=layers, backbone="resnet18", goal_sensor_uuid=GOAL,
                               normalize_visual_inputs=False, obs_transform=obs_transform, vis_types=["depth"])
    assert list(pol.state_dict().keys()) == list(sd.keys())
    pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return pol.to(DEV).eval()


def weights(H, W, hidden, layers, n_actions=4, rnn_type="LSTM", seed=5):
    return synth.make_state_dict(policy_state_dict_spec(width=W, height=H, hidden=hidden, n_actions=n_actions, rnn_layers=layers,
                                                        rnn_type=rnn_type), seed=seed)


def case_policy(case, rnn_type="LSTM"):
    c = R.CASES[case]
    if rnn_type == "GRU":
        sd = synth.make_state_dict(G.spec(H=c["H"], W=c["W"], hidden=c["hidden"], A=c["A"], L=c["L"]), seed=c["wseed"])
    else:
        sd = R.state_dict(case)
    return make_policy(c["H"], c["W"], sd, hidden=c["hidden"], layers=c["L"], n_actions=c["A"], rnn_type=rnn_type)


def close(got, want, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got.reshape(want.shape) - want).max() / (np.abs(want).max() + 1e-6)
    return err < tol, err


def loss_close(got, want):
    return abs(got - want) < 1e-4 * max(1.0, abs(want))


def oracle_features(sd, depth):
    """The fp64 compression tap of the oracle on [B,H,W,1] frames, as [B, C, fh, fw]."""
    x = policy_oracle.avgpool2(np.asarray(depth, np.float64))
    comp = oracle.encoder_({k: np.asarray(v) for k, v in sd.items()}, np.ascontiguousarray(x), 16, pre=ENC)
    return np.ascontiguousarray(comp.transpose(0, 3, 1, 2))


def encode(pol, depth):
    return pol.net.visual_encoder({"depth": gpu(depth)})


# ------------------------------------------------------------------------------------------------------------------ 1. features
@functools.lru_cache(maxsize=None)
def feature_case(H, W, nmax):
    sd = weights(H, W, 128, 1)
    depth = synth.uniform(1000 + W, "depth", (nmax, H, W, 1), 0.0, 1.0).astype(np.float32)
    return sd, depth, oracle_features(sd, depth), make_policy(H, W, sd, hidden=128, layers=1)


@pytest.mark.parametrize("H,W,B,shape", [(96, 128, 1, (512, 2, 2)), (96, 128, 8, (512, 2, 2)), (96, 128, 9, (512, 2, 2)),
                                         (192, 341, 2, (114, 3, 6)), (192, 300, 3, (137, 3, 5))])
def test_visual_encoder_matches_the_fp64_compression_tap(H, W, B, shape):
    """GroupNorm works per sample, so the first B frames of the largest batch of a frame size share one oracle run."""
    sd, depth, ref, pol = feature_case(H, W, 9 if W == 128 else B)
    enc = pol.net.visual_encoder
    assert tuple(enc.output_shape) == shape and enc.is_blind is False
    got = encode(pol, depth[:B])
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B,) + shape and got.dtype == torch.float32 and got.device == DEV
    want = ref[:B]
    err = np.abs(got.cpu().double().numpy() - want).max() / np.abs(want).max()
    print(f"[features {W}x{H} B={B}] {err:.2e} of max|ref| (bound {ACT_TOL:.0e})")
    assert err <= ACT_TOL, err
    assert (got >= 0).all() and got.any()
    again = encode(pol, depth[:B])
    torch.cuda.synchronize()
    assert torch.equal(got, again)


def test_visual_encoder_applies_the_observation_transform():
    """RL.OBS_TRANSFORM resize_crop from a 160x200 frame to 128x96: the oracle runs on the frame torch's area resampling gives."""
    H, W, Hs, Ws, B = 96, 128, 160, 200, 2
    sd = weights(H, W, 128, 1)
    tr = ResizeCenterCropper((W, H))
    pol = make_policy(H, W, sd, hidden=128, layers=1, obs_transform=tr, frame=(Hs, Ws))
    assert tuple(pol.net.visual_encoder.output_shape) == (512, 2, 2)
    depth = synth.uniform(77, "depth", (B, Hs, Ws, 1), 0.0, 1.0).astype(np.float32)
    rs_h, rs_w, cy, cx, oh, ow = transformed_size(Hs, Ws, tr.mode, (W, H))
    assert (oh, ow) == (H, W)
    x = torch.from_numpy(depth).permute(0, 3, 1, 2).contiguous()
    y = F.interpolate(x, size=(rs_h, rs_w), mode="area")[..., cy:cy + oh, cx:cx + ow].permute(0, 2, 3, 1).contiguous().numpy()
    want = oracle_features(sd, y)
    got = encode(pol, depth).cpu().double().numpy()
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"[features resize_crop] {err:.2e} of max|ref|")
    assert err <= ACT_TOL, err


# ------------------------------------------------------------------------------------------------------------------ 2. act
@pytest.mark.parametrize("fname,rnn_type", [("policy_128x96_b2.npz", "LSTM"), ("policy_gru_128x96_h128_b2.npz", "GRU")])
def test_act_from_features_matches_the_recorded_fp64_steps(fname, rnn_type):
    rec = load_golden(fname)
    H, W, B, steps = (int(rec[k]) for k in ("H", "W", "B", "steps"))
    Hd, L, A = (int(rec.get(k, d)) for k, d in (("hidden", 512), ("layers", 2), ("n_actions", 4)))
    assert steps >= 3
    sd = weights(H, W, Hd, L, A, rnn_type, seed=int(rec["weight_seed"]))
    pol = make_policy(H, W, sd, hidden=Hd, layers=L, n_actions=A, rnn_type=rnn_type)
    hidden = torch.zeros(pol.num_recurrent_layers, B, Hd, device=DEV)
    for t, (depth, goal, prev, mask) in enumerate(synth.make_policy_inputs(H, W, B, steps, int(rec["input_seed"]), A)):
        obs = {FEAT: encode(pol, depth), GOAL: gpu(goal)}                       # no "depth" key
        pa, mk = gpu(prev).view(B, 1), gpu(mask).view(B, 1)
        feats, hnew, logits, value = pol.features_and_logits(obs, hidden, pa, mk)
        v2, action, logp, h2 = pol.act(obs, hidden, pa, mk, deterministic=True)
        v3 = pol.get_value(obs, hidden, pa, mk)
        torch.cuda.synchronize()
        assert torch.equal(h2, hnew) and torch.equal(v2, value) and torch.equal(v3, value)
        for key, got in (("features64", feats), ("hidden64", hnew), ("logits_raw64", logits), ("value64", value)):
            ok, err = close(got.cpu().numpy(), rec[f"{key}/{t}"])
            assert ok, (t, key, err)
        if f"action64/{t}" in rec:
            np.testing.assert_array_equal(action.cpu().numpy(), rec[f"action64/{t}"])
        hidden = hnew


# ------------------------------------------------------------------------------------------------------------------ 3. batch regimes
def regime_step(H, W, B, seed):
    """One step with a distinct frame, goal and non-zero incoming state per environment, masks 0 at b % 5 == 0 and at b = 64."""
    depth = synth.uniform(seed, "depth", (B, H, W, 1), 0.0, 1.0).astype(np.float32)
    goal = np.stack([synth.uniform(seed, "rho", (B,), 0.2, 6.0), synth.uniform(seed, "phi", (B,), -3.0, 3.0)], axis=-1).astype(np.float32)
    b = np.arange(B)
    zero = (b % 5 == 0) | (b == 64)
    prev = np.empty(B, np.int64)
    for sel in (zero, ~zero):
        idx = np.flatnonzero(sel)
        prev[idx] = np.arange(len(idx)) % 4
    return depth, goal, prev, np.where(zero, 0.0, 1.0).astype(np.float32)


def regime_hidden(L, B, Hd, seed):
    h = synth.uniform(seed, "h0", (L, B, Hd), -1.0, 1.0)
    c = synth.uniform(seed, "c0", (L, B, Hd), -3.0, 3.0)
    return np.concatenate([h, c]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def regime_policy(H, W):
    sd = weights(H, W, 512, 2)
    return sd, make_policy(H, W, sd, hidden=512, layers=2)


# 48 / 49: visual_fc's row kernel / GEMM; 64 / 65 / 130: the recurrent kernels' 64-sample chunks
@pytest.mark.parametrize("H,W,B", [(96, 128, 1), (96, 128, 5), (96, 128, 48), (96, 128, 49), (96, 128, 64), (96, 128, 65), (96, 128, 130),
                                   (192, 300, 5)])
def test_batch_regimes_from_features_match_the_oracle(H, W, B):
    sd, pol = regime_policy(H, W)
    L, Hd = 2, 512
    depth, goal, prev, mask = regime_step(H, W, B, 500 + B)
    hid = regime_hidden(L, B, Hd, 500 + B)
    obs = {FEAT: encode(pol, depth), GOAL: gpu(goal)}
    feats, hnew, logits, value = pol.features_and_logits(obs, gpu(hid), gpu(prev).view(B, 1), gpu(mask).view(B, 1))
    torch.cuda.synchronize()
    o = policy_oracle.policy_step(sd, depth, goal, prev, mask, hid.astype(np.float64))
    got = dict(features=feats, logits=logits, value=value)
    for k in got:
        ok, err = close(got[k].cpu().numpy(), o[k])
        assert ok, (B, k, err)
    for blk in range(2 * L):
        ok, err = close(hnew[blk].cpu().numpy(), o["hidden"][blk])
        assert ok, (B, "hidden", blk, err)


def test_gemm_and_row_kernel_agree_on_unaligned_rows():
    """F = 2055 at 49 rows (the GEMM, K not a multiple of its 32-wide step) against the same rows in two calls of the row kernel, which
    the oracle test above checks: float32-grade equal."""
    H, W, B = 192, 300, 49
    sd, pol = regime_policy(H, W)
    C_, fh, fw = pol.net.visual_encoder.output_shape
    assert C_ * fh * fw == 2055
    feats = torch.from_numpy(synth.uniform(9, "f", (B, C_, fh, fw), 0.0, 2.0).astype(np.float32)).to(DEV)
    _, goal, prev, mask = regime_step(8, 8, B, 9)
    hid = gpu(regime_hidden(2, B, 512, 9))
    run = lambda s: pol.features_and_logits({FEAT: feats[s], GOAL: gpu(goal)[s]}, hid[:, s].contiguous(), gpu(prev).view(B, 1)[s],
                                            gpu(mask).view(B, 1)[s])
    whole, a, b = run(slice(0, B)), run(slice(0, 48)), run(slice(48, B))
    torch.cuda.synchronize()
    for k, dim in ((0, 0), (1, 1), (2, 0), (3, 0)):
        parts = torch.cat([a[k], b[k]], dim=dim)
        ok, err = close(whole[k].cpu().numpy(), parts.cpu().numpy(), 2e-5)
        assert ok, (k, err)


# ------------------------------------------------------------------------------------------------------------------ 4. update
def run_update(pol, step, inp, li, use_clipped=True):
    """features from the case's frames, then evaluate_actions + ppo_loss + backward from them (no "depth" key)."""
    M = inp["T"] * inp["N"]
    obs = {FEAT: encode(pol, inp["depth"]), GOAL: gpu(inp["goal"])}
    value, logp, entropy, hout = step.evaluate_actions(obs, gpu(inp["hidden"]), gpu(inp["prev"]).view(M, 1), gpu(inp["masks"]).view(M, 1),
                                                       gpu(inp["actions"]).view(M, 1))
    del obs                                                   # the handle keeps its own copy of the feature rows
    t = lambda k: torch.from_numpy(li[k]).to(DEV)
    out3 = step.ppo_loss(t("old"), t("adv"), t("vp"), t("ret"), R.CLIP, R.VALUE_COEF, R.ENTROPY_COEF, use_clipped)
    step.backward()
    torch.cuda.synchronize()
    return dict(value=value.cpu().numpy(), logp=logp.cpu().numpy(), entropy=float(entropy), hidden=hout.cpu().numpy(),
                losses=out3.cpu().numpy().astype(np.float64), grad=step.grad.cpu().double().numpy())


def check_update(what, step, got, ref):
    for k in ("value", "logp", "hidden"):
        ok, err = close(got[k], ref[k])
        print(f"[{what}] {k}: {err:.2e} of scale")
        assert ok, (what, k, err)
    ok, err = close(got["entropy"], ref["entropy"])
    assert ok, (what, "entropy", err)
    for k, g, w in zip(("value_loss", "action_loss", "dist_entropy"), got["losses"], ref["losses"]):
        print(f"[{what}] {k}: {g:.8f} vs {w:.8f}")
        assert loss_close(g, w), (what, k, g, w)
    errs = {}
    for name, (off, n) in step.offsets.items():
        g, gr = got["grad"][off:off + n], ref["grads"][name].reshape(-1)
        if name.startswith(ENC):
            assert not g.any(), (what, name, "an encoder gradient is not exactly zero")
            continue
        if not gr.any():
            assert not g.any(), (what, name)
            continue
        errs[name] = np.linalg.norm(g - gr) / max(np.linalg.norm(gr), 1e-12)
    worst = max(errs, key=errs.get)
    print(f"[{what}] worst gradient tensor {errs[worst]:.2e} ({worst}), GRAD_TOL {GRAD_TOL:.1e}")
    assert "net.visual_fc.1.weight" in errs and "net.visual_fc.1.bias" in errs
    assert max(errs.values()) <= GRAD_TOL, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    lo, hi = step.encoder_range
    assert hi > lo and not got["grad"][lo:hi].any() and not got["grad"][step.n_params:].any()


@pytest.mark.parametrize("case,rnn_type,train_encoder", [("A", "LSTM", True), ("A", "LSTM", False), ("B1", "LSTM", True), ("C", "LSTM", True),
                                                         ("A", "GRU", True), ("S", "LSTM", True)])
def test_update_from_features_matches_fp64_autograd(case, rnn_type, train_encoder):
    gru = rnn_type == "GRU"
    pol = case_policy("B" if case == "B1" else case, rnn_type)
    step = PolicyTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM, train_encoder=train_encoder)
    ref = G.reference(case) if gru else R.reference(case)
    inp = G.gru_rollout(case) if gru else R.rollout(case)
    got = run_update(pol, step, inp, ref["loss_inputs"])
    check_update(f"{case} {rnn_type} train_encoder={train_encoder}", step, got, ref)
    again = run_update(pol, step, inp, ref["loss_inputs"])
    for k in ("value", "logp", "hidden", "losses", "grad"):
        assert np.array_equal(got[k], again[k]), k          # every reduction has a fixed order


# ------------------------------------------------------------------------------------------------------------------ 5. step
def test_step_from_features_leaves_the_encoder_alone_and_act_reads_the_new_weights():
    case = "A"
    pol = case_policy(case)
    step = PolicyTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM, train_encoder=True)
    ref = R.reference(case)
    newp, norm, coef, _ = R.clip_and_adam(ref["params"], ref["grads"], lr=LR, eps=EPS, max_norm=MAX_GRAD_NORM, frozen=(ENC,))
    assert coef < 1.0
    lo, hi = step.encoder_range
    step.exp_avg[lo:hi] = 0.1                                 # moments a checkpoint of a trained encoder would bring along
    step.exp_avg_sq[lo:hi] = 0.01
    fresh = R.rollout(case, 77)
    one = dict(fresh, depth=fresh["depth"][:3], goal=fresh["goal"][:3], prev=fresh["prev"][:3], masks=np.ones(3, np.float32),
               actions=fresh["actions"][:3], T=1, N=3)
    obs = {FEAT: encode(pol, one["depth"]), GOAL: gpu(one["goal"])}
    act = lambda: pol.act(obs, gpu(one["hidden"]), gpu(one["prev"]).view(3, 1), gpu(one["masks"]).view(3, 1), deterministic=True)
    value0, _, _, hidden0 = act()
    run_update(pol, step, R.rollout(case), ref["loss_inputs"])
    before, m0, v0 = step.flat.clone(), step.exp_avg.clone(), step.exp_avg_sq.clone()
    gnorm = step.clip_grad_norm()
    step.optimizer_step()
    torch.cuda.synchronize()
    assert abs(float(gnorm) - norm) < 1e-4 * norm
    assert torch.equal(before[lo:hi], step.flat[lo:hi]) and not torch.equal(before, step.flat)
    assert torch.equal(m0[lo:hi], step.exp_avg[lo:hi]) and torch.equal(v0[lo:hi], step.exp_avg_sq[lo:hi])
    worst = 0.0
    for name, (off, n) in step.offsets.items():
        got, want = step.flat[off:off + n].cpu().double().numpy(), newp[name].reshape(-1)
        g = ref["grads"][name].reshape(-1)
        sel = np.ones_like(g, bool) if name.startswith(ENC) else np.abs(g) > 1e-6 * max(np.abs(g).max(), 1e-30)
        worst = max(worst, np.abs(got[sel] - want[sel]).max(initial=0.0))
        np.testing.assert_allclose(got[sel], want[sel], rtol=0, atol=2e-6, err_msg=name)
    print(f"[step] worst parameter difference after clip + Adam: {worst:.2e}")
    v1, a1, lp1, h1 = act()
    torch.cuda.synchronize()
    wv, _, _, wh, wl = R.evaluate(newp, one)
    for k, g, w in (("value", v1, wv), ("hidden", h1, wh)):
        ok, err = close(g.cpu().numpy(), w)
        assert ok, ("act after the step", k, err)
    wlp = torch.log_softmax(torch.from_numpy(wl), -1).numpy()
    np.testing.assert_allclose(lp1.cpu().numpy()[:, 0], wlp[np.arange(3), a1.cpu().numpy()[:, 0]], rtol=0, atol=2e-4)
    assert not torch.equal(value0, v1) and not torch.equal(hidden0, h1)      # the feature path reads the new weights


# ------------------------------------------------------------------------------------------------------------------ 6. storage
def storage_run():
    """300x192, T = 4, N = 4, two minibatches: one rollout acted out once (from features), stored as features in one storage and as
    frames in another; the feature-fed policy and a twin with a frozen encoder each run PPO.update on theirs."""
    H, W, T, N, Hd, L, A = 192, 300, 4, 4, 128, 2, 4
    sd = weights(H, W, Hd, L, A, seed=21)
    pol_f = make_policy(H, W, sd, hidden=Hd, layers=L, n_actions=A)
    pol_d = make_policy(H, W, sd, hidden=Hd, layers=L, n_actions=A)
    enc = pol_f.net.visual_encoder
    shape = tuple(enc.output_shape)
    assert shape == (137, 3, 5) and (shape[0] * shape[1] * shape[2]) % 4 != 0
    space = Space({"depth": Box((H, W, 1)), FEAT: Box(shape), GOAL: Box((2,))})
    st_f = RolloutStorage(T, N, space, ActionSpace(A), Hd, 2 * L, sensors=[FEAT, GOAL])
    st_d = RolloutStorage(T, N, space, ActionSpace(A), Hd, 2 * L, sensors=["depth", GOAL])
    assert "depth" not in st_f.observations and tuple(st_f.observations[FEAT].shape) == (T + 1, N) + shape
    for st in (st_f, st_d):
        st.to(DEV)
    depth = [gpu(synth.uniform(900, f"depth{t}", (N, H, W, 1), 0.0, 1.0).astype(np.float32)) for t in range(T + 1)]
    goal = [gpu(np.stack([synth.uniform(900, f"rho{t}", (N,), 0.2, 6.0), synth.uniform(900, f"phi{t}", (N,), -3.0, 3.0)],
                         axis=-1).astype(np.float32)) for t in range(T + 1)]
    masks = [torch.ones(N, 1) for _ in range(T + 1)]
    masks[0][:] = 0.0
    masks[2][1] = 0.0
    feats = [enc({"depth": d}) for d in depth]
    st_f.observations[FEAT][0].copy_(feats[0])
    st_d.observations["depth"][0].copy_(depth[0])
    for st in (st_f, st_d):
        st.observations[GOAL][0].copy_(goal[0])
        st.masks[0].copy_(masks[0])
    hidden = torch.zeros(2 * L, N, Hd, device=DEV)
    prev = torch.zeros(N, 1, dtype=torch.int64, device=DEV)
    gen = torch.Generator(device="cpu").manual_seed(5)
    for t in range(T):
        value, action, logp, hidden = pol_f.act({FEAT: feats[t], GOAL: goal[t]}, hidden, prev, masks[t].to(DEV), deterministic=True)
        action = torch.randint(0, A, (N, 1), generator=gen).to(DEV)           # off-policy actions: every action occurs
        rewards = torch.rand(N, 1, generator=gen) - 0.5
        st_f.insert({FEAT: feats[t + 1], GOAL: goal[t + 1]}, hidden, action, logp - 0.1, value, rewards, masks[t + 1])
        st_d.insert({"depth": depth[t + 1], GOAL: goal[t + 1]}, hidden, action, logp - 0.1, value, rewards, masks[t + 1])
        prev = action
    next_value = pol_f.get_value({FEAT: feats[T], GOAL: goal[T]}, hidden, prev, masks[T].to(DEV))
    for p in pol_d.net.visual_encoder.parameters():
        p.requires_grad_(False)                                # what the reference trainers do for train_encoder False
    out = []
    for pol, st in ((pol_f, st_f), (pol_d, st_d)):
        st.compute_returns(next_value, True, 0.99, 0.95)
        agent = PPO(pol, R.CLIP, 1, 2, R.VALUE_COEF, R.ENTROPY_COEF, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM,
                    use_clipped_value_loss=True, use_normalized_advantage=True)
        torch.manual_seed(2024)
        losses = agent.update(st)
        torch.cuda.synchronize()
        assert agent.train_step.step_count == 2
        out.append((losses, {k: v.detach().cpu().clone() for k, v in pol.state_dict().items()}, agent.train_step))
    assert out[0][2].train_encoder and not out[1][2].train_encoder
    return out, sd


def test_ppo_update_from_a_storage_of_features_matches_the_frozen_frames_twin():
    (feat_run, depth_run), sd = storage_run()
    for k, a, b in zip(("value_loss", "action_loss", "dist_entropy"), feat_run[0], depth_run[0]):
        print(f"[storage] {k}: features {a:.8f} vs frames {b:.8f}")
        assert np.isfinite(a) and loss_close(a, b), (k, a, b)
    worst, moved = 0.0, 0
    for name in sd:
        a, b = feat_run[1][name].double().numpy(), depth_run[1][name].double().numpy()
        worst = max(worst, np.abs(a - b).max())
        np.testing.assert_allclose(a, b, rtol=0, atol=2e-6, err_msg=name)
        if name.startswith(ENC):
            assert np.array_equal(a, np.asarray(sd[name], np.float32)), name     # the encoder did not move
        else:
            moved += int(not np.array_equal(a, np.asarray(sd[name], np.float32)))
    print(f"[storage] worst parameter difference between the twins: {worst:.2e}")
    assert moved >= 10
    (again, _), _ = storage_run()
    assert again[0] == feat_run[0]
    for name in sd:
        assert torch.equal(again[1][name], feat_run[1][name]), name


# ------------------------------------------------------------------------------------------------------------------ 7. errors
def test_wrong_shape_and_missing_key_raise_before_any_launch():
    sd, pol = regime_policy(96, 128)
    B = 2
    hid, pa, mk = torch.zeros(4, B, 512, device=DEV), torch.zeros(B, 1, dtype=torch.int64, device=DEV), torch.ones(B, 1, device=DEV)
    goal = torch.zeros(B, 2, device=DEV)
    bad = torch.zeros(B, 512, 2, 3, device=DEV)
    with pytest.raises(ValueError, match=r"\(2, 512, 2, 3\).*\('B', 512, 2, 2\)"):
        pol.act({FEAT: bad, GOAL: goal}, hid, pa, mk)
    with pytest.raises(ValueError, match="neither 'visual_features' nor 'depth'"):
        pol.act({GOAL: goal}, hid, pa, mk)
    step = PolicyTrainStep(case_policy("A"), lr=LR, eps=EPS)
    c = R.CASES["A"]
    hid = torch.zeros(2 * c["L"], B, c["hidden"], device=DEV)
    with pytest.raises(ValueError, match=r"\(2, 512, 2, 3\).*\('B', 512, 2, 2\)"):
        step.evaluate_actions({FEAT: bad, GOAL: goal}, hid, pa, mk, pa)
    with pytest.raises(ValueError, match="neither 'visual_features' nor 'depth'"):
        step.evaluate_actions({GOAL: goal}, hid, pa, mk, pa)
    step.policy._release()


def test_overlapping_hidden_buffers_are_refused_on_the_feature_entry_points():
    pol = case_policy("A")
    step = PolicyTrainStep(pol, lr=LR, eps=EPS)
    c = R.CASES["A"]
    B, Hd, L = 3, c["hidden"], c["L"]
    n = 2 * L * B * Hd
    feats = torch.zeros((B,) + tuple(pol.net.visual_encoder.output_shape), device=DEV)
    goal, pa, mk = torch.zeros(B, 2, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV), torch.ones(B, device=DEV)
    out = [torch.full(s, 7.0, device=DEV) for s in ((B, Hd), (B, c["A"]), (B,))]
    p = lambda t: C.c_void_p(t.data_ptr())
    for off in (0, B * Hd):
        buf = torch.zeros(2 * n, device=DEV)
        before = buf.clone()
        hin, hout = C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + 4 * off)
        with torch.cuda.device(DEV):
            stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
            rc = _lib.lib.pnvo_policy_act_features(pol._handle, p(feats), p(goal), p(pa), p(mk), hin, B, hout, p(out[0]), p(out[1]),
                                                   p(out[2]), stream)
            assert rc == -1 and "overlap" in _lib.lib.pnvo_last_error(None).decode(), (off, rc)
            rc = _lib.lib.pnvo_policy_evaluate_features(pol._handle, p(feats), p(goal), p(pa), p(mk), hin, 1, B, p(pa), hout, p(out[2]),
                                                        None, None, stream)
            assert rc == -1 and "overlap" in _lib.lib.pnvo_last_error(None).decode(), (off, rc)
        torch.cuda.synchronize()
        assert torch.equal(buf, before) and all((t == 7).all() for t in out)
    pol._release()


def live():
    gc.collect()
    torch.cuda.synchronize()
    return _lib.lib.pnvo_device_bytes_live()


def test_feature_path_memory_is_counted_and_released():
    base = live()
    pol = case_policy("A")
    inp, ref = R.rollout("A"), R.reference("A")
    feats = encode(pol, inp["depth"][:3])
    c = R.CASES["A"]
    hid = torch.zeros(2 * c["L"], 3, c["hidden"], device=DEV)
    pol.act({FEAT: feats, GOAL: gpu(inp["goal"][:3])}, hid, gpu(inp["prev"][:3]).view(3, 1), torch.ones(3, 1, device=DEV))
    first = live()
    assert first > base
    pol.act({FEAT: feats, GOAL: gpu(inp["goal"][:3])}, hid, gpu(inp["prev"][:3]).view(3, 1), torch.ones(3, 1, device=DEV))
    assert live() == first
    step = PolicyTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    run_update(pol, step, inp, ref["loss_inputs"])
    steady = live()
    run_update(pol, step, inp, ref["loss_inputs"])
    assert live() == steady
    pol._release()
    assert live() == base
