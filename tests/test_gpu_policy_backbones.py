"""GPU (-m gpu): the Bottleneck / ResNeXt / SE-ResNeXt backbones of the navigation policy (and of the VO models) on the HIP path: the
grouped 3x3 conv (conv_group.hip) and the squeeze-and-excite gate (se_gate.hip) behind PointNavResNetPolicy(backbone=...).

  1. every case of tests/golden/policy_backbones_136x104_h128_b2.npz (recorded from the imported reference in float64): act steps,
     features, hidden, logits, value, and net.visual_encoder(obs) against the recorded encoder output;
  2. each of the six backbones at B = 5 and B = 9 (no multiples of the encoder's sample chunks) against the float64 restatement of
     tests/backbone_reference.py, depth input, and once rgb + depth uint8 with normalisation;
  3. the same call twice is bit-identical;
  4. se_resneXt50 with a frozen encoder, T = 3, N = 2, a mid-sequence reset: one update from frames and one from visual_features
     against the restatement's update (criteria of tests/test_gpu_static_encoder.py), the encoder's parameters and Adam moments
     untouched;
  5. the VO model on se_resneXt50 against the recorded reference output, with the block taps against the restatement (the tap
     mechanism lives on the VO handle; the policy's encoder handle is not reachable from Python, so the policy's block outputs are
     covered through this model and through everything downstream of them);
  6. a resnet18 policy built after a se_resneXt50 one in the same process still matches its own golden.

Frames are 104 x 136: stage maps 13x17, 7x9, 4x5, 2x3 (every stride-2 grouped conv sees an odd input), compression 341 channels.
Criterion: 2e-4 of each tensor's scale (tests/test_gpu_policy.py); the reference's own float32 run sits at 2 - 3e-6 on these models.
"""
import functools

import numpy as np
import pytest
import torch

import backbone_reference as BR
from conftest import load_golden
from pointnav_vo_amd import synth
from pointnav_vo_amd.policy import PointNavResNetPolicy, policy_state_dict_spec
from pointnav_vo_amd.ppo import PPO
from pointnav_vo_amd.vo_cnn import VisualOdometryCNNBase

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GOAL, FEAT, ENC = BR.GOAL, "visual_features", BR.ENC
TOL, GRAD_TOL = 2e-4, 1.0e-4
LR, EPS, MAX_GRAD_NORM = 2.5e-4, 1e-5, 0.2               # configs/rl/ddppo_pointnav.yaml
BACKBONES = ["resnet50", "resnet101", "resneXt50", "se_resnet50", "se_resneXt50", "se_resneXt101"]


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class Act:
    def __init__(self, n):
        self.n = n


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_policy(sd, backbone, vis=("depth",), rnn="LSTM", normalize=False, H=BR.H, W=BR.W, hidden=BR.HIDDEN):
    space = Space({"depth": Box((H, W, 1)), "rgb": Box((H, W, 3)), GOAL: Box((2,))})
    pol = PointNavResNetPolicy(observation_space=space, action_space=Act(BR.N_ACT), hidden_size=hidden, rnn_type=rnn,
                               num_recurrent_layers=BR.LAYERS, backbone=backbone, goal_sensor_uuid=GOAL,
                               normalize_visual_inputs=normalize, obs_transform=None, vis_types=list(vis))
    assert list(pol.state_dict().keys()) == list(sd.keys())
    pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return pol.to(DEV).eval()


def err_of(got, want):
    want = np.asarray(want, np.float64)
    got = np.asarray(got, np.float64).reshape(want.shape)
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-6))


def check(what, got, want, tol=TOL):
    e = err_of(got.detach().cpu().numpy() if torch.is_tensor(got) else got, want)
    print(f"[{what}] {e:.2e} of scale (bound {tol:.0e})")
    assert np.isfinite(e) and e < tol, (what, e)


def obs_of(frames, goal):
    obs = {k: gpu(v) for k, v in frames.items()}
    obs[GOAL] = gpu(goal)
    return obs


# ------------------------------------------------------------------------------------------------------------------ 1. fixture
@pytest.mark.parametrize("case", list(BR.CASES))
def test_fixture_case_matches_the_recorded_reference(case):
    rec = load_golden("policy_backbones_136x104_h128_b2.npz")
    c = BR.CASES[case]
    B = int(rec["B"])
    pol = make_policy(BR.state_dict(case), c["backbone"], c["vis"], c["rnn"], c["normalize"])
    assert tuple(pol.net.visual_encoder.output_shape) == (341, 2, 3)
    hidden = torch.zeros(pol.num_recurrent_layers, B, BR.HIDDEN, device=DEV)
    for t, (frames, goal, prev, mask) in enumerate(BR.step_inputs(case)):
        obs = obs_of(frames, goal)
        pa, mk = gpu(prev).view(B, 1), gpu(mask).view(B, 1)
        enc = pol.net.visual_encoder(obs)
        feats, hnew, logits, value = pol.features_and_logits(obs, hidden, pa, mk)
        v2, action, logp, h2 = pol.act(obs, hidden, pa, mk, deterministic=True)
        torch.cuda.synchronize()
        assert torch.equal(h2, hnew) and torch.equal(v2, value)
        assert tuple(enc.shape) == (B, 341, 2, 3) and (enc >= 0).all()
        check(f"{case}/{t} encoder", enc, rec[f"{case}/encoder64/{t}"])
        for key, got in (("features64", feats), ("hidden64", hnew), ("logits_raw64", logits), ("value64", value)):
            check(f"{case}/{t} {key}", got, rec[f"{case}/{key}/{t}"])
        # the visual_features path on the same encoder output
        f2, h3, l3, v3 = pol.features_and_logits({FEAT: enc, GOAL: obs[GOAL]}, hidden, pa, mk)
        check(f"{case}/{t} hidden from features", h3, rec[f"{case}/hidden64/{t}"])
        hidden = hnew
    pol._release()


# ------------------------------------------------------------------------------------------------------------------ 2. batches
NB = 9


@functools.lru_cache(maxsize=None)
def batch_reference(backbone, rgbd):
    """One float64 restatement step of NB environments with distinct frames and a non-zero incoming state; every sample is independent
    of the others (GroupNorm, the SE squeeze and the recurrent core work per sample), so smaller batches are its first rows."""
    vis, normalize = (("rgb", "depth"), True) if rgbd else (("depth",), False)
    sd = BR.state_dict(backbone=backbone, vis=vis, normalize=normalize, rnn="LSTM")
    rgb, depth, goal, prev, _ = synth.make_policy_rgbd_inputs(BR.H, BR.W, NB, 1, 700 + len(backbone), BR.N_ACT)[0]
    mask = np.ones(NB, np.float32)
    mask[[0, 5]] = 0.0
    h0 = synth.uniform(71, "h0", (BR.LAYERS, NB, BR.HIDDEN), -1.0, 1.0)
    c0 = synth.uniform(71, "c0", (BR.LAYERS, NB, BR.HIDDEN), -3.0, 3.0)
    hidden = np.concatenate([h0, c0]).astype(np.float32)
    frames = {"rgb": rgb, "depth": depth} if rgbd else {"depth": depth}
    ref = BR.policy_step(sd, frames, goal, prev, mask, hidden, "LSTM")
    return sd, frames, goal, prev, mask, hidden, ref, vis, normalize


@pytest.mark.parametrize("backbone,rgbd", [(b, False) for b in BACKBONES] + [("se_resneXt50", True)])
def test_batches_match_the_float64_restatement_and_repeat_bit_for_bit(backbone, rgbd):
    sd, frames, goal, prev, mask, hidden, ref, vis, normalize = batch_reference(backbone, rgbd)
    pol = make_policy(sd, backbone, vis, "LSTM", normalize)
    for B in (5, NB):
        obs = obs_of({k: v[:B] for k, v in frames.items()}, goal[:B])
        if rgbd:
            assert obs["rgb"].dtype == torch.uint8
        hin, pa, mk = gpu(hidden[:, :B]), gpu(prev[:B]).view(B, 1), gpu(mask[:B]).view(B, 1)
        enc = pol.net.visual_encoder(obs)
        out = pol.features_and_logits(obs, hin, pa, mk)
        torch.cuda.synchronize()
        check(f"{backbone} B={B} encoder", enc, ref["encoder"][:B])
        for k, got, want in (("features", out[0], ref["features"][:B]), ("hidden", out[1], ref["hidden"][:, :B]),
                             ("logits", out[2], ref["logits"][:B]), ("value", out[3], ref["value"][:B])):
            check(f"{backbone} B={B} {k}", got, want)
        again, enc2 = pol.features_and_logits(obs, hin, pa, mk), pol.net.visual_encoder(obs)       # 3. the same call twice
        torch.cuda.synchronize()
        assert torch.equal(enc, enc2) and all(torch.equal(a, b) for a, b in zip(out, again)), (backbone, B)
    pol._release()


# ------------------------------------------------------------------------------------------------------------------ 4. update
def frozen_agent(pol):
    for p in pol.net.visual_encoder.parameters():
        p.requires_grad_(False)                                # what the reference trainers do for train_encoder False
    agent = PPO(pol, BR.G.CLIP, 1, 1, BR.G.VALUE_COEF, BR.G.ENTROPY_COEF, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM,
                use_clipped_value_loss=True, use_normalized_advantage=True)
    assert not agent.train_step.train_encoder
    return agent


@pytest.mark.parametrize("source", ["frames", "visual_features"])
def test_frozen_encoder_update_matches_the_restatement(source):
    ref = BR.ppo_reference()
    inp, li = BR.ppo_rollout(), ref["loss_inputs"]
    assert BR.G.census_ok(ref["value"], ref["logp"], li)       # every branch of both clamps is live, none within 1e-6 of a boundary
    M = inp["T"] * inp["N"]
    sd = BR.state_dict(**{k: BR.PPO[k] for k in ("backbone", "vis", "normalize", "rnn")})
    pol = make_policy(sd, BR.PPO["backbone"])
    agent = frozen_agent(pol)
    step = agent.train_step
    lo, hi = step.encoder_range
    step.exp_avg[lo:hi] = 0.1                                  # moments a checkpoint of a trained encoder would bring along
    step.exp_avg_sq[lo:hi] = 0.01
    before, m0, v0 = step.flat.clone(), step.exp_avg.clone(), step.exp_avg_sq.clone()
    if source == "frames":
        obs = {"depth": gpu(inp["depth"]), GOAL: gpu(inp["goal"])}
    else:
        obs = {FEAT: pol.net.visual_encoder({"depth": gpu(inp["depth"])}), GOAL: gpu(inp["goal"])}
    value, logp, entropy, hout = pol.evaluate_actions(obs, gpu(inp["hidden"]), gpu(inp["prev"]).view(M, 1), gpu(inp["masks"]).view(M, 1),
                                                      gpu(inp["actions"]).view(M, 1))
    t = lambda k: torch.from_numpy(li[k]).to(DEV)
    out3 = step.ppo_loss(t("old"), t("adv"), t("vp"), t("ret"), BR.G.CLIP, BR.G.VALUE_COEF, BR.G.ENTROPY_COEF, True)
    step.backward()
    torch.cuda.synchronize()
    for k, got in (("value", value), ("logp", logp), ("hidden", hout)):
        check(f"update from {source}: {k}", got, ref[k])
    check(f"update from {source}: entropy", entropy.reshape(1), np.array([ref["entropy"]]))
    for k, g, w in zip(("value_loss", "action_loss", "dist_entropy"), out3.cpu().numpy().astype(np.float64), ref["losses"]):
        print(f"[update from {source}] {k}: {g:.8f} vs {w:.8f}")
        assert abs(g - w) < 1e-4 * max(1.0, abs(w)), (k, g, w)
    grad = step.grad.cpu().double().numpy()
    errs = {}
    for name, (off, n) in step.offsets.items():
        g, gr = grad[off:off + n], ref["grads"][name].reshape(-1)
        if name.startswith(ENC):
            assert not g.any(), (name, "an encoder gradient is not exactly zero")
        elif gr.any():
            errs[name] = np.linalg.norm(g - gr) / max(np.linalg.norm(gr), 1e-12)
        else:
            assert not g.any(), name
    worst = max(errs, key=errs.get)
    print(f"[update from {source}] worst gradient tensor {errs[worst]:.2e} ({worst}), GRAD_TOL {GRAD_TOL:.1e}")
    assert "net.visual_fc.1.weight" in errs and max(errs.values()) <= GRAD_TOL, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    # clip + Adam: everything but the encoder moves to where float64 puts it; the encoder and its moments stay bit for bit
    newp, norm, coef, _ = BR.G.clip_and_adam(ref["params"], ref["grads"], lr=LR, eps=EPS, max_norm=MAX_GRAD_NORM, frozen=(ENC,))
    gnorm = step.clip_grad_norm()
    step.optimizer_step()
    torch.cuda.synchronize()
    assert abs(float(gnorm) - norm) < 1e-4 * norm
    assert torch.equal(before[lo:hi], step.flat[lo:hi]) and not torch.equal(before, step.flat)
    assert torch.equal(m0[lo:hi], step.exp_avg[lo:hi]) and torch.equal(v0[lo:hi], step.exp_avg_sq[lo:hi])
    for name, (off, n) in step.offsets.items():
        got, want = step.flat[off:off + n].cpu().double().numpy(), newp[name].reshape(-1)
        g = ref["grads"][name].reshape(-1)
        sel = np.ones_like(g, bool) if name.startswith(ENC) else np.abs(g) > 1e-6 * max(np.abs(g).max(), 1e-30)
        np.testing.assert_allclose(got[sel], want[sel], rtol=0, atol=2e-6, err_msg=name)
    # act after the step reads the new heads and the unchanged encoder
    one = dict(inp, depth=inp["depth"][:2], goal=inp["goal"][:2], prev=inp["prev"][:2], masks=np.ones(2, np.float32),
               actions=inp["actions"][:2], T=1, N=2)
    with BR.policy() as g_:
        with torch.no_grad():
            P = BR.G.R.leaves(newp, torch.float64)
            wv, _, _, wh, _, _, _ = g_.forward(P, None, one, torch.float64, "LSTM", False)
    v1, _, _, h1 = pol.act({"depth": gpu(one["depth"]), GOAL: gpu(one["goal"])}, gpu(one["hidden"]), gpu(one["prev"]).view(2, 1),
                           torch.ones(2, 1, device=DEV), deterministic=True)
    check(f"act after the step ({source}): value", v1, wv.detach().numpy())
    check(f"act after the step ({source}): hidden", h1, wh.detach().numpy())
    pol._release()


# ------------------------------------------------------------------------------------------------------------------ 5. VO model
def test_vo_model_on_se_resnext50_matches_the_recorded_reference_and_its_block_taps():
    rec = load_golden("policy_backbones_136x104_h128_b2.npz")
    v = BR.VO
    sd, obs = BR.vo_inputs()
    model = VisualOdometryCNNBase(observation_space=list(v["space"]), observation_size=(v["W"], v["H"]), hidden_size=v["hidden"],
                                  backbone=v["backbone"], normalize_visual_inputs=True, output_dim=3,
                                  discretized_depth_channels=v["dd_bins"])
    assert list(model.state_dict().keys()) == list(sd.keys())
    model.load_state_dict({k: torch.from_numpy(np.array(t)) for k, t in sd.items()})
    model = model.to(DEV).eval()
    tobs = {k: gpu(t) for k, t in obs.items()}
    with torch.no_grad():
        out = model(tobs)
    torch.cuda.synchronize()
    want = rec["vo/out64"]
    rel = np.linalg.norm(out.cpu().double().numpy() - want, axis=-1) / np.maximum(np.linalg.norm(want, axis=-1), 1e-2)
    print(f"[vo se_resneXt50] per-pair relative error {rel}")
    assert (rel < TOL).all(), rel
    assert model.layer_kernel("visual_encoder.backbone.layer2.0.convs.3", v["B"])[0] == "group"
    taps = {}
    params = {k: torch.as_tensor(np.asarray(t)).double() for k, t in sd.items()}
    with torch.no_grad():
        BR.encoder_forward(params, params, {k: torch.as_tensor(t) for k, t in obs.items()}, ngroups=16, train=False, record=taps)
    for name in ("layer1.0", "layer2.0", "layer3.0", "layer4.0", "layer4.2"):
        with torch.no_grad():
            _, got = model.tap(name, tobs)
        check(f"vo tap {name}", got, taps[name].permute(0, 2, 3, 1).numpy(), 2e-5)


# ------------------------------------------------------------------------------------------------------------------ 6. resnet18 after
def test_resnet18_policy_built_after_a_se_resnext50_one_matches_its_golden():
    first = make_policy(BR.state_dict("a"), "se_resneXt50")
    frames, goal, prev, mask = BR.step_inputs("a")[0]
    first.act(obs_of(frames, goal), torch.zeros(4, 2, BR.HIDDEN, device=DEV), gpu(prev).view(2, 1), gpu(mask).view(2, 1))
    rec = load_golden("policy_128x96_b2.npz")
    H, W, B, steps = (int(rec[k]) for k in ("H", "W", "B", "steps"))
    sd = synth.make_state_dict(policy_state_dict_spec(width=W, height=H), seed=int(rec["weight_seed"]))
    pol = make_policy(sd, "resnet18", H=H, W=W, hidden=512)
    hidden = torch.zeros(4, B, 512, device=DEV)
    for t, (depth, goal, prev, mask) in enumerate(synth.make_policy_inputs(H, W, B, steps, int(rec["input_seed"]), 4)):
        feats, hnew, logits, value = pol.features_and_logits({"depth": gpu(depth), GOAL: gpu(goal)}, hidden, gpu(prev).view(B, 1),
                                                             gpu(mask).view(B, 1))
        for key, got in (("features64", feats), ("hidden64", hnew), ("logits_raw64", logits), ("value64", value)):
            check(f"resnet18 after se_resneXt50 {key}/{t}", got, rec[f"{key}/{t}"])
        hidden = hnew
    first._release()
    pol._release()
