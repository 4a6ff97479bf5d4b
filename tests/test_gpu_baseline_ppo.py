"""GPU (-m gpu): one PPO minibatch update of the baseline navigation policy (pointnav_vo_amd.ppo.BaselineTrainStep on
pnvo_baseline_evaluate / _ppo_loss / _backward / _clip_grad_norm: SimpleCNN's backward, BPTT through the GRU, Adam on the flat buffer)
against the torch-CPU float64 model of tests/baseline_ppo_reference.py (autograd), which tests/test_baseline_ppo_host.py pins to the
reference's own evaluate_actions, loss lines and backward.

Cases (hidden 128 unless said; the smallest shapes at which each kernel can still go wrong) —
  A   rgb-d uint8, 85x53 (maps 12x20, 5x9, 3x7: conv1 drops a remainder row and column, no pixel count is a multiple of 16), T = 5,
      N = 3: a start reset, one environment reset mid-sequence, two at once, a non-zero initial state
  Ap  the same frames as float32 rgb: gradients bit-equal to A's
  B   depth, 64x64 (maps 15, 6, 4: conv2 drops a row and a column of its input), T = 4, N = 1;  B1: the same policy, T = 1, N = 4
  C   rgb only, 85x53, T = 2, N = 2
  D   depth, 36 wide x 37 high, the smallest frame: conv3 has one output row, T = 2, N = 1
  E   blind, T = 3, N = 2
  F   rgb-d, 341x192, hidden 512, T = 2, N = 2: the Linear has 33 K slices and a 51 MB weight, conv2 drops a row

Tolerances.  Forward: baseline_policy_reference.TOL = 2e-4 of each tensor's scale.  Loss: 1e-4 * max(1, |x|).  Gradients, relative L2
per parameter tensor: the float64 model run in float32 on the CPU (python tests/baseline_ppo_reference.py) deviates from its float64
self by at most
    Intel Xeon host, 8 threads    A 2.850e-06   B 1.011e-05   B1 7.550e-05   C 6.432e-06   D 1.424e-06   E 2.216e-07   F 1.447e-06
    AMD EPYC host, 16 threads     A 1.364e-06   B 5.082e-06   B1 3.993e-05   C 7.350e-06   D 1.672e-06   E 4.148e-07   F 1.166e-06
(worst tensor: critic.fc.bias in B, B1 and C — a sum of a few signed d value, whose float32 figure moves with the CPU's instruction set
and thread count: B1 reads 7.5e-06 on 2 and 4 threads of the first machine — and weight_hh_l0, critic.fc.weight or cnn.0.weight
elsewhere; medians 1e-07 to 1e-06).  GRAD_TOL = 10 x the worst of both machines = 7.55e-4, the rule that gave GRAD_TOL of
tests/test_gpu_ppo.py and tests/test_gpu_ppo_gru.py: what a float32 framework itself loses.  Step: on the shipped optimiser settings
(lr 2.5e-4, eps 1e-5, max_grad_norm 0.2) the float32 CPU model's gradients put the parameters within
    Xeon   A 5.29e-08   B 6.70e-08   B1 4.84e-08   C 3.96e-08   D 2.10e-08   E 1.14e-08   F 3.06e-08
    EPYC   A 5.89e-08   B 7.93e-08   B1 3.83e-08   C 4.26e-08   D 3.67e-08   E 1.15e-08   F 2.02e-08
of the float64 ones after clip + Adam: STEP_ATOL = 10 x the worst (7.932e-08) = 7.94e-7.

Bit-equality with the act path: value and the final state come out of the same kernels in the same summation order and are compared
bit for bit.  act's log-probabilities are torch.log_softmax of the library's logits while evaluate's come from heads_eval_kernel
(x - (max + log(sum exp))): the same logits, another association of the same three terms, so they are compared at 4 float32 ulps of
max(1, |x|) instead.
"""
import functools

import numpy as np
import pytest
import torch

import baseline_policy_reference as BR
import baseline_ppo_reference as P
from pointnav_vo_amd import PointNavBaselinePolicy
from pointnav_vo_amd.ddppo import DDPPO
from pointnav_vo_amd.ppo import PPO, BaselineTrainStep
from pointnav_vo_amd.rollout_storage import RolloutStorage

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TOL = BR.TOL
GRAD_TOL = 7.55e-4
STEP_ATOL = 7.94e-7
# MEASURED (MI355X, the tests' own printout).  Worst gradient tensor, relative L2 against float64 autograd (median over the tensors):
#   A 1.26e-06 cnn.6.weight (1.08e-06)   B 4.52e-06 critic.fc.bias (9.40e-07)   B1 3.94e-05 critic.fc.bias (6.49e-07)
#   C 1.84e-06 critic.fc.bias (6.33e-07)   D 1.96e-06 weight_hh_l0 (5.06e-07)   E 2.29e-07 weight_hh_l0 (1.64e-07)
#   F 9.81e-07 weight_hh_l0 (8.15e-07)                                                   -> 3.94e-05 against GRAD_TOL 7.55e-04
#   forward, of scale: value <= 1.8e-06, logp <= 4.9e-07, hidden <= 2.2e-06 (TOL 2e-04); losses within 1.5e-07 (1e-04)
#   after clip + Adam: A 4.43e-08, E 6.71e-08 (STEP_ATOL 7.94e-07); PPO.update over the storage (4 steps): losses within 1.8e-07
LR, EPS, MAX_GRAD_NORM = P.LR, P.EPS, P.MAX_GRAD_NORM
GOAL = P.GOAL
ULP4 = 4 * 2.0 ** -23


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class Act:
    def __init__(self, n):
        self.n = n


class ActionSpace(Act):                                   # RolloutStorage asks for the class by this name
    pass


def space(case):
    c = P.CASES[case]
    d = {GOAL: Box((2,))}
    if "rgb" in c["vis"]:
        d["rgb"] = Box((c["H"], c["W"], 3))
    if "depth" in c["vis"]:
        d["depth"] = Box((c["H"], c["W"], 1))
    return Space(d)


def make_policy(case, device=DEV):
    pol = PointNavBaselinePolicy(space(case), Act(P.N_ACTIONS), GOAL, P.CASES[case]["hidden"])
    sd = P.state_dict(case)
    assert list(pol.state_dict().keys()) == list(sd.keys())
    pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return pol.to(device).eval()


def close(got, want, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max() + 1e-6
    err = np.abs(got.reshape(want.shape) - want).max() / scale
    return err < tol, err


def loss_close(got, want):
    return abs(got - want) < 1e-4 * max(1.0, abs(want))


def to_gpu(inp, rgb_float=False):
    M = inp["T"] * inp["N"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    obs = {GOAL: t(inp["goal"])}
    if inp["rgb"] is not None:
        obs["rgb"] = t(inp["rgb"]).float() if rgb_float else t(inp["rgb"])
    if inp["depth"] is not None:
        obs["depth"] = t(inp["depth"])
    prev = torch.zeros(M, 1, dtype=torch.int64, device=DEV)
    return obs, t(inp["hidden"]), prev, t(inp["masks"]).view(M, 1), t(inp["actions"]).view(M, 1)


def run_update(step, inp, li, rgb_float=False):
    """evaluate_actions + ppo_loss + backward on the GPU -> numpy results (the gradient buffer is copied out)."""
    obs, hidden, prev, masks, actions = to_gpu(inp, rgb_float)
    value, logp, entropy, hout = step.evaluate_actions(obs, hidden, prev, masks, actions)
    del obs                                                 # the handle keeps what the backward reads
    t = lambda k: torch.from_numpy(li[k]).to(DEV)
    out3 = step.ppo_loss(t("old"), t("adv"), t("vp"), t("ret"), P.CLIP, P.VALUE_COEF, P.ENTROPY_COEF, True)
    step.backward()
    torch.cuda.synchronize()
    return dict(value=value.cpu().numpy(), logp=logp.cpu().numpy(), entropy=float(entropy), hidden=hout.cpu().numpy(),
                losses=out3.cpu().numpy().astype(np.float64), grad=step.grad.cpu().numpy().copy(), shapes=(value.shape, logp.shape))


@functools.lru_cache(maxsize=None)
def gpu_case(case):
    """The policy of a case with a train step attached and one update's results, shared by the forward / loss / gradient tests.
    B1 runs on B's policy and step (a workspace sized for N = 1 meets N = 4), Ap on A's with float32 rgb."""
    base = {"B1": "B", "Ap": "A"}.get(case)
    if base:
        pol, step, _ = gpu_case(base)
    else:
        pol = make_policy(case)
        step = BaselineTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    ref_case = "A" if case == "Ap" else case
    return pol, step, run_update(step, P.rollout(ref_case), P.reference(ref_case)["loss_inputs"], rgb_float=case == "Ap")


def grad_errors(step, grad, ref_grads, what):
    """Per-tensor relative L2 against float64 autograd (denominator floor 1e-12); a zero reference gradient must be exactly zero."""
    errs = {}
    for name, (off, n) in step.offsets.items():
        g, gr = grad[off:off + n].astype(np.float64), ref_grads[name].reshape(-1)
        if not gr.any():
            assert not g.any(), (what, name, "reference gradient is exactly zero, the HIP gradient is not")
            continue
        errs[name] = np.linalg.norm(g - gr) / max(np.linalg.norm(gr), 1e-12)
    worst = max(errs, key=errs.get)
    print(f"[{what}] worst gradient tensor {errs[worst]:.2e} ({worst}), median {np.median(list(errs.values())):.2e}, GRAD_TOL {GRAD_TOL:.2e}")
    return errs


CASES = ["A", "B", "B1", "C", "D", "E", "F"]


# ------------------------------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("case", CASES)
def test_forward_matches_fp64_and_is_bit_equal_to_the_act_path(case):
    pol, step, got = gpu_case(case)
    ref, inp = P.reference(case), P.rollout(case)
    T, N, M, Hd = inp["T"], inp["N"], inp["T"] * inp["N"], P.CASES[case]["hidden"]
    assert got["shapes"] == ((M, 1), (M, 1)) and got["hidden"].shape == (1, N, Hd)
    for k in ("value", "logp", "hidden"):
        ok, err = close(got[k], ref[k])
        print(f"[{case}] {k}: {err:.2e} of scale")
        assert ok, (case, k, err)
    ok, err = close(got["entropy"], ref["entropy"])
    assert ok, (case, "entropy", err)
    # the same rollout as T successive act-path calls on the same policy (which reads the same flat buffer now)
    obs, hidden, prev, masks, actions = to_gpu(inp)
    vals, lps = [], []
    for t in range(T):
        s = slice(t * N, (t + 1) * N)
        _, hidden, logits, value = pol.features_and_logits({k: v[s] for k, v in obs.items()}, hidden, prev[s], masks[s])
        vals.append(value)
        lps.append(torch.log_softmax(logits, -1).gather(-1, actions[s]))
    assert np.array_equal(torch.cat(vals).cpu().numpy(), got["value"]), (case, "act path", "value")
    assert np.array_equal(hidden.cpu().numpy(), got["hidden"]), (case, "act path", "hidden")
    lp = torch.cat(lps).cpu().numpy().astype(np.float64)
    assert np.all(np.abs(lp - got["logp"]) <= ULP4 * np.maximum(1.0, np.abs(lp))), (case, "act path", "logp", np.abs(lp - got["logp"]).max())
    if not pol.net.is_blind:                                 # the embedding of all M rows at once against the rows one step at a time
        emb = pol.net.visual_encoder(obs)
        for t in range(T):
            s = slice(t * N, (t + 1) * N)
            assert torch.equal(emb[s], pol.net.visual_encoder({k: v[s] for k, v in obs.items()}))


def test_hidden_state_of_the_wrong_shape_is_refused():
    pol, step, _ = gpu_case("A")
    obs, hidden, prev, masks, actions = to_gpu(P.rollout("A"))
    with pytest.raises(ValueError, match="rnn_hidden_states"):
        step.evaluate_actions(obs, torch.cat([hidden, hidden]), prev, masks, actions)
    with pytest.raises(ValueError, match="rnn_hidden_states"):
        step.evaluate_actions(obs, hidden[:, :2], prev, masks, actions)      # 15 rows do not divide into 2 environments


# ------------------------------------------------------------------------------------------------------------------ 2. loss
@pytest.mark.parametrize("case", CASES)
def test_loss_matches_fp64(case):
    _, _, got = gpu_case(case)
    ref = P.reference(case)
    for k, g, w in zip(("value_loss", "action_loss", "dist_entropy"), got["losses"], ref["losses"]):
        print(f"[{case}] {k}: {g:.8f} vs {w:.8f}")
        assert loss_close(g, w), (case, k, g, w)


# ------------------------------------------------------------------------------------------------------------------ 3. gradients
@pytest.mark.parametrize("case", CASES)
def test_gradients_match_fp64_autograd(case):
    _, step, got = gpu_case(case)
    ref = P.reference(case)
    assert set(step.offsets) == set(ref["grads"])
    errs = grad_errors(step, got["grad"], ref["grads"], case)
    assert max(errs.values()) <= GRAD_TOL, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    assert len(errs) == len(step.offsets)                    # every tensor of these cases has a gradient
    # the alignment gaps between the tensors stay zero
    covered = np.zeros(got["grad"].size, bool)
    for off, n in step.offsets.values():
        covered[off:off + n] = True
    assert not got["grad"][~covered].any()


def test_float32_rgb_gives_the_bits_of_uint8_rgb():
    _, _, a = gpu_case("A")
    _, _, ap = gpu_case("Ap")
    assert np.array_equal(a["grad"], ap["grad"])
    for k in ("value", "logp", "hidden", "losses"):
        assert np.array_equal(a[k], ap[k]), k


def test_a_second_identical_update_is_bit_identical():
    for case in ("A", "F"):
        _, step, first = gpu_case(case)
        again = run_update(step, P.rollout(case), P.reference(case)["loss_inputs"])
        for k in ("grad", "value", "logp", "hidden", "losses"):
            assert np.array_equal(first[k], again[k]), (case, k)


def test_frozen_encoder_leaves_its_range_zero_and_the_rest_unchanged():
    _, full_step, full = gpu_case("A")
    pol = make_policy("A")
    for n, p in pol.named_parameters():
        p.requires_grad_(not n.startswith(P.ENC))
    agent = PPO(pol, P.CLIP, 1, 1, P.VALUE_COEF, P.ENTROPY_COEF, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    step = agent.train_step
    assert isinstance(step, BaselineTrainStep) and not step.train_encoder   # what PPO derives from requires_grad
    got = run_update(step, P.rollout("A"), P.reference("A")["loss_inputs"])
    lo, hi = step.encoder_range
    assert hi > lo and not got["grad"][lo:hi].any()
    rest = np.ones(got["grad"].size, bool)
    rest[lo:hi] = False
    assert step.offsets == full_step.offsets and np.array_equal(got["grad"][rest], full["grad"][rest])
    assert got["grad"][rest].any()
    before = step.flat.clone()
    step.clip_grad_norm()
    step.optimizer_step()
    torch.cuda.synchronize()
    assert torch.equal(before[lo:hi], step.flat[lo:hi]) and not torch.equal(before, step.flat)
    assert len(step.state_dict()["state"]) == sum(1 for n in step.offsets if not n.startswith(P.ENC))


# ------------------------------------------------------------------------------------------------------------------ 4. step
@pytest.mark.parametrize("case", ["A", "E"])
def test_step_matches_fp64_adam_and_act_reads_the_new_weights(case):
    pol = make_policy(case)
    step = BaselineTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    ref = P.reference(case)
    newp, norm, coef, _ = P.clip_and_adam(ref["params"], ref["grads"], lr=LR, eps=EPS, max_norm=MAX_GRAD_NORM)
    assert coef < 1.0                                      # the clipping is live
    sel = {k: np.abs(g) > 1e-6 * max(np.abs(g).max(), 1e-30) for k, g in ref["grads"].items()}
    assert sum(int(s.sum()) for s in sel.values()) >= 0.5 * sum(s.size for s in sel.values())
    run_update(step, P.rollout(case), ref["loss_inputs"])
    gnorm = step.clip_grad_norm()
    step.optimizer_step()
    torch.cuda.synchronize()
    assert abs(float(gnorm) - norm) < 1e-4 * norm
    worst = 0.0
    for name, (off, n) in step.offsets.items():
        got = step.flat[off:off + n].cpu().double().numpy()
        s = sel[name].reshape(-1)
        worst = max(worst, np.abs(got[s] - newp[name].reshape(-1)[s]).max(initial=0.0))
        np.testing.assert_allclose(got[s], newp[name].reshape(-1)[s], rtol=0, atol=STEP_ATOL, err_msg=name)
    print(f"[step {case}] worst parameter difference after clip + Adam: {worst:.2e}")
    # state_dict() returns the new weights (the parameters are views of the flat buffer)
    sd = {k: v.detach().cpu().numpy() for k, v in pol.state_dict().items()}
    for name, (off, n) in step.offsets.items():
        assert np.array_equal(sd[name].reshape(-1), step.flat[off:off + n].cpu().numpy())
        assert not np.array_equal(sd[name], np.asarray(P.state_dict(case)[name], np.float32)), name
    # act after the step: the float64 model on the weights the device holds now
    inp = P.rollout(case)
    N = inp["N"]
    s = slice(0, N)
    obs, hidden, prev, masks, _ = to_gpu(inp)
    feats, hout, logits, value = pol.features_and_logits({k: v[s] for k, v in obs.items()}, hidden, prev[s], masks[s])
    f = lambda a: None if a is None else a[s]
    want = BR.policy_step({k: v.astype(np.float64) for k, v in sd.items()}, f(inp["rgb"]), f(inp["depth"]), inp["goal"][s],
                          inp["masks"][s], inp["hidden"])
    old = BR.policy_step(P.state_dict(case), f(inp["rgb"]), f(inp["depth"]), inp["goal"][s], inp["masks"][s], inp["hidden"])
    for k, g in (("features", feats), ("hidden", hout), ("logits", logits), ("value", value)):
        ok, err = close(g.cpu().numpy(), want[k])
        assert ok, (case, "act after the step", k, err)
    assert np.abs(want["logits"] - old["logits"]).max() > 10 * TOL * np.abs(old["logits"]).max()    # the step is visible at TOL


# ------------------------------------------------------------------------------------------------------------------ 5. end to end
def fill_storage(pol, T=4, N=2):
    c = P.CASES["A"]
    H, W, Hd = c["H"], c["W"], c["hidden"]
    inp = P.rollout("A")
    cut = lambda a, *tail: torch.from_numpy(a.reshape(c["T"], c["N"], *tail)[:T + 1, :N].copy())
    rgb, depth = cut(inp["rgb"], H, W, 3).float().to(DEV), cut(inp["depth"], H, W, 1).to(DEV)
    goals, masks = cut(inp["goal"], 2).to(DEV), cut(inp["masks"], 1)
    st = RolloutStorage(T, N, space("A"), ActionSpace(P.N_ACTIONS), Hd, pol.net.num_recurrent_layers)
    st.to(DEV)
    st.observations["rgb"][0].copy_(rgb[0])
    st.observations["depth"][0].copy_(depth[0])
    st.observations[GOAL][0].copy_(goals[0])
    st.recurrent_hidden_states[0].copy_(torch.from_numpy(inp["hidden"][:, :N].copy()))
    st.masks[0].copy_(masks[0])
    for t in range(T):
        obs = {k: v[st.step] for k, v in st.observations.items()}
        value, action, logp, hidden = pol.act(obs, st.recurrent_hidden_states[st.step], st.prev_actions[st.step], st.masks[st.step],
                                              deterministic=True)
        rewards = torch.tensor([[0.25 * (t + 1)], [-0.5 + 0.125 * t]])
        st.insert({"rgb": rgb[t + 1], "depth": depth[t + 1], GOAL: goals[t + 1]}, hidden, action, logp, value, rewards, masks[t + 1])
    obs = {k: v[st.step] for k, v in st.observations.items()}
    next_value = pol.get_value(obs, st.recurrent_hidden_states[st.step], st.prev_actions[st.step], st.masks[st.step])
    st.compute_returns(next_value, True, 0.99, 0.95)
    torch.cuda.synchronize()
    return st


def test_ppo_update_over_a_rollout_storage_returns_the_reference_floats():
    """T = 4, N = 2, two epochs of two minibatches (one environment each): four optimiser steps.  The reference: the float64 model run
    over the same four minibatches (read from the storage's own generator under the same torch seed), each followed by
    clip_and_adam on the float64 gradients with the moments carried, the losses averaged as PPO.update averages them."""
    pol = make_policy("A")
    st = fill_storage(pol)
    agent = PPO(pol, P.CLIP, 2, 2, P.VALUE_COEF, P.ENTROPY_COEF, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM,
                use_clipped_value_loss=True, use_normalized_advantage=True)
    assert isinstance(agent.train_step, BaselineTrainStep)
    torch.manual_seed(11)
    adv = agent.get_advantages(st)
    samples = [mb for _ in range(2) for mb in st.recurrent_generator(adv, 2)]
    n = lambda t: t.detach().cpu().numpy()
    params = {k: np.asarray(v, np.float64) for k, v in P.state_dict("A").items()}
    state, sums = None, np.zeros(3)
    for k, (obs, hid, act, prev, vp, ret, mask, old, adv_t) in enumerate(samples):
        M = act.shape[0]
        assert M == 4 and tuple(hid.shape) == (1, 1, P.CASES["A"]["hidden"])
        inp = dict(rgb=n(obs["rgb"]), depth=n(obs["depth"]), goal=n(obs[GOAL]), masks=n(mask).reshape(M), actions=n(act).reshape(M),
                   hidden=n(hid), T=M, N=1)
        li = dict(old=n(old).reshape(M), adv=n(adv_t).reshape(M), vp=n(vp).reshape(M), ret=n(ret).reshape(M))
        r = P.update(params, inp, li)
        sums += np.array(r["losses"])
        params, _, _, state = P.clip_and_adam(params, r["grads"], lr=LR, eps=EPS, max_norm=MAX_GRAD_NORM, state=state, step=k + 1)
    want = sums / 4
    torch.manual_seed(11)
    got = agent.update(st)
    torch.cuda.synchronize()
    print(f"[end to end] losses {got} vs float64 {want.tolist()}")
    assert len(got) == 3 and all(isinstance(x, float) for x in got)
    for g, w in zip(got, want):
        assert loss_close(g, w), (got, want)
    assert agent.train_step.step_count == 4
    for name, (off, k) in agent.train_step.offsets.items():   # four steps later the weights still follow the float64 model
        ok, err = close(agent.train_step.flat[off:off + k].cpu().numpy(), params[name].reshape(-1))
        assert ok, (name, err)


def test_policy_and_optimizer_state_loaded_after_attach_resume_bit_equal():
    ref = P.reference("B")
    a = make_policy("B")
    sa = BaselineTrainStep(a, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    run_update(sa, P.rollout("B"), ref["loss_inputs"])
    sa.clip_grad_norm()
    sa.optimizer_step()
    # a fresh process would build the policy, attach, then load the checkpoint
    b = PointNavBaselinePolicy(space("B"), Act(P.N_ACTIONS), GOAL, P.CASES["B"]["hidden"]).to(DEV).eval()
    sb = BaselineTrainStep(b, lr=1.0, eps=1.0, max_grad_norm=MAX_GRAD_NORM)
    b.load_state_dict({k: v.clone() for k, v in a.state_dict().items()})
    sb.load_state_dict(sa.state_dict())
    assert (sb.lr, sb.eps, sb.step_count) == (sa.lr, sa.eps, 1)
    outs = []
    for s in (sa, sb):
        r = run_update(s, P.rollout("B"), ref["loss_inputs"])
        s.clip_grad_norm()
        s.optimizer_step()
        torch.cuda.synchronize()
        outs.append((r, s.flat.cpu().numpy(), s.exp_avg.cpu().numpy(), s.exp_avg_sq.cpu().numpy()))
    (ra, fa, ma, va), (rb, fb, mb, vb) = outs
    assert np.array_equal(ra["grad"], rb["grad"]) and np.array_equal(ra["value"], rb["value"])
    assert np.array_equal(fa, fb) and np.array_equal(ma, mb) and np.array_equal(va, vb)
    obs, hidden, prev, masks, _ = to_gpu(P.rollout("B"))
    s0 = slice(0, 1)                                         # (N = 1: one row per step)
    fa_ = a.features_and_logits({k: v[s0] for k, v in obs.items()}, hidden, prev[s0], masks[s0])
    fb_ = b.features_and_logits({k: v[s0] for k, v in obs.items()}, hidden, prev[s0], masks[s0])
    assert all(torch.equal(x, y) for x, y in zip(fa_, fb_))


# ------------------------------------------------------------------------------------------------------------------ 6. refusals
def test_unattached_policy_still_raises_and_ddppo_refuses():
    pol = make_policy("E")
    obs, hidden, prev, masks, actions = to_gpu(P.rollout("E"))
    with pytest.raises(NotImplementedError, match="PPO update"):
        pol.evaluate_actions(obs, hidden, prev, masks, actions)
    with pytest.raises(NotImplementedError, match="PointNavBaselinePolicy"):
        DDPPO(pol, P.CLIP, 1, 1, P.VALUE_COEF, P.ENTROPY_COEF, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    assert pol._train_step is None                           # nothing was attached on the way to the refusal
    step = BaselineTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    value, logp, entropy, hout = pol.evaluate_actions(obs, hidden, prev, masks, actions)      # delegates now
    assert value.shape == (6, 1) and step.encoder_range is None


def test_library_refuses_calls_out_of_order():
    import ctypes as C

    from pointnav_vo_amd import _lib
    pol = make_policy("E")
    pol._ensure(DEV)
    h = pol._handle
    assert _lib.lib.pnvo_baseline_backward(h, 1, None) == -3 and b"pnvo_baseline_train_attach first" in _lib.lib.pnvo_last_error(None)
    step = BaselineTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    assert _lib.lib.pnvo_baseline_backward(h, 1, None) == -3 and b"before pnvo_baseline_evaluate" in _lib.lib.pnvo_last_error(None)
    blob = np.zeros(4, np.float32)
    assert _lib.lib.pnvo_baseline_load_weights(h, blob.ctypes.data_as(C.c_void_p), 4, step.store.toc, 0) == -3
    assert b"after pnvo_baseline_train_attach" in _lib.lib.pnvo_last_error(None)
