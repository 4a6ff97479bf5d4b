"""GPU (-m gpu): one PPO minibatch update of the HIP navigation policy (pointnav_vo_amd.ppo on pnvo_policy_evaluate / _ppo_loss /
_backward / _clip_grad_norm / pnvo_adam_step) against a torch-CPU float64 model of the whole policy (tests/ppo_reference.py:
oracle.torch_train_ref's encoder, torch.nn.LSTM stepped with the masks applied, Linear heads, the reference agent's loss, autograd).

Cases (ppo_reference.CASES; the smallest shapes that reach every branch):
  A   96x128, hidden 128, 2 layers, 4 actions, T = 5, N = 3: a start reset, a mid-sequence reset of one environment, two at once,
      carried state, a non-zero initial state; M = 15 frames (above the 8-frame persistent encoder of the act path)
  B   96x128, hidden 256, 1 layer, 3 actions, T = 4, N = 1: no reset anywhere, one environment, one layer (an embedding row no sample
      gathers: its gradient must be exactly zero); B1: the same policy in the M == N single-step form, N = 4
  C   192x341, hidden 512, 2 layers, 4 actions, T = 3, N = 2: the default sizes, odd width through the average pool; M = 6

Tolerances.  Forward: 2e-4 of each tensor's scale (close() of tests/test_gpu_policy.py).  Loss: 1e-4 * max(1, |x|) (the bound of
tests/test_gpu_train.py).  Gradients, relative L2 per parameter tensor: the float64 model run in float32 on the CPU deviates from its
float64 self by at most 9.96e-06 over the cases (tools/ppo_grad_error_table.py: worst tensors are GroupNorm weights of layer1, median
4-6e-06); GRAD_TOL = 10 x that = 1.0e-4, the margin GRAD_TOL of tests/test_gpu_train.py was given.
  The HIP path's measured worst tensor (MI355X): see MEASURED below.
Step: the reference's shipped optimiser settings (lr 2.5e-4, eps 1e-5, max_grad_norm 0.2); on them the float32 CPU model is within
1.9e-07 of the float64 parameters after the step, so atol 2e-6 (the existing train test's) holds for a float32 framework.
"""
import functools

import numpy as np
import pytest
import torch

import ppo_reference as R
from pointnav_vo_amd import synth
from pointnav_vo_amd.policy import PointNavResNetPolicy
from pointnav_vo_amd.ppo import PPO, PolicyTrainStep

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TOL = 2e-4
GRAD_TOL = 1.0e-4
# MEASURED (MI355X, this file's own printout): worst per-tensor relative L2 of the HIP gradients against float64 autograd —
#   A 3.65e-06, B 2.58e-06, B1 3.06e-06, C 3.87e-06 (A with the plain value loss 3.46e-06, A with a frozen encoder 2.08e-06);
#   losses within 7e-08, parameters after clip + Adam within 9.3e-08.
LR, EPS, MAX_GRAD_NORM = 2.5e-4, 1e-5, 0.2               # configs/rl/ddppo_pointnav.yaml
GOAL = R.GOAL


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class Act:
    def __init__(self, n):
        self.n = n


def make_policy(case, device=DEV):
    c = R.CASES[case]
    space = Space({"depth": Box((c["H"], c["W"], 1)), "rgb": Box((c["H"], c["W"], 3)), GOAL: Box((2,))})
    pol = PointNavResNetPolicy(observation_space=space, action_space=Act(c["A"]), hidden_size=c["hidden"], rnn_type="LSTM",
                               num_recurrent_layers=c["L"], backbone="resnet18", goal_sensor_uuid=GOAL,
                               normalize_visual_inputs=False, obs_transform=None, vis_types=["depth"])
    sd = R.state_dict(case)
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


def to_gpu(inp):
    M = inp["T"] * inp["N"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    obs = {"depth": t(inp["depth"]), GOAL: t(inp["goal"])}
    return obs, t(inp["hidden"]), t(inp["prev"]).view(M, 1), t(inp["masks"]).view(M, 1), t(inp["actions"]).view(M, 1)


def run_update(step, inp, li, use_clipped=True):
    """evaluate_actions + ppo_loss + backward on the GPU -> numpy results (the gradient buffer is copied out)."""
    obs, hidden, prev, masks, actions = to_gpu(inp)
    value, logp, entropy, hout = step.evaluate_actions(obs, hidden, prev, masks, actions)
    t = lambda k: torch.from_numpy(li[k]).to(DEV)
    out3 = step.ppo_loss(t("old"), t("adv"), t("vp"), t("ret"), R.CLIP, R.VALUE_COEF, R.ENTROPY_COEF, use_clipped)
    step.backward()
    torch.cuda.synchronize()
    return dict(value=value.cpu().numpy(), logp=logp.cpu().numpy(), entropy=float(entropy), hidden=hout.cpu().numpy(),
                losses=out3.cpu().numpy().astype(np.float64), grad=step.grad.cpu().double().numpy(), shapes=(value.shape, logp.shape))


@functools.lru_cache(maxsize=None)
def gpu_case(case):
    """The policy of a case with a train step attached and one update's results, shared by the forward / loss / gradient tests."""
    pol = make_policy("B" if case == "B1" else case)
    step = PolicyTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    ref = R.reference(case)
    return pol, step, run_update(step, R.rollout(case), ref["loss_inputs"])


def grad_errors(step, grad, ref_grads, what):
    """Per-tensor relative L2 against float64 autograd (denominator floor 1e-12); a zero reference gradient must be exactly zero."""
    errs = {}
    for name, (off, n) in step.offsets.items():
        g, gr = grad[off:off + n], ref_grads[name].reshape(-1)
        if not gr.any():
            assert not g.any(), (what, name, "reference gradient is exactly zero, the HIP gradient is not")
            continue
        errs[name] = np.linalg.norm(g - gr) / max(np.linalg.norm(gr), 1e-12)
    worst = max(errs, key=errs.get)
    print(f"[{what}] worst gradient tensor {errs[worst]:.2e} ({worst}), median {np.median(list(errs.values())):.2e}, GRAD_TOL {GRAD_TOL:.1e}")
    return errs


# ------------------------------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("case", ["A", "B", "B1", "C"])
def test_forward_matches_fp64_and_the_act_path(case):
    pol, step, got = gpu_case(case)
    ref, inp = R.reference(case), R.rollout(case)
    T, N, M = inp["T"], inp["N"], inp["T"] * inp["N"]
    assert got["shapes"] == ((M, 1), (M, 1))
    for k in ("value", "logp", "hidden"):
        ok, err = close(got[k], ref[k])
        print(f"[{case}] {k}: {err:.2e} of scale")
        assert ok, (case, k, err)
    ok, err = close(got["entropy"], ref["entropy"])
    assert ok, (case, "entropy", err)
    # the same rollout as T successive calls of the act path (which reads the same flat buffer now)
    obs, hidden, prev, masks, actions = to_gpu(inp)
    vals, lps = [], []
    for t in range(T):
        s = slice(t * N, (t + 1) * N)
        _, hidden, logits, value = pol.features_and_logits({k: v[s] for k, v in obs.items()}, hidden, prev[s], masks[s])
        vals.append(value)
        lps.append(torch.log_softmax(logits, -1).gather(-1, actions[s]))
    for k, seq in (("value", vals), ("logp", lps)):
        ok, err = close(torch.cat(seq).cpu().numpy(), got[k])
        assert ok, (case, "act path", k, err)
    ok, err = close(hidden.cpu().numpy(), got["hidden"])
    assert ok, (case, "act path", "hidden", err)
    # two identical calls are bit-equal
    a = step.evaluate_actions(*to_gpu(inp))
    b = step.evaluate_actions(*to_gpu(inp))
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(a[0].cpu().numpy(), got["value"]) and np.array_equal(a[3].cpu().numpy(), got["hidden"])


# ------------------------------------------------------------------------------------------------------------------ 2. loss
def assert_every_branch_is_live(case):
    """From the float64 side alone.  Case A (M = 15): each of {surrogate clipped, unclipped} x {value clipped, unclipped} holds at
    least two elements.  Cases B, B1, C have M = 4 / 6 elements, fewer than the eight the four cells need: there each branch of
    each clamp holds at least two.  No element lies within 1e-6 of a branch boundary."""
    ref = R.reference(case)
    s, v, margin = R.branch_census(ref["value"], ref["logp"], ref["loss_inputs"])
    assert margin.min() > 1e-6, (case, margin.min())
    adv = ref["loss_inputs"]["adv"]
    assert (adv > 0).any() and (adv < 0).any()
    if case == "A":
        cells = {(a, b): int(((s == a) & (v == b)).sum()) for a in (True, False) for b in (True, False)}
        assert min(cells.values()) >= 2, cells
    else:
        assert min(int(s.sum()), int((~s).sum()), int(v.sum()), int((~v).sum())) >= 2, (case, s, v)


@pytest.mark.parametrize("case", ["A", "B", "B1", "C"])
def test_loss_matches_fp64(case):
    assert_every_branch_is_live(case)
    _, _, got = gpu_case(case)
    ref = R.reference(case)
    for k, g, w in zip(("value_loss", "action_loss", "dist_entropy"), got["losses"], ref["losses"]):
        print(f"[{case}] {k}: {g:.8f} vs {w:.8f}")
        assert loss_close(g, w), (case, k, g, w)


def test_plain_value_loss_matches_fp64():
    """use_clipped_value_loss = False: loss and gradients."""
    assert_every_branch_is_live("A")
    pol, step, _ = gpu_case("A")
    ref = R.reference("A", "float64", False)
    got = run_update(step, R.rollout("A"), ref["loss_inputs"], use_clipped=False)
    for g, w in zip(got["losses"], ref["losses"]):
        assert loss_close(g, w), (got["losses"], ref["losses"])
    errs = grad_errors(step, got["grad"], ref["grads"], "A, plain value loss")
    assert max(errs.values()) <= GRAD_TOL, sorted(errs.items(), key=lambda kv: -kv[1])[:5]


# ------------------------------------------------------------------------------------------------------------------ 3. gradients
@pytest.mark.parametrize("case", ["A", "B", "B1", "C"])
def test_gradients_match_fp64_autograd(case):
    _, step, got = gpu_case(case)
    ref = R.reference(case)
    errs = grad_errors(step, got["grad"], ref["grads"], case)
    assert max(errs.values()) <= GRAD_TOL, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    if case in ("B", "B1"):      # embedding rows no sample gathered: exactly zero
        inp = R.rollout(case)
        used = set((((inp["prev"].astype(np.float32) + 1.0) * inp["masks"]).astype(np.int64)).tolist())
        off, n = step.offsets["net.prev_action_embedding.weight"]
        emb = got["grad"][off:off + n].reshape(-1, 32)
        unused = [r for r in range(emb.shape[0]) if r not in used]
        assert unused and not emb[unused].any()
        assert all(emb[r].any() for r in used)


def test_frozen_encoder_leaves_its_range_zero():
    pol = make_policy("A")
    step = PolicyTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM, train_encoder=False)
    ref = R.reference("A")
    got = run_update(step, R.rollout("A"), ref["loss_inputs"])
    lo, hi = step.encoder_range
    assert hi > lo and not got["grad"][lo:hi].any()
    assert not got["grad"][step.n_params:].any()
    want = {k: (np.zeros_like(g) if k.startswith(R.ENC) else g) for k, g in ref["grads"].items()}
    errs = grad_errors(step, got["grad"], want, "A, frozen encoder")
    assert "net.visual_fc.1.weight" in errs and max(errs.values()) <= GRAD_TOL, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    # the optimiser leaves the frozen range alone
    before = step.flat.clone()
    step.clip_grad_norm()
    step.optimizer_step()
    torch.cuda.synchronize()
    assert torch.equal(before[lo:hi], step.flat[lo:hi]) and not torch.equal(before, step.flat)


# ------------------------------------------------------------------------------------------------------------------ 4. step
def test_step_matches_fp64_adam_and_act_reads_the_new_weights():
    case = "A"
    pol = make_policy(case)
    step = PolicyTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    ref = R.reference(case)
    newp, norm, coef, _ = R.clip_and_adam(ref["params"], ref["grads"], lr=LR, eps=EPS, max_norm=MAX_GRAD_NORM)
    assert coef < 1.0                                      # the clipping is live
    sel = {k: np.abs(g) > 1e-6 * max(np.abs(g).max(), 1e-30) for k, g in ref["grads"].items()}
    assert sum(int(s.sum()) for s in sel.values()) >= 0.5 * sum(s.size for s in sel.values())
    # a fresh frame for the act path, before and after the step
    fresh = R.rollout("A", 77)
    one = dict(fresh, depth=fresh["depth"][:3], goal=fresh["goal"][:3], prev=fresh["prev"][:3], masks=np.ones(3, np.float32),
               actions=fresh["actions"][:3], T=1, N=3)
    obs, hidden, prev, masks, _ = to_gpu(one)
    v0, a0, lp0, h0 = pol.act(obs, hidden, prev, masks, deterministic=True)
    run_update(step, R.rollout(case), ref["loss_inputs"])
    gnorm = step.clip_grad_norm()
    step.optimizer_step()
    torch.cuda.synchronize()
    assert abs(float(gnorm) - norm) < 1e-4 * norm
    worst = 0.0
    for name, (off, n) in step.offsets.items():
        got = step.flat[off:off + n].cpu().double().numpy()
        s = sel[name].reshape(-1)
        worst = max(worst, np.abs(got[s] - newp[name].reshape(-1)[s]).max(initial=0.0))
        np.testing.assert_allclose(got[s], newp[name].reshape(-1)[s], rtol=0, atol=2e-6, err_msg=name)
    print(f"[step] worst parameter difference after clip + Adam: {worst:.2e}")
    v1, a1, lp1, h1 = pol.act(obs, hidden, prev, masks, deterministic=True)
    torch.cuda.synchronize()
    wv, _, _, wh, wl = R.evaluate(newp, one)
    for k, g, w in (("value", v1, wv), ("hidden", h1, wh)):
        ok, err = close(g.cpu().numpy(), w)
        assert ok, ("act after the step", k, err)
    wlp = torch.log_softmax(torch.from_numpy(wl), -1).numpy()
    np.testing.assert_allclose(lp1.cpu().numpy()[:, 0], wlp[np.arange(3), a1.cpu().numpy()[:, 0]], rtol=0, atol=2e-4)
    assert not torch.equal(v0, v1) and not torch.equal(h0, h1)      # the act path reads the new weights


# ------------------------------------------------------------------------------------------------------------------ 5. PPO.update
class Rollouts:
    """The part of RolloutStorage PPO.update reads: returns, value_preds and a recurrent_generator over fixed minibatches."""

    def __init__(self, minibatches):
        self.mbs = minibatches                            # [(inputs, loss inputs)], each T x N
        T, N = minibatches[0][0]["T"], minibatches[0][0]["N"]
        self.T, self.N = T, N
        f = lambda k: torch.cat([torch.from_numpy(li[k]).view(T, N, 1) for _, li in minibatches], dim=1)
        pad = torch.zeros(1, N * len(minibatches), 1)
        self.value_preds = torch.cat([f("vp"), pad]).to(DEV)
        self.returns = torch.cat([f("ret"), pad]).to(DEV)

    def recurrent_generator(self, advantages, num_mini_batch):
        assert num_mini_batch == len(self.mbs)
        T, N, M = self.T, self.N, self.T * self.N
        for i, (inp, li) in enumerate(self.mbs):
            envs = slice(i * N, (i + 1) * N)
            obs, hidden, prev, masks, actions = to_gpu(inp)
            yield (obs, hidden, actions, prev, self.value_preds[:T, envs].reshape(M, 1), self.returns[:T, envs].reshape(M, 1), masks,
                   torch.from_numpy(li["old"]).view(M, 1).to(DEV), advantages[:T, envs].reshape(M, 1))


def test_ppo_update_matches_fp64_and_reduces_the_loss():
    case = "A"
    sd = R.state_dict(case)
    mbs = []
    for iseed in (None, 41):
        inp = R.rollout(case, iseed)
        v, lp = R.evaluate(sd, inp)[:2]
        mbs.append((inp, R.loss_inputs(case, v, lp, iseed=iseed)))
    # float64: minibatch 1 on the initial parameters, clip + Adam, minibatch 2 on the stepped parameters
    P, state, want = {k: np.asarray(v, np.float64) for k, v in sd.items()}, None, []
    for k, (inp, li) in enumerate(mbs):
        li64 = dict(li, adv=(li["ret"].astype(np.float64) - li["vp"].astype(np.float64)))     # get_advantages: returns - value_preds
        r = R.update(P, inp, li64)
        want.append(r["losses"])
        P, _, _, state = R.clip_and_adam(P, r["grads"], lr=LR, eps=EPS, max_norm=MAX_GRAD_NORM, state=state, step=k + 1)
    want = np.mean(want, axis=0)
    pol = make_policy(case)
    agent = PPO(pol, R.CLIP, 1, 2, R.VALUE_COEF, R.ENTROPY_COEF, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM,
                use_clipped_value_loss=True, use_normalized_advantage=False)
    rollouts = Rollouts(mbs)
    first = agent.update(rollouts)
    assert len(first) == 3 and all(isinstance(x, float) and np.isfinite(x) for x in first)
    for k, g, w in zip(("value_loss", "action_loss", "dist_entropy"), first, want):
        print(f"[update] {k}: {g:.8f} vs {w:.8f}")
        assert loss_close(g, w), (k, g, w)
    second = agent.update(rollouts)
    total = lambda x: x[0] * R.VALUE_COEF + x[1] - x[2] * R.ENTROPY_COEF
    assert np.isfinite(second).all() and total(second) < total(first), (first, second)
    assert agent.train_step.step_count == 4


# ------------------------------------------------------------------------------------------------------------------ 6. resume
def small_minibatch(iseed):
    """T = 3, N = 2 on case A's policy: the first three steps of the first two environments of its rollout (resets at t = 0 and t = 2,
    a non-zero initial state), with loss inputs of both signs."""
    inp = R.rollout("A", iseed)
    T, N, M = 3, 2, 6
    rows = np.array([t * inp["N"] + n for t in range(T) for n in range(N)])
    mb = dict({k: np.ascontiguousarray(inp[k][rows]) for k in ("depth", "goal", "prev", "masks", "actions")},
              hidden=np.ascontiguousarray(inp["hidden"][:, :N]), T=T, N=N)
    seed = 1000 * (iseed or 0) + 7
    u = lambda tag, lo, hi: synth.uniform(seed, tag, (M,), lo, hi).astype(np.float32)
    vp, adv = u("vp", -0.5, 0.5), u("adv", -1.0, 1.0)
    return mb, dict(old=u("old", -1.8, -1.0), vp=vp, adv=adv, ret=vp + adv)


def test_policy_and_optimizer_loaded_after_attach_resume_bit_equal():
    """What test_parameters_loaded_after_attach_are_used_by_the_next_training_forward (test_gpu_fullsize.py) checks for VOTrainStep, for
    the policy: policy.load_state_dict() and train_step.load_state_dict() AFTER a fresh PolicyTrainStep was attached must reach the
    kernels (flat buffer, the encoder's packed operands, Adam's moments and step count).  Every reduction of the update has a fixed
    order, so the resumed run is bit-equal to the one that never stopped."""
    def update(step, mb):
        run_update(step, *mb)
        step.clip_grad_norm()
        step.optimizer_step()

    first, second = small_minibatch(None), small_minibatch(41)
    pol_a = make_policy("A")
    step_a = PolicyTrainStep(pol_a, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    update(step_a, first)
    ckpt_policy = {k: v.detach().cpu().clone() for k, v in pol_a.state_dict().items()}
    ckpt_optim = step_a.state_dict()
    pol_b = make_policy("A")                                      # the initial weights again
    step_b = PolicyTrainStep(pol_b, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    assert not torch.equal(step_b.flat, step_a.flat)
    pol_b.load_state_dict(ckpt_policy)                            # lands in the flat buffer, AFTER the attach
    step_b.load_state_dict(ckpt_optim)
    update(step_a, second)
    update(step_b, second)
    torch.cuda.synchronize()
    assert step_a.step_count == step_b.step_count == 2
    n = step_a.n_params
    assert torch.equal(step_b.flat[:n], step_a.flat[:n])
    assert torch.equal(step_b.exp_avg, step_a.exp_avg) and torch.equal(step_b.exp_avg_sq, step_a.exp_avg_sq)
    assert step_a.exp_avg.any() and step_a.exp_avg_sq.any()
    one = dict(second[0], **{k: second[0][k][:2] for k in ("depth", "goal", "prev", "masks", "actions")}, T=1)
    obs, hidden, prev, masks, _ = to_gpu(one)
    la = pol_a.features_and_logits(obs, hidden, prev, masks)[2]
    lb = pol_b.features_and_logits(obs, hidden, prev, masks)[2]
    torch.cuda.synchronize()
    assert torch.isfinite(la).all() and torch.equal(la, lb)


# ------------------------------------------------------------------------------------------------------------------ 7. unattached
def test_unattached_policy_still_refuses_evaluate_actions():
    pol = make_policy("A")
    obs, hidden, prev, masks, actions = to_gpu(R.rollout("A"))
    with pytest.raises(NotImplementedError):
        pol.evaluate_actions(obs, hidden, prev, masks, actions)
