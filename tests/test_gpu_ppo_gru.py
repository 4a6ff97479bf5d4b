"""GPU (-m gpu): one PPO minibatch update of the GRU navigation policy (pointnav_vo_amd.ppo on pnvo_policy_evaluate / _ppo_loss /
_backward with rnn_type = GRU: gru_step_kernel, gru_bptt_step_kernel) against the torch-CPU float64 model of tests/gru_reference.py
(torch.nn.GRU stepped with the mask applied to h, autograd), which tests/test_policy_gru_host.py pins to the reference policy.

Cases: the GRU twins of ppo_reference.CASES (same frames, masks, weights' seeds; the state is [L, N, hidden]) —
  A   96x128, hidden 128, 2 layers, 4 actions, T = 5, N = 3: a start reset, a mid-sequence reset of one environment, two at once,
      carried state, a non-zero initial state
  B   96x128, hidden 256, 1 layer, 3 actions, T = 4, N = 1 (an embedding row no sample gathers); B1: the same policy, T = 1, N = 4
  C   192x341, hidden 512, 2 layers, 4 actions, T = 3, N = 2: the default sizes

Tolerances.  Forward: 2e-4 of each tensor's scale.  Loss: 1e-4 * max(1, |x|).  Gradients, relative L2 per parameter tensor: the float64
model run in float32 on the CPU (python tests/gru_reference.py) deviates from its float64 self by at most 1.857e-05 over the cases
(worst tensor: the stem GroupNorm weight of case C; A 5.64e-06, B 6.80e-06, B1 1.05e-05; medians 3-7e-06); GRAD_TOL = 10 x that =
1.85e-4, the rule that gave GRAD_TOL of tests/test_gpu_ppo.py and tests/test_gpu_train.py: what a float32 framework itself loses.
  The HIP path's measured worst tensor (MI355X): not measured yet, see MEASURED below.
Step: the reference's shipped optimiser settings (lr 2.5e-4, eps 1e-5, max_grad_norm 0.2); on them the float32 CPU model's gradients
put the parameters within 2.2e-07 of the float64 ones after clip + Adam, so the LSTM test's atol 2e-6 (10 x) holds for a float32
framework here too.
"""
import functools

import numpy as np
import pytest
import torch

import gru_reference as G
from pointnav_vo_amd.policy import PointNavResNetPolicy
from pointnav_vo_amd.ppo import PPO, PolicyTrainStep
from pointnav_vo_amd.rollout_storage import RolloutStorage

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TOL = 2e-4
GRAD_TOL = 1.85e-4
# MEASURED (MI355X): not measured yet — no GPU run could be made when this file was written.  The tests print the worst per-tensor
#   relative L2 of the HIP gradients, the three losses and the worst parameter difference after clip + Adam; put them here.
LR, EPS, MAX_GRAD_NORM = 2.5e-4, 1e-5, 0.2               # configs/rl/ddppo_pointnav.yaml
GOAL = G.GOAL
RNN = G.RNN


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


def make_policy(case, device=DEV):
    c = G.CASES[case]
    space = Space({"depth": Box((c["H"], c["W"], 1)), "rgb": Box((c["H"], c["W"], 3)), GOAL: Box((2,))})
    pol = PointNavResNetPolicy(observation_space=space, action_space=Act(c["A"]), hidden_size=c["hidden"], rnn_type="GRU",
                               num_recurrent_layers=c["L"], backbone="resnet18", goal_sensor_uuid=GOAL,
                               normalize_visual_inputs=False, obs_transform=None, vis_types=["depth"])
    sd = G.state_dict(case)
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
    out3 = step.ppo_loss(t("old"), t("adv"), t("vp"), t("ret"), G.CLIP, G.VALUE_COEF, G.ENTROPY_COEF, use_clipped)
    step.backward()
    torch.cuda.synchronize()
    return dict(value=value.cpu().numpy(), logp=logp.cpu().numpy(), entropy=float(entropy), hidden=hout.cpu().numpy(),
                losses=out3.cpu().numpy().astype(np.float64), grad=step.grad.cpu().double().numpy(), shapes=(value.shape, logp.shape))


@functools.lru_cache(maxsize=None)
def gpu_case(case):
    """The policy of a case with a train step attached and one update's results, shared by the forward / loss / gradient tests."""
    pol = make_policy("B" if case == "B1" else case)
    step = PolicyTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    ref = G.reference(case)
    return pol, step, run_update(step, G.gru_rollout(case), ref["loss_inputs"])


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
    print(f"[{what}] worst gradient tensor {errs[worst]:.2e} ({worst}), median {np.median(list(errs.values())):.2e}, GRAD_TOL {GRAD_TOL:.2e}")
    return errs


# ------------------------------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("case", ["A", "B", "B1", "C"])
def test_forward_matches_fp64_and_the_act_path(case):
    pol, step, got = gpu_case(case)
    ref, inp = G.reference(case), G.gru_rollout(case)
    T, N, M, L = inp["T"], inp["N"], inp["T"] * inp["N"], G.CASES[case]["L"]
    assert got["shapes"] == ((M, 1), (M, 1)) and got["hidden"].shape == (L, N, G.CASES[case]["hidden"])
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


def test_lstm_shaped_state_is_refused():
    pol, step, _ = gpu_case("A")
    obs, hidden, prev, masks, actions = to_gpu(G.gru_rollout("A"))
    with pytest.raises(ValueError, match="rnn_hidden_states"):
        step.evaluate_actions(obs, torch.cat([hidden, hidden]), prev, masks, actions)


# ------------------------------------------------------------------------------------------------------------------ 2. loss
def assert_every_branch_is_live(case):
    """The census of tests/test_gpu_ppo.py, from the float64 side alone.  Case A (M = 15): each of {surrogate clipped, unclipped} x
    {value clipped, unclipped} holds at least two elements.  Cases B, B1, C (M = 4 / 6): each branch of each clamp holds at least
    two.  No element lies within 1e-6 of a branch boundary."""
    ref = G.reference(case)
    s, v, margin = G.branch_census(ref["value"], ref["logp"], ref["loss_inputs"])
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
    ref = G.reference(case)
    for k, g, w in zip(("value_loss", "action_loss", "dist_entropy"), got["losses"], ref["losses"]):
        print(f"[{case}] {k}: {g:.8f} vs {w:.8f}")
        assert loss_close(g, w), (case, k, g, w)


# ------------------------------------------------------------------------------------------------------------------ 3. gradients
@pytest.mark.parametrize("case", ["A", "B", "B1", "C"])
def test_gradients_match_fp64_autograd(case):
    _, step, got = gpu_case(case)
    ref = G.reference(case)
    errs = grad_errors(step, got["grad"], ref["grads"], case)
    assert max(errs.values()) <= GRAD_TOL, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    # bias_hh and bias_ih are separate tensors with separate gradients: equal in the r and z blocks, and in the n block
    # d bias_hh = sum(dn_pre * r) while d bias_ih = sum(dn_pre)
    Hd = G.CASES[case]["hidden"]
    for l in range(G.CASES[case]["L"]):
        ih, hh = f"{RNN}bias_ih_l{l}", f"{RNN}bias_hh_l{l}"
        assert ih in errs and hh in errs
        rih, rhh = ref["grads"][ih], ref["grads"][hh]
        assert np.allclose(rih[:2 * Hd], rhh[:2 * Hd], rtol=1e-10, atol=1e-14 * np.abs(rih).max())
        assert np.linalg.norm(rih[2 * Hd:] - rhh[2 * Hd:]) > 0.1 * np.linalg.norm(rih[2 * Hd:])
        (oi, n), (oh, _) = step.offsets[ih], step.offsets[hh]
        gi, gh = got["grad"][oi:oi + n], got["grad"][oh:oh + n]
        assert np.array_equal(gi[:2 * Hd], gh[:2 * Hd]) and not np.array_equal(gi[2 * Hd:], gh[2 * Hd:])
    if case in ("B", "B1"):      # embedding rows no sample gathered: exactly zero
        inp = G.gru_rollout(case)
        used = set((((inp["prev"].astype(np.float32) + 1.0) * inp["masks"]).astype(np.int64)).tolist())
        off, n = step.offsets["net.prev_action_embedding.weight"]
        emb = got["grad"][off:off + n].reshape(-1, 32)
        unused = [r for r in range(emb.shape[0]) if r not in used]
        assert unused and not emb[unused].any()
        assert all(emb[r].any() for r in used)


def test_frozen_encoder_leaves_its_range_zero():
    pol = make_policy("A")
    step = PolicyTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM, train_encoder=False)
    ref = G.reference("A")
    got = run_update(step, G.gru_rollout("A"), ref["loss_inputs"])
    lo, hi = step.encoder_range
    assert hi > lo and not got["grad"][lo:hi].any()
    assert not got["grad"][step.n_params:].any()
    want = {k: (np.zeros_like(g) if k.startswith(G.ENC) else g) for k, g in ref["grads"].items()}
    errs = grad_errors(step, got["grad"], want, "A, frozen encoder")
    assert "net.visual_fc.1.weight" in errs and max(errs.values()) <= GRAD_TOL, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    before = step.flat.clone()
    step.clip_grad_norm()
    step.optimizer_step()
    torch.cuda.synchronize()
    assert torch.equal(before[lo:hi], step.flat[lo:hi]) and not torch.equal(before, step.flat)


# ------------------------------------------------------------------------------------------------------------------ 4. step
def test_step_matches_fp64_adam():
    case = "A"
    pol = make_policy(case)
    step = PolicyTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    ref = G.reference(case)
    newp, norm, coef, _ = G.clip_and_adam(ref["params"], ref["grads"], lr=LR, eps=EPS, max_norm=MAX_GRAD_NORM)
    assert coef < 1.0                                      # the clipping is live
    sel = {k: np.abs(g) > 1e-6 * max(np.abs(g).max(), 1e-30) for k, g in ref["grads"].items()}
    assert sum(int(s.sum()) for s in sel.values()) >= 0.5 * sum(s.size for s in sel.values())
    run_update(step, G.gru_rollout(case), ref["loss_inputs"])
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


# ------------------------------------------------------------------------------------------------------------------ 5. end to end
def test_rollout_storage_filled_by_act_feeds_ppo_update():
    """RolloutStorage needs nothing for a GRU: built with policy.net.num_recurrent_layers (= L) it is filled by act() for T = 4, N = 2,
    compute_returns, then PPO.update with one epoch and one minibatch.  The update's losses are those of the piecewise path
    (evaluate_actions + ppo_loss on a twin policy) on the same minibatch, bit for bit: every reduction has a fixed order."""
    c = G.CASES["A"]
    T, N, L, Hd, H, W = 4, 2, c["L"], c["hidden"], c["H"], c["W"]
    inp = G.gru_rollout("A")
    frames = torch.from_numpy(inp["depth"].reshape(c["T"], c["N"], H, W, 1)[:T + 1, :N].copy()).to(DEV)
    goals = torch.from_numpy(inp["goal"].reshape(c["T"], c["N"], 2)[:T + 1, :N].copy()).to(DEV)
    masks = torch.from_numpy(inp["masks"].reshape(c["T"], c["N"], 1)[:T + 1, :N].copy())
    assert masks[:T, :, 0].tolist() == [[0, 1], [1, 1], [1, 0], [1, 1]]
    pol, twin = make_policy("A"), make_policy("A")
    assert pol.net.num_recurrent_layers == L
    space = Space({"depth": Box((H, W, 1)), "rgb": Box((H, W, 3)), GOAL: Box((2,))})
    st = RolloutStorage(T, N, space, ActionSpace(c["A"]), Hd, pol.net.num_recurrent_layers, sensors=["depth", GOAL])
    st.to(DEV)
    assert tuple(st.recurrent_hidden_states.shape) == (T + 1, L, N, Hd)
    st.observations["depth"][0].copy_(frames[0])
    st.observations[GOAL][0].copy_(goals[0])
    st.recurrent_hidden_states[0].copy_(torch.from_numpy(inp["hidden"][:, :N].copy()))
    st.masks[0].copy_(masks[0])
    for t in range(T):
        obs = {k: v[st.step] for k, v in st.observations.items()}
        value, action, logp, hidden = pol.act(obs, st.recurrent_hidden_states[st.step], st.prev_actions[st.step], st.masks[st.step],
                                              deterministic=True)
        assert tuple(hidden.shape) == (L, N, Hd)
        rewards = torch.tensor([[0.25 * (t + 1)], [-0.5 + 0.125 * t]])
        st.insert({"depth": frames[t + 1], GOAL: goals[t + 1]}, hidden, action, logp, value, rewards, masks[t + 1])
    obs = {k: v[st.step] for k, v in st.observations.items()}
    next_value = pol.get_value(obs, st.recurrent_hidden_states[st.step], st.prev_actions[st.step], st.masks[st.step])
    st.compute_returns(next_value, True, 0.99, 0.95)
    torch.cuda.synchronize()
    assert st.step == T and st.recurrent_hidden_states[1:].abs().sum() > 0

    agent = PPO(pol, G.CLIP, 1, 1, G.VALUE_COEF, G.ENTROPY_COEF, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM,
                use_clipped_value_loss=True, use_normalized_advantage=True)
    # the piecewise path on a twin with the same weights and the same minibatch (the generator's permutation comes from torch's seed)
    step = PolicyTrainStep(twin, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    assert torch.equal(step.flat[:step.n_params], agent.train_step.flat[:step.n_params])
    torch.manual_seed(7)
    (mb,) = list(st.recurrent_generator(agent.get_advantages(st), 1))
    obs_b, hid_b, act_b, prev_b, vp_b, ret_b, mask_b, old_b, adv_b = mb
    assert tuple(hid_b.shape) == (L, N, Hd) and obs_b["depth"].shape[0] == T * N
    step.evaluate_actions(obs_b, hid_b, prev_b, mask_b, act_b)
    want = step.ppo_loss(old_b, adv_b, vp_b, ret_b, G.CLIP, G.VALUE_COEF, G.ENTROPY_COEF, True).cpu().tolist()
    before = agent.train_step.flat[:step.n_params].clone()
    torch.manual_seed(7)
    got = agent.update(st)
    torch.cuda.synchronize()
    print(f"[end to end] losses {got}")
    assert len(got) == 3 and all(isinstance(x, float) and np.isfinite(x) for x in got)
    assert list(got) == want, (got, want)
    assert agent.train_step.step_count == 1 and not torch.equal(before, agent.train_step.flat[:step.n_params])
