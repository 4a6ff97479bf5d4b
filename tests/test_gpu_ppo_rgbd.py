"""GPU (-m gpu): one PPO minibatch update of the navigation policy with rgb / rgb-d input and RunningMeanAndVar (pointnav_vo_amd.ppo on
pnvo_policy_evaluate_rgbd / _ppo_loss / _backward: policy_input_kernel, the train-mode encoder forward on the updated statistics, the
stem gradient copied back from the handle's 2C channels) against the torch-CPU float64 model of tests/rgbd_policy_reference.py
(autograd), which tests/test_policy_rgbd_host.py pins to the reference policy.

Cases (frames 96 x 128, hidden 128, 2 layers, 4 actions; the policy in training mode, statistics zero-initialised):
  RGBD  rgb + depth, LSTM, T = 3, N = 2: a start reset and a mid-sequence reset of one environment, a non-zero initial state
  RGB   rgb alone, GRU, T = 1, N = 3: the M == N single-step form

Tolerances.  Forward: 2e-4 of each tensor's scale.  Loss: 1e-4 * max(1, |x|).  Gradients, relative L2 per parameter tensor and per input
channel of the stem weight: the float64 model run in float32 on the CPU (python tests/rgbd_policy_reference.py) deviates from its
float64 self by at most 3.711e-06 over the cases (worst: critic.fc.bias of RGB; RGBD 3.23e-06, a GroupNorm weight of layer1; medians
2.1-2.4e-06); GRAD_TOL = 10 x that = 3.7e-5, the rule that gave GRAD_TOL of tests/test_gpu_ppo.py.
Statistics after one and after two evaluate_actions calls: the float32 model's _mean / _var deviate by at most 1.27e-07 / 1.50e-07 of
the tensor's largest magnitude; STAT_TOL = 10 x that.  _count is exact.
Step: the shipped optimiser settings (lr 2.5e-4, eps 1e-5, max_grad_norm 0.2); on them the float32 model's gradients put the
parameters within 6.13e-08 of the float64 ones after clip + Adam; atol = 10 x that = 6.2e-7 (the rule of tests/test_gpu_ppo_gru.py).
"""
import functools

import numpy as np
import pytest
import torch

import rgbd_policy_reference as Q
from pointnav_vo_amd import synth
from pointnav_vo_amd.policy import RMV_PREFIX, PointNavResNetPolicy
from pointnav_vo_amd.ppo import PPO, PolicyTrainStep
from pointnav_vo_amd.rollout_storage import RolloutStorage

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TOL = 2e-4
GRAD_TOL = 3.7e-5
STAT_TOL = {"_mean": 1.27e-6, "_var": 1.50e-6}
STEP_ATOL = 6.2e-7
LR, EPS, MAX_GRAD_NORM = 2.5e-4, 1e-5, 0.2               # configs/rl/ddppo_pointnav.yaml
GOAL = Q.GOAL


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


def make_policy(case):
    c = Q.CASES[case]
    space = Space({"depth": Box((c["H"], c["W"], 1)), "rgb": Box((c["H"], c["W"], 3)), GOAL: Box((2,))})
    pol = PointNavResNetPolicy(observation_space=space, action_space=Act(c["A"]), hidden_size=c["hidden"], rnn_type=c["rnn"],
                               num_recurrent_layers=c["L"], backbone="resnet18", goal_sensor_uuid=GOAL,
                               normalize_visual_inputs=True, obs_transform=None, vis_types=list(c["vis"]))
    sd = Q.state_dict(case)
    assert list(pol.state_dict().keys()) == list(sd.keys())
    pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return pol.to(DEV).train()


def buffers(pol):
    rmv = pol.net.visual_encoder.running_mean_and_var
    return {"_mean": rmv._mean, "_var": rmv._var, "_count": rmv._count}


def stats_numpy(pol):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy().copy() for k, v in buffers(pol).items()}


def close(got, want, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got.reshape(want.shape) - want).max() / (np.abs(want).max() + 1e-6)
    return err < tol, err


def loss_close(got, want):
    return abs(got - want) < 1e-4 * max(1.0, abs(want))


def to_gpu(inp):
    M = inp["T"] * inp["N"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    obs = {k: t(inp[k]) for k in ("rgb", "depth") if k in inp}
    obs[GOAL] = t(inp["goal"])
    return obs, t(inp["hidden"]), t(inp["prev"]).view(M, 1), t(inp["masks"]).view(M, 1), t(inp["actions"]).view(M, 1)


def run_update(step, inp, li):
    """evaluate_actions + ppo_loss + backward on the GPU -> numpy results (the gradient buffer is copied out)."""
    obs, hidden, prev, masks, actions = to_gpu(inp)
    value, logp, entropy, hout = step.evaluate_actions(obs, hidden, prev, masks, actions)
    t = lambda k: torch.from_numpy(li[k]).to(DEV)
    out3 = step.ppo_loss(t("old"), t("adv"), t("vp"), t("ret"), Q.CLIP, Q.VALUE_COEF, Q.ENTROPY_COEF, True)
    step.backward()
    torch.cuda.synchronize()
    return dict(value=value.cpu().numpy(), logp=logp.cpu().numpy(), entropy=float(entropy), hidden=hout.cpu().numpy(),
                losses=out3.cpu().numpy().astype(np.float64), grad=step.grad.cpu().double().numpy(), shapes=(value.shape, logp.shape),
                stats=stats_numpy(step.policy))


@functools.lru_cache(maxsize=None)
def gpu_case(case):
    """The policy of a case (training mode, zero statistics) with a train step attached, one update's results, and the statistics
    after a second evaluate_actions on other frames: shared by the forward / loss / gradient / statistics tests."""
    pol = make_policy(case)
    ptrs = [b.data_ptr() for b in buffers(pol).values()]
    step = PolicyTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    assert [b.data_ptr() for b in buffers(pol).values()] == ptrs        # attaching moves the parameters, never the buffers
    got = run_update(step, Q.rollout(case), Q.reference(case)["loss_inputs"])
    step.evaluate_actions(*to_gpu(Q.rollout(case, 1)))
    got["stats2"] = stats_numpy(pol)
    assert [b.data_ptr() for b in buffers(pol).values()] == ptrs
    return pol, step, got


def grad_errors(step, grad, ref_grads, what):
    """Per-tensor relative L2 against float64 autograd, the stem weight also per input channel; a zero reference gradient must be
    exactly zero."""
    errs, ref = {}, Q.with_stem_channels(ref_grads)
    off, n = step.offsets[Q.STEM]
    got = {name: grad[o:o + k] for name, (o, k) in step.offsets.items()}
    stem = got[Q.STEM].reshape(ref_grads[Q.STEM].shape)
    for c in range(stem.shape[1]):
        got[f"{Q.STEM}[:, {c}]"] = stem[:, c]
    assert set(got) == set(ref)
    for name, g in got.items():
        gr = ref[name].reshape(-1)
        if not gr.any():
            assert not g.any(), (what, name, "reference gradient is exactly zero, the HIP gradient is not")
            continue
        errs[name] = np.linalg.norm(g.reshape(-1) - gr) / max(np.linalg.norm(gr), 1e-12)
    worst = max(errs, key=errs.get)
    print(f"[{what}] worst gradient tensor {errs[worst]:.2e} ({worst}), median {np.median(list(errs.values())):.2e}, GRAD_TOL {GRAD_TOL:.2e}")
    return errs


def assert_stats(got, want, what):
    assert float(got["_count"]) == float(want["_count"]), (what, got["_count"], want["_count"])
    for k, tol in STAT_TOL.items():
        w = np.asarray(want[k], np.float64)
        e = np.abs(got[k].astype(np.float64).reshape(w.shape) - w).max() / np.abs(w).max()
        print(f"[{what}] {k}: {e:.2e} of the largest magnitude (STAT_TOL {tol:.2e})")
        assert e <= tol, (what, k, e)


# ------------------------------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("case", ["RGBD", "RGB"])
def test_forward_matches_fp64(case):
    pol, step, got = gpu_case(case)
    ref, inp, c = Q.reference(case), Q.rollout(case), Q.CASES[case]
    M = inp["T"] * inp["N"]
    assert got["shapes"] == ((M, 1), (M, 1)) and got["hidden"].shape == ref["hidden"].shape
    assert got["hidden"].shape[0] == c["L"] * (2 if c["rnn"] == "LSTM" else 1)
    for k in ("value", "logp", "hidden"):
        ok, err = close(got[k], ref[k])
        print(f"[{case}] {k}: {err:.2e} of scale")
        assert ok, (case, k, err)
    ok, err = close(got["entropy"], ref["entropy"])
    assert ok, (case, "entropy", err)


# ------------------------------------------------------------------------------------------------------------------ 2. loss
@pytest.mark.parametrize("case", ["RGBD", "RGB"])
def test_loss_matches_fp64(case):
    ref = Q.reference(case)
    s, v, margin = Q.branch_census(ref["value"], ref["logp"], ref["loss_inputs"])     # from the float64 side alone
    adv = ref["loss_inputs"]["adv"]
    assert margin.min() > 1e-6 and (adv > 0).any() and (adv < 0).any()
    assert min(int(s.sum()), int((~s).sum()), int(v.sum()), int((~v).sum())) >= 1, (s, v)      # every branch of each clamp is live
    _, _, got = gpu_case(case)
    for k, g, w in zip(("value_loss", "action_loss", "dist_entropy"), got["losses"], ref["losses"]):
        print(f"[{case}] {k}: {g:.8f} vs {w:.8f}")
        assert loss_close(g, w), (case, k, g, w)


# ------------------------------------------------------------------------------------------------------------------ 3. gradients
@pytest.mark.parametrize("case", ["RGBD", "RGB"])
def test_gradients_match_fp64_autograd(case):
    _, step, got = gpu_case(case)
    ref = Q.reference(case)
    C = len(Q.CASES[case]["vis"]) + (2 if "rgb" in Q.CASES[case]["vis"] else 0)
    assert ref["grads"][Q.STEM].shape == (32, C, 7, 7) and step.offsets[Q.STEM][1] == 32 * C * 49
    errs = grad_errors(step, got["grad"], ref["grads"], case)
    assert all(f"{Q.STEM}[:, {c}]" in errs for c in range(C))                  # every input channel carries a gradient
    assert max(errs.values()) <= GRAD_TOL, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    assert not any(n.startswith(RMV_PREFIX) for n in step.offsets)             # the statistics receive no gradient: they are not in the store


# ------------------------------------------------------------------------------------------------------------------ 4. statistics
@pytest.mark.parametrize("case", ["RGBD", "RGB"])
def test_statistics_after_one_and_two_evaluate_actions(case):
    _, _, got = gpu_case(case)
    ref, c = Q.reference(case), Q.CASES[case]
    M = c["T"] * c["N"]
    assert float(ref["stats"]["_count"]) == M and float(ref["stats2"]["_count"]) == 2 * M     # the M rows are one batch
    assert_stats(got["stats"], ref["stats"], f"{case}, one call")
    assert_stats(got["stats2"], ref["stats2"], f"{case}, two calls")
    v = np.asarray(ref["stats"]["_var"]).reshape(-1)
    assert ((v > 2e-2) | (v < 5e-3)).all()                                     # clear of the 1e-2 clamp


# ------------------------------------------------------------------------------------------------------------------ 5. step
def test_step_matches_fp64_adam_and_the_optimiser_knows_no_statistics():
    case = "RGBD"
    pol = make_policy(case)
    step = PolicyTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    ref = Q.reference(case)
    newp, norm, coef, _ = Q.clip_and_adam(ref["params"], ref["grads"], lr=LR, eps=EPS, max_norm=MAX_GRAD_NORM)
    assert coef < 1.0                                      # the clipping is live
    sel = {k: np.abs(g) > 1e-6 * max(np.abs(g).max(), 1e-30) for k, g in ref["grads"].items()}
    run_update(step, Q.rollout(case), ref["loss_inputs"])
    stats = stats_numpy(pol)
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
    print(f"[step] worst parameter difference after clip + Adam: {worst:.2e}")
    # Adam stepped the parameters only: the statistics keep the bits the evaluate left, and no optimiser entry names them
    assert all(np.array_equal(stats_numpy(pol)[k], stats[k]) for k in stats)
    names = [n for n, _ in pol.named_parameters()]
    osd = step.state_dict()
    assert len(osd["state"]) == len(names) == len(osd["param_groups"][0]["params"]) and not any(RMV_PREFIX in n for n in names)
    assert [tuple(osd["state"][i]["exp_avg"].shape) for i in range(len(names))] == [tuple(p.shape) for _, p in pol.named_parameters()]
    assert set(pol.state_dict()) - set(names) == {RMV_PREFIX + k for k in Q.STATS}
    # the act path reads the stepped weights and the same buffers
    inp = Q.rollout(case)
    obs, hidden, prev, masks, _ = to_gpu(inp)
    N = inp["N"]
    pol.eval()
    value = pol.get_value({k: v[:N] for k, v in obs.items()}, hidden, prev[:N], masks[:N])
    sd_new = Q.with_stats({k: newp[k] for k in newp}, {k: stats[k] for k in stats})
    want = Q.policy_step(sd_new, {k: inp[k][:N] for k in ("rgb", "depth")}, inp["goal"][:N], inp["prev"][:N], inp["masks"][:N],
                         inp["hidden"], Q.CASES[case]["rnn"], False)
    ok, err = close(value.cpu().numpy(), want["value"])
    assert ok, err


def test_frozen_encoder_leaves_its_range_zero_but_updates_the_statistics():
    case = "RGBD"
    pol = make_policy(case)
    step = PolicyTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM, train_encoder=False)
    ref = Q.reference(case)
    got = run_update(step, Q.rollout(case), ref["loss_inputs"])
    lo, hi = step.encoder_range
    assert hi > lo and not got["grad"][lo:hi].any()
    assert not got["grad"][step.n_params:].any()
    assert_stats(got["stats"], ref["stats"], "frozen encoder")              # training mode: the reference's module would update too
    want = {k: (np.zeros_like(g) if k.startswith(Q.ENC) else g) for k, g in ref["grads"].items()}
    errs = grad_errors(step, got["grad"], want, "RGBD, frozen encoder")
    assert "net.visual_fc.1.weight" in errs and max(errs.values()) <= GRAD_TOL, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    before = step.flat.clone()
    step.clip_grad_norm()
    step.optimizer_step()
    torch.cuda.synchronize()
    assert torch.equal(before[lo:hi], step.flat[lo:hi]) and not torch.equal(before, step.flat)
    # .eval(): evaluate_actions reads the statistics and leaves them alone
    pol.eval()
    st = stats_numpy(pol)
    step.evaluate_actions(*to_gpu(Q.rollout(case, 1)))
    assert all(np.array_equal(stats_numpy(pol)[k], st[k]) for k in st)


# ------------------------------------------------------------------------------------------------------------------ 6. end to end
def test_rollout_storage_with_rgb_and_depth_feeds_ppo_update():
    """A RolloutStorage that holds rgb (float32 0..255, as batch_obs hands it) and depth, filled by act() in training mode for T = 3,
    N = 2, compute_returns, then PPO.update with two epochs of one minibatch: three finite floats, the parameters move, and the
    statistics have merged every batch they were shown (T collection steps and get_value of N frames, 2 minibatches of T * N)."""
    c = Q.CASES["RGBD"]
    T, N, L, Hd, H, W = 3, 2, c["L"], c["hidden"], c["H"], c["W"]
    steps = synth.make_policy_rgbd_inputs(H, W, N, T + 1, 91, c["A"])
    pol = make_policy("RGBD")
    space = Space({"depth": Box((H, W, 1)), "rgb": Box((H, W, 3)), GOAL: Box((2,))})
    st = RolloutStorage(T, N, space, ActionSpace(c["A"]), Hd, pol.net.num_recurrent_layers, sensors=["rgb", "depth", GOAL])
    st.to(DEV)
    assert st.observations["rgb"].dtype == torch.float32 and tuple(st.observations["rgb"].shape) == (T + 1, N, H, W, 3)
    frame = lambda t: {"rgb": torch.from_numpy(steps[t][0]).float().to(DEV), "depth": torch.from_numpy(steps[t][1]).to(DEV),
                       GOAL: torch.from_numpy(steps[t][2]).to(DEV)}
    for k, v in frame(0).items():
        st.observations[k][0].copy_(v)
    st.masks[0].zero_()
    for t in range(T):
        obs = {k: v[st.step] for k, v in st.observations.items()}
        value, action, logp, hidden = pol.act(obs, st.recurrent_hidden_states[st.step], st.prev_actions[st.step], st.masks[st.step])
        rewards = torch.tensor([[0.25 * (t + 1)], [-0.5 + 0.125 * t]])
        st.insert(frame(t + 1), hidden, action, logp, value, rewards, torch.from_numpy(steps[t + 1][4]).view(N, 1))
    obs = {k: v[st.step] for k, v in st.observations.items()}
    next_value = pol.get_value(obs, st.recurrent_hidden_states[st.step], st.prev_actions[st.step], st.masks[st.step])
    st.compute_returns(next_value, True, 0.99, 0.95)
    assert float(stats_numpy(pol)["_count"]) == (T + 1) * N
    agent = PPO(pol, Q.CLIP, 2, 1, Q.VALUE_COEF, Q.ENTROPY_COEF, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM,
                use_clipped_value_loss=True, use_normalized_advantage=True)
    before = agent.train_step.flat[:agent.train_step.n_params].clone()
    got = agent.update(st)
    torch.cuda.synchronize()
    print(f"[end to end] losses {got}")
    assert len(got) == 3 and all(isinstance(x, float) and np.isfinite(x) for x in got)
    assert agent.train_step.step_count == 2 and not torch.equal(before, agent.train_step.flat[:agent.train_step.n_params])
    after = stats_numpy(pol)
    assert float(after["_count"]) == (T + 1) * N + 2 * T * N and np.isfinite(after["_mean"]).all() and (after["_var"] > 0).all()
