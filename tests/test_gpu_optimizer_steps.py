"""GPU (-m gpu): the optimiser step of every caller of pnvo_adam_step — VOTrainStep, PolicyTrainStep, BaselineTrainStep,
GeoInvarianceTrainStep — over SEVERAL steps with PRESCRIBED gradients: the sequences of tests/adam_reference.py, scaled per tensor
(1, 1e-3, 30, 1e-6: the last puts whole tensors where eps rules), are written into `step.grad`, and no forward or backward runs in between.
Nothing here is chaotic, so the bounds are those of adam_reference.close per parameter tensor (err <= margin * d32 + floor against
torch.optim.Adam in float64, d32 = torch's own float32 Adam on the same gradients), after EVERY step for the parameters and after the
last one for the moments.

  VOTrainStep            8 steps on the model of the model_default_45x37_b3 fixture: step count, flat / exp_avg / exp_avg_sq, the module's
                         state_dict (views of the flat buffer), and the eval forward on the re-packed operands against oracle.forward in
                         float64 on the reference's parameters.
  state dict <-> torch   4 steps on the HIP path, state_dict() into torch.optim.Adam over the model's parameters in named_parameters order,
                         4 more steps on both; and the converse, torch's state_dict() and parameters into a fresh model + VOTrainStep.
  PolicyTrainStep (ppo_reference case A), BaselineTrainStep (baseline_ppo_reference case D)
                         6 rounds of clip_grad_norm() + optimizer_step(), the gradient norm above max_grad_norm in some rounds and below it
                         in others, against ppo_reference.clip_and_adam threaded with state= and step=; once with a frozen encoder, whose
                         range of flat and of both moments (pre-filled, so that a decay would show) must stay bit-unchanged.
  GeoInvarianceTrainStep one process, two models: a model that never had a backward does not move; one that had and has no entries in
                         the batch takes an Adam step with an all-zero gradient at ITS OWN step count.

Measured on the MI355X, worst err / d32 per quantity over the tensors of all tests (bounds 4 / 8 / 3):
    parameters 1.06 (PolicyTrainStep A, frozen encoder, round 4: net.state_encoder.rnn.weight_ih_l1)
    exp_avg 1.00 (VOTrainStep, step 8: conv1.0.weight)      exp_avg_sq 1.87 (torch -> HIP, step 8: output_head.1.bias, three elements)
    eval forward after the eight VO steps: 1.2e-6 of the float64 oracle on the reference's parameters (bound 1e-4; the output of the
    initial weights lies 2.9e-2 away).
Wall time of the module on the MI355X host: 7 s for the 7 tests (VOTrainStep's 8 steps with two torch references of 5 M parameters: 2.9 s);
with tests/test_gpu_adam.py (5.1 s) and tests/test_adam_reference_host.py (0.1 s) the three new modules take 13 s.
"""
import copy

import numpy as np
import pytest
import torch

import adam_reference as A
import baseline_ppo_reference as BP
import ppo_reference as R
from conftest import golden_case, load_golden, pair_rel_err
from oracle import oracle
from oracle import torch_train_ref as ttr
from pointnav_vo_amd import vo_cnn  # noqa: F401
from pointnav_vo_amd.ppo import BaselineTrainStep, PolicyTrainStep
from pointnav_vo_amd.registry import baseline_registry
from pointnav_vo_amd.train import TURN_LEFT, TURN_RIGHT, GeoInvarianceTrainStep, VOTrainStep

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SCALES = (1.0, 1e-3, 30.0, 1e-6)
LR, BETAS = 2.5e-4, (0.9, 0.999)
WORST = A.Worst()


# ---------------------------------------------------------------------------------------------------------------------- helpers
def grad_sequence(offsets, total, K, skip=None, kind="normal"):
    """[K, total] float32: tensor i of `offsets` gets adam_reference.grads(kind, K, n, seed=i) * SCALES[i % 4]; gaps, the tail and the
    tensors whose name starts with `skip` stay zero."""
    G = np.zeros((K, total), np.float32)
    for i, (name, (off, n)) in enumerate(offsets.items()):
        if skip and name.startswith(skip):
            continue
        G[:, off:off + n] = A.grads(kind, K, n, seed=i) * np.float32(SCALES[i % len(SCALES)])
    return G


def by_name(offsets, flat):
    flat = np.asarray(flat)
    return {name: flat[off:off + n] for name, (off, n) in offsets.items()}


class TorchAdam:
    """The real torch.optim.Adam on the CPU over named tensors in `dtype`, optionally behind nn.utils.clip_grad_norm_."""

    def __init__(self, named, dtype, lr, eps, betas=BETAS, state_dict=None):
        self.names = [n for n, _ in named]
        self.params = [torch.nn.Parameter(torch.as_tensor(np.asarray(v)).to(dtype).clone()) for _, v in named]
        self.opt = torch.optim.Adam(self.params, lr=lr, betas=betas, eps=eps)
        if state_dict is not None:
            self.opt.load_state_dict(copy.deepcopy(state_dict))     # (torch keeps the `step` tensor it is given: never share one)

    def step(self, grads, max_norm=None):
        for name, p in zip(self.names, self.params):
            p.grad = torch.as_tensor(np.asarray(grads[name])).to(p.dtype).reshape(p.shape).clone()
        norm = None if max_norm is None else float(torch.nn.utils.clip_grad_norm_(self.params, max_norm))
        self.opt.step()
        return norm

    def state(self):
        """-> (params, exp_avg, exp_avg_sq): name -> flat float64 ndarray."""
        out = ({}, {}, {})
        for name, p in zip(self.names, self.params):
            st = self.opt.state[p]
            for d, t in zip(out, (p.detach(), st["exp_avg"], st["exp_avg_sq"])):
                d[name] = t.double().numpy().reshape(-1)
        return out


def read_back(step):
    """(flat, exp_avg, exp_avg_sq) of a train step as float64 host arrays."""
    torch.cuda.synchronize()
    return tuple(t.detach().cpu().double().numpy() for t in (step.flat, step.exp_avg, step.exp_avg_sq))


def compare(what, step, names, ref64, ref32, moments):
    """adam_reference's criterion per parameter tensor: the parameters, and with `moments` both moments -> list of failures."""
    got = [by_name(step.offsets, a) for a in read_back(step)]
    bad = []
    for q, which in enumerate(("param", "exp_avg", "exp_avg_sq")):
        if q and not moments:
            break
        for name in names:
            g, r64, r32 = got[q][name], ref64[q][name].reshape(-1), ref32[q][name].reshape(-1)
            ok, err, d32 = A.close_params(g, r64, r32) if q == 0 else A.close_moment(which, g, r64, r32)
            WORST.add(which, f"{what}: {name}", err, d32)
            if not ok:
                bad.append((what, which, name, err, d32))
    return bad


def vo_model(rec, sd=None):
    cfg, sd0, obs, _ = golden_case(rec)
    space = str(rec["obs_space"]).split(",")
    model = baseline_registry.get_vo_model(str(rec["model"]))(
        observation_space=space, observation_size=(cfg.width, cfg.height), hidden_size=512, backbone="resnet18",
        normalize_visual_inputs=True, output_dim=3, dropout_p=0.0, discretized_depth_channels=int(rec["dd_bins"]))
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in (sd or sd0).items()})
    return model.to(DEV), cfg, sd0, obs


def is_buffer(name):
    return name.rsplit(".", 1)[-1] in ("_mean", "_var", "_count")


def run_steps(ts, G, ks, refs, what, names):
    """Write G[k] into ts.grad and step, for k in ks; the references step along; parameters compared after every step."""
    bad = []
    for k in ks:
        ts.grad.copy_(torch.from_numpy(G[k]).to(DEV))
        ts.optimizer_step()
        g = by_name(ts.offsets, G[k])
        for r in refs:
            r.step(g)
        bad += compare(f"{what}, step {k + 1}", ts, names, refs[0].state(), refs[1].state(), moments=k == ks[-1])
    return bad


# ---------------------------------------------------------------------------------------------------------------------- VOTrainStep
def test_vo_train_step_follows_fp64_adam_for_eight_steps_and_the_forward_reads_the_stepped_weights():
    rec = load_golden("model_default_45x37_b3.npz")
    model, cfg, sd, obs = vo_model(rec)
    tobs = {k: torch.from_numpy(v).to(DEV) for k, v in obs.items()}
    with torch.no_grad():
        out0 = model.eval()(tobs).cpu().numpy()
    ts = VOTrainStep(model, lr=LR, eps=1e-8)
    assert ts.dropout_p == 0.0
    names = list(ts.offsets)
    K = 8
    G = grad_sequence(ts.offsets, ts.flat.numel(), K)
    named = [(n, sd[n]) for n in names]
    refs = [TorchAdam(named, dt, LR, 1e-8) for dt in (torch.float64, torch.float32)]
    bad = run_steps(ts, G, range(K), refs, "VOTrainStep", names)
    print("worst err/d32 so far:", WORST)
    assert not bad, bad[:6]
    assert ts.step_count == K
    msd = model.state_dict()
    for name, (off, n) in ts.offsets.items():                                        # the module's parameters are views of the flat buffer
        assert torch.equal(msd[name].reshape(-1), ts.flat[off:off + n]), name
    # the eval forward runs on the operands re-packed after the LAST step (float16-piece range bounds lag two refreshes)
    p64 = refs[0].state()[0]
    newsd = {k: (np.asarray(v, np.float64) if is_buffer(k) else p64[k].reshape(np.shape(v))) for k, v in sd.items()}
    want = oracle.forward(newsd, obs, ngroups=cfg.ngroups, dtype=np.float64)
    with torch.no_grad():
        got = model.eval()(tobs).cpu().numpy()
    err = pair_rel_err(got, want)
    moved = pair_rel_err(out0, want)
    print(f"[VOTrainStep] eval forward after {K} steps: {err.max():.2e} of the fp64 oracle on the reference's parameters "
          f"(the initial weights' output is {moved.min():.2e} away)")
    assert moved.min() > 1e-2, moved                     # the eight steps moved the output: stale operands would not pass
    assert err.max() < 1e-4, err


def test_vo_optimizer_state_dict_continues_in_torch_and_torchs_continues_here():
    rec = load_golden("model_default_45x37_b3.npz")
    model, cfg, sd, obs = vo_model(rec)
    ts = VOTrainStep(model, lr=LR, eps=1e-8)
    names = [n for n, _ in model.named_parameters()]
    assert names == list(ts.offsets)
    G = grad_sequence(ts.offsets, ts.flat.numel(), 8)

    def host_params(m):
        return [(n, p.detach().cpu().numpy().copy()) for n, p in m.named_parameters()]

    # 1. four steps here, the state dict into torch (float32 as the yardstick, float64 as the reference), four more on all three
    for k in range(4):
        ts.grad.copy_(torch.from_numpy(G[k]).to(DEV))
        ts.optimizer_step()
    torch.cuda.synchronize()
    ckpt, params = ts.state_dict(), host_params(model)
    assert all(int(st["step"]) == 4 for st in ckpt["state"].values()) and len(ckpt["state"]) == len(names)
    refs = [TorchAdam(params, dt, 1.0, 1.0, (0.0, 0.0), state_dict=ckpt) for dt in (torch.float64, torch.float32)]   # the group comes from the checkpoint
    g0 = refs[1].opt.param_groups[0]
    assert (g0["lr"], tuple(g0["betas"]), g0["eps"]) == (LR, BETAS, 1e-8)
    bad = run_steps(ts, G, range(4, 8), refs, "HIP -> torch", names)
    assert ts.step_count == 8 and int(refs[1].opt.state[refs[1].params[0]]["step"]) == 8
    # 2. four steps of torch's float32 Adam from the initial weights, its state dict and parameters into a fresh model + step
    t32 = TorchAdam([(n, sd[n]) for n in names], torch.float32, LR, 1e-8)
    for k in range(4):
        t32.step(by_name(ts.offsets, G[k]))
    ckpt2 = copy.deepcopy(t32.opt.state_dict())
    model2, *_ = vo_model(rec)
    ts2 = VOTrainStep(model2, lr=1.0, eps=1.0, betas=(0.0, 0.0))
    full = {k: v.detach().cpu().clone() for k, v in model2.state_dict().items()}
    full.update({n: p.detach().clone() for n, p in zip(names, t32.params)})
    model2.load_state_dict(full)                                   # lands in the flat buffer, after the attach
    ts2.load_state_dict(ckpt2)
    assert (ts2.step_count, ts2.lr, tuple(ts2.betas), ts2.eps) == (4, LR, BETAS, 1e-8)
    t64 = TorchAdam([(n, p.detach().numpy()) for n, p in zip(names, t32.params)], torch.float64, 1.0, 1.0, (0.0, 0.0), state_dict=ckpt2)
    bad += run_steps(ts2, G, range(4, 8), [t64, t32], "torch -> HIP", names)
    print("worst err/d32 so far:", WORST)
    assert not bad, bad[:6]
    assert ts2.step_count == 8


# ---------------------------------------------------------------------------------------------------------------------- PPO steps
ROUNDS = (3.0, 0.3, 1.5, 0.5, 2.0, 0.8)          # the gradient norm of each round in units of max_grad_norm: clipped, not, ...


def ppo_rounds(make_step, sd, lr, eps, max_norm, enc_prefix, train_encoder, what):
    """Six rounds of clip_grad_norm() + optimizer_step() on prescribed gradients against ppo_reference.clip_and_adam (float64) and
    torch's float32 clip_grad_norm_ + Adam."""
    step = make_step(train_encoder)
    names = list(step.offsets)
    frozen = () if train_encoder else (enc_prefix,)
    live = [n for n in names if not (frozen and n.startswith(frozen))]
    assert train_encoder or len(live) < len(names)
    end = max(o + k for o, k in step.offsets.values())
    G = grad_sequence(step.offsets, step.grad.numel(), len(ROUNDS), skip=None if train_encoder else enc_prefix)
    for k, f in enumerate(ROUNDS):                    # the norm of round k: f * max_grad_norm (float64 arithmetic, then float32 values)
        G[k] = (G[k].astype(np.float64) * (f * max_norm / np.linalg.norm(G[k].astype(np.float64)))).astype(np.float32)
    tail = np.zeros(step.grad.numel(), np.float32)
    tail[end:] = 0.25                                 # what a backward may leave behind the last parameter: not a gradient of anything
    if not train_encoder:
        # moments a stepped-over range would decay and apply: the frozen range must keep them, and its parameters, bit for bit
        lo, hi = step.encoder_range
        rng = np.random.default_rng(5)
        step.exp_avg[lo:hi] = torch.from_numpy((1e-2 * rng.standard_normal(hi - lo)).astype(np.float32)).to(DEV)
        step.exp_avg_sq[lo:hi] = torch.from_numpy((1e-4 * rng.random(hi - lo)).astype(np.float32)).to(DEV)
        frozen_before = [t[lo:hi].clone() for t in (step.flat, step.exp_avg, step.exp_avg_sq)]
    P64, state = {n: np.asarray(sd[n], np.float64) for n in names}, None
    t32 = TorchAdam([(n, sd[n]) for n in live], torch.float32, lr, eps)
    bad, clipped = [], []
    for k in range(len(ROUNDS)):
        step.grad.copy_(torch.from_numpy(G[k] + tail).to(DEV))
        gnorm = step.clip_grad_norm()
        step.optimizer_step()
        g = by_name(step.offsets, G[k])
        P64, norm, coef, state = R.clip_and_adam(P64, {n: g[n].astype(np.float64).reshape(np.shape(sd[n])) for n in names}, lr=lr, eps=eps,
                                                 max_norm=max_norm, frozen=frozen, state=state, step=k + 1)
        clipped.append(coef < 1.0)
        n32 = t32.step({n: g[n] for n in live}, max_norm=max_norm)
        assert abs(float(gnorm) - norm) < 1e-4 * norm, (k, float(gnorm), norm)
        assert abs(n32 - norm) < 1e-4 * norm
        ref64 = ({n: P64[n].reshape(-1) for n in live}, {n: state[n][0].numpy().reshape(-1) for n in live},
                 {n: state[n][1].numpy().reshape(-1) for n in live})
        bad += compare(f"{what}, round {k + 1}", step, live, ref64, t32.state(), moments=k == len(ROUNDS) - 1)
    print("worst err/d32 so far:", WORST)
    assert clipped == [f > 1.0 for f in ROUNDS] and any(clipped) and not all(clipped), clipped
    assert not bad, bad[:6]
    assert step.step_count == len(ROUNDS)
    torch.cuda.synchronize()
    # behind the last parameter (the final alignment gap; the library's tail starts there) no moment is collected
    assert not step.exp_avg[end:].any() and not step.exp_avg_sq[end:].any()
    if not train_encoder:
        for t, b in zip((step.flat, step.exp_avg, step.exp_avg_sq), frozen_before):
            assert torch.equal(t[lo:hi], b)
        assert b.any()


@pytest.mark.parametrize("train_encoder", [True, False])
def test_policy_train_step_clips_and_steps_like_fp64_for_six_rounds(train_encoder):
    from test_gpu_ppo import EPS, MAX_GRAD_NORM, make_policy
    make = lambda te: PolicyTrainStep(make_policy("A"), lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM, train_encoder=te)
    ppo_rounds(make, R.state_dict("A"), LR, EPS, MAX_GRAD_NORM, R.ENC, train_encoder, f"PolicyTrainStep A, train_encoder={train_encoder}")


@pytest.mark.parametrize("train_encoder", [True, False])
def test_baseline_train_step_clips_and_steps_like_fp64_for_six_rounds(train_encoder):
    from test_gpu_baseline_ppo import make_policy
    make = lambda te: BaselineTrainStep(make_policy("D"), lr=BP.LR, eps=BP.EPS, max_grad_norm=BP.MAX_GRAD_NORM, train_encoder=te)
    ppo_rounds(make, BP.state_dict("D"), BP.LR, BP.EPS, BP.MAX_GRAD_NORM, BP.ENC, train_encoder,
               f"BaselineTrainStep D, train_encoder={train_encoder}")


# ---------------------------------------------------------------------------------------------------------------------- absent models
def test_a_model_without_entries_takes_a_zero_gradient_step_at_its_own_count_and_none_before_its_first_backward():
    rec = load_golden("model_default_45x37_b3.npz")
    _, sd, obs, _ = golden_case(rec)
    steps, rmv = {}, {}
    for act, seed_shift in ((TURN_LEFT, 0.0), (TURN_RIGHT, 0.01)):
        model, cfg, sd0, obs = vo_model(rec, {k: (v if is_buffer(k) else v + np.float32(seed_shift)) for k, v in sd.items()})
        steps[act] = VOTrainStep(model, lr=LR, eps=1e-8)
        rmv[act] = model.visual_encoder.running_mean_and_var
    js = GeoInvarianceTrainStep(steps, invariance_types=())
    tobs = {k: torch.from_numpy(v).to(DEV) for k, v in obs.items()}
    M = next(iter(tobs.values())).shape[0]
    assert M == 3
    target = torch.from_numpy(np.random.default_rng(3).uniform(-0.25, 0.25, (M, 3)).astype(np.float32))
    types = np.zeros(M, np.int64)

    def snapshot(act):
        torch.cuda.synchronize()
        st, r = steps[act], rmv[act]
        return [t.detach().clone() for t in (st.flat, st.exp_avg, st.exp_avg_sq, r._mean, r._var, r._count)]

    def zero_gradient_step(before, after, step_count, act):
        """`after` against one float64 Adam step with g = 0 at `step_count` from `before`."""
        p, m, v = (t.cpu().double() for t in before[:3])
        rp, rm, rv = ttr.adam_step(p, torch.zeros_like(p), m, v, step_count, LR, BETAS[0], BETAS[1], 1e-8)
        gp, gm, gv = (t.cpu().double() for t in after[:3])
        ulp = torch.from_numpy(np.spacing(np.abs(rp.numpy()).astype(np.float32)).astype(np.float64))
        over = ((gp - rp).abs() - ulp - 1e-6 * LR).max()
        assert over <= 0, (act, "parameters", float(over))
        for name, (off, n) in steps[act].offsets.items():
            for which, g, r in (("exp_avg", gm, rm), ("exp_avg_sq", gv, rv)):
                rel = float((g[off:off + n] - r[off:off + n]).norm() / r[off:off + n].norm().clamp_min(1e-300))
                assert rel <= A.ULP32, (act, which, name, rel)
        moved = float((gp != p).double().mean())
        assert moved > 0.5, (act, moved)                            # the decayed moments were applied
        assert all(torch.equal(a, b) for a, b in zip(after[3:], before[3:]))      # no forward ran: RunningMeanAndVar stays

    # iteration 1, left only: the right model never had a backward and must not move at all
    right0 = snapshot(TURN_RIGHT)
    js.step(tobs, np.full(M, TURN_LEFT), types, target)
    assert all(torch.equal(a, b) for a, b in zip(snapshot(TURN_RIGHT), right0))
    assert (steps[TURN_LEFT].step_count, steps[TURN_RIGHT].step_count) == (1, 0)
    # iteration 2, right only: both step; the left model with an all-zero gradient, at its step 2
    left1 = snapshot(TURN_LEFT)
    assert left1[1].any() and left1[2].any()
    js.step(tobs, np.full(M, TURN_RIGHT), types, target)
    assert (steps[TURN_LEFT].step_count, steps[TURN_RIGHT].step_count) == (2, 1)
    zero_gradient_step(left1, snapshot(TURN_LEFT), 2, TURN_LEFT)
    # iteration 3, left only: the same for the right model, at ITS step 2 (the left model is at 3)
    right1 = snapshot(TURN_RIGHT)
    js.step(tobs, np.full(M, TURN_LEFT), types, target)
    assert (steps[TURN_LEFT].step_count, steps[TURN_RIGHT].step_count) == (3, 2)
    zero_gradient_step(right1, snapshot(TURN_RIGHT), 2, TURN_RIGHT)
