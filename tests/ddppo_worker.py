"""Worker of tests/test_gpu_ddppo_multi.py: two ranks (torch.distributed.run) of the data-parallel PPO agent, pointnav_vo_amd.ddppo.DDPPO.
    --mode C | B1 | RGBD : each rank takes its environment columns of a case the float64 models of tests/ppo_reference.py /
                   tests/rgbd_policy_reference.py cover (row t*N + n goes to the rank that owns environment n; equal shards, so the mean
                   over the ranks of the per-rank gradients is the float64 gradient of the whole case).  Checked: the broadcast of
                   init_distributed, the ranges the gradient hook reported (disjoint, inside the parameters, complete, equal to
                   pnvo_policy_grad_buckets), the all-reduced averaged gradient per tensor, the parameters after before_step +
                   optimizer_step, RGBD's statistics after one and two evaluate_actions, bit-identical ranks, and the flat all-reduce
                   schedule against the bucketed one.  B1 also runs the frozen-encoder and the visual_features backward.
    --mode update : DDPPO.get_advantages (normalised) against numpy on the concatenation, then one DDPPO.update per rank through
                   RolloutStorage.recurrent_generator on a normalising policy, rank 0 with a full rollout and rank 1 with one that
                   ended a step early: finite losses, bit-identical parameters, moments and statistics.
    --shared-gpu : both ranks use cuda:0 and the collectives go through gloo; without it backend nccl (= RCCL), one GPU per rank.
Exit code 0 = all assertions held; the first failed assertion ends the rank."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ppo_reference as R  # noqa: E402
import rgbd_policy_reference as Q  # noqa: E402
import test_gpu_ppo as TP  # noqa: E402   (its policy builder and tolerances: the same comparison against the same reference)
import test_gpu_ppo_rgbd as TQ  # noqa: E402
from pointnav_vo_amd import synth  # noqa: E402
from pointnav_vo_amd.ddppo import DDPPO  # noqa: E402
from pointnav_vo_amd.ppo import ENCODER_PREFIX, EPS_PPO  # noqa: E402
from pointnav_vo_amd.rollout_storage import RolloutStorage  # noqa: E402

LR, EPS, MAX_GRAD_NORM = TP.LR, TP.EPS, TP.MAX_GRAD_NORM           # the shipped settings (lr 2.5e-4, eps 1e-5, max_grad_norm 0.2)
STEP_ATOL = {"C": 2e-6, "B1": 2e-6, "RGBD": TQ.STEP_ATOL}          # the step tests' atol of tests/test_gpu_ppo.py / _ppo_rgbd.py
GRAD_TOL = {"C": TP.GRAD_TOL, "B1": TP.GRAD_TOL, "RGBD": TQ.GRAD_TOL}
GOAL = R.GOAL


def same_on_all_ranks(t, what):
    """Bit-identical on the ranks, compared through the CPU (as mgpu_worker.geo does)."""
    c = t.detach().reshape(-1).cpu().contiguous()
    parts = [torch.empty_like(c) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, c)
    for p in parts[1:]:
        diff = (parts[0] != p).nonzero().flatten()
        assert diff.numel() == 0, (dist.get_rank(), what, f"{diff.numel()} values differ, the first at {int(diff[0])} of {c.numel()}")


def shard(inp, rank, world, keys):
    """The rows of the environments rank `rank` owns, T-major, and those environments' initial state."""
    T, N = inp["T"], inp["N"]
    per = N // world
    envs = list(range(rank * per, (rank + 1) * per))
    rows = np.array([t * N + n for t in range(T) for n in envs])
    out = {k: np.ascontiguousarray(inp[k][rows]) for k in keys}
    out.update(hidden=np.ascontiguousarray(inp["hidden"][:, envs]), T=T, N=per)
    return out, rows


class Recorder:
    """Wraps the agent's bucket all-reduce: the ranges the gradient hook reported in one backward, in order."""

    def __init__(self, agent):
        self.ranges = []
        start = agent._buckets.start

        def recording(grad, first, count):
            self.ranges.append((first, count))
            start(grad, first, count)
        agent._buckets.start = recording

    def take(self):
        r, self.ranges = self.ranges, []
        return r


def check_ranges(step, ranges, want_names, what):
    """Disjoint, inside the parameters (never the library's tail behind the last one; between tensors only the alignment gaps, which hold
    zeros), every float of the tensors `want_names` covered and no float of any other tensor."""
    end = max(o + k for o, k in step.offsets.values())
    cover = np.zeros(step.flat.numel(), np.int32)
    for first, count in ranges:
        assert count > 0 and first + count <= end, (what, first, count, end)
        cover[first:first + count] += 1
    assert cover.max() == 1, (what, "ranges overlap")
    named = np.zeros_like(cover)
    for name, (o, k) in step.offsets.items():
        named[o:o + k] = 1
        if name in want_names:
            assert cover[o:o + k].all(), (what, name, "not reported")
        else:
            assert not cover[o:o + k].any(), (what, name, "reported without a gradient")
    assert not cover[end:].any()
    stray = np.flatnonzero((cover == 1) & (named == 0))
    assert all(named[max(0, i - 3):i].any() and named[i + 1:i + 4].any() for i in stray), (what, "a range leaves the alignment gaps")


def update_piecewise(agent, obs, hidden, prev, masks, actions, li, mod):
    """evaluate_actions + ppo_loss + backward between the agent's own hooks -> the summed gradient is in step.grad afterwards."""
    step = agent.train_step
    out = step.evaluate_actions(obs, hidden, prev, masks, actions)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(step.dev)
    step.ppo_loss(t(li["old"]), t(li["adv"]), t(li["vp"]), t(li["ret"]), mod.CLIP, mod.VALUE_COEF, mod.ENTROPY_COEF, True)
    agent.before_backward(None)
    step.backward()
    agent.after_backward(None)
    torch.cuda.synchronize()
    return out


def to_dev(inp, dev, keys):
    M = inp["T"] * inp["N"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    obs = {k: t(inp[k]) for k in keys}
    obs[GOAL] = t(inp["goal"])
    return obs, t(inp["hidden"]), t(inp["prev"]).view(M, 1), t(inp["masks"]).view(M, 1), t(inp["actions"]).view(M, 1)


def make_agent(pol, mod, **kw):
    return DDPPO(pol, mod.CLIP, 1, 1, mod.VALUE_COEF, mod.ENTROPY_COEF, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM,
                 use_clipped_value_loss=True, use_normalized_advantage=False, **kw)


def case_mode(case, rank, world, dev):
    rgbd = case == "RGBD"
    mod, T_ = (Q, TQ) if rgbd else (R, TP)
    frames = ("rgb", "depth") if rgbd else ("depth",)
    ref = mod.reference(case)                                          # float64, the whole case
    pol = TQ.make_policy(case) if rgbd else TP.make_policy("B" if case == "B1" else case, dev)
    pol = pol.to(dev)
    if rank != 0:                                                      # rank 0's parameters and statistics must arrive by broadcast
        with torch.no_grad():
            for p in pol.parameters():
                p.add_(0.5)
            for b in pol.buffers():
                b.add_(1.0)
    agent = make_agent(pol, mod)
    step = agent.train_step
    agent.init_distributed()
    n = step.n_params
    # the gradient is compared up to the end of the last parameter: the library's tail (the padded stem's gradient, every rank's own,
    # never all-reduced, clipped or stepped) starts right behind it, inside the final alignment gap
    end = max(o + k for o, k in step.offsets.values())
    sd = mod.state_dict(case)
    for name, (o, k) in step.offsets.items():
        assert np.array_equal(step.flat[o:o + k].cpu().numpy(), np.asarray(sd[name], np.float32).reshape(-1)), (rank, name)
    if rgbd:
        assert all(not b.any() for b in TQ.buffers(pol).values())
    rec = Recorder(agent)
    inp = mod.rollout(case)
    mine, rows = shard(inp, rank, world, frames + ("goal", "prev", "masks", "actions"))
    li = {k: v[rows] for k, v in ref["loss_inputs"].items()}
    # ---- one backward: the ranges, the averaged gradient
    update_piecewise(agent, *to_dev(mine, dev, frames), li, mod)
    ranges = rec.take()
    check_ranges(step, ranges, set(step.offsets), f"{case}, encoder trains")
    assert ranges == agent.grad_ranges() == agent.grad_ranges(True, False), (rank, ranges, agent.grad_ranges())
    stem = step.offsets[ENCODER_PREFIX + "backbone.conv1.0.weight"]
    assert ranges[-1] == stem and ranges[0][0] == 0                    # early group first, the un-padded stem last
    grad = (step.grad[:n] * (1.0 / world)).cpu().double().numpy()      # the mean over the ranks (x 0.5: exact)
    errs = T_.grad_errors(step, grad, ref["grads"], f"{case}, rank {rank} of {world}")
    assert max(errs.values()) <= GRAD_TOL[case], sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    same_on_all_ranks(step.grad[:end], "summed gradient")
    if rgbd:
        TQ.assert_stats(TQ.stats_numpy(pol), ref["stats"], f"RGBD, rank {rank}, one call")
        assert float(TQ.buffers(pol)["_count"]) == inp["T"] * inp["N"]  # the frames of BOTH ranks
    # ---- before_step (mean + clip in one pass) + optimizer_step against float64 clip + Adam
    newp, norm, coef, _ = R.clip_and_adam(ref["params"], ref["grads"], lr=LR, eps=EPS, max_norm=MAX_GRAD_NORM)
    assert coef < 1.0                                                  # the clipping is live
    gnorm = agent.before_step()
    step.optimizer_step()
    torch.cuda.synchronize()
    assert abs(float(gnorm) - norm) < 1e-4 * norm, (float(gnorm), norm)
    worst = 0.0
    for name, (o, k) in step.offsets.items():
        g = ref["grads"][name]
        sel = (np.abs(g) > 1e-6 * max(np.abs(g).max(), 1e-30)).reshape(-1)
        got = step.flat[o:o + k].cpu().double().numpy()
        worst = max(worst, np.abs(got[sel] - newp[name].reshape(-1)[sel]).max(initial=0.0))
        np.testing.assert_allclose(got[sel], newp[name].reshape(-1)[sel], rtol=0, atol=STEP_ATOL[case], err_msg=name)
    print(f"[{case}, rank {rank}] worst parameter difference after mean + clip + Adam: {worst:.2e} (atol {STEP_ATOL[case]:.1e})")
    if rgbd:
        step.evaluate_actions(*to_dev(shard(Q.rollout(case, 1), rank, world, frames + ("goal", "prev", "masks", "actions"))[0], dev, frames))
        TQ.assert_stats(TQ.stats_numpy(pol), ref["stats2"], f"RGBD, rank {rank}, two calls")
        assert float(TQ.buffers(pol)["_count"]) == 2 * inp["T"] * inp["N"]
        for k, b in TQ.buffers(pol).items():
            same_on_all_ranks(b, k)
    for t, what in ((step.flat[:n], "parameters"), (step.exp_avg, "exp_avg"), (step.exp_avg_sq, "exp_avg_sq")):
        same_on_all_ranks(t, what)
    # ---- the flat schedule gives the bits of the bucketed one (a sum of two is the same sum in any chunking)
    if not rgbd:                                                       # (another evaluate would merge another batch into RGBD's statistics)
        got = {}
        for bucketed in (True, False):
            agent.bucketed = bucketed
            update_piecewise(agent, *to_dev(mine, dev, frames), li, mod)
            got[bucketed] = step.grad[:end].clone()
            assert bool(rec.take()) == bucketed
        agent.bucketed = True
        assert torch.equal(got[True], got[False]) and got[True].any()
    if case == "B1":
        partial_backwards(case, rank, world, dev, agent, rec, mine, li, ref)
    if not rgbd:                                                       # max_grad_norm None still averages
        update_piecewise(agent, *to_dev(mine, dev, frames), li, mod)
        summed = step.grad[:end].clone()
        step.max_grad_norm = None
        agent.before_step()
        torch.cuda.synchronize()
        assert torch.equal(step.grad[:end], summed * (1.0 / world)) and summed.any()
        step.max_grad_norm = MAX_GRAD_NORM


def partial_backwards(case, rank, world, dev, agent, rec, mine, li, ref):
    """The backwards in which the encoder has no gradient: after an evaluate from visual_features (features from this rank's own
    encoder), and with a frozen encoder (train_encoder False): every tensor but the encoder's is reported, the encoder's range is not
    and stays exactly zero."""
    step, pol = agent.train_step, agent.actor_critic
    others = {n for n in step.offsets if not n.startswith(ENCODER_PREFIX)}
    lo, hi = step.encoder_range
    obs, hidden, prev, masks, actions = to_dev(mine, dev, ("depth",))
    feats = pol.net.visual_encoder(obs)
    update_piecewise(agent, {"visual_features": feats, GOAL: obs[GOAL]}, hidden, prev, masks, actions, li, R)
    ranges = rec.take()
    check_ranges(step, ranges, others, "B1, visual_features")
    assert ranges == agent.grad_ranges() == agent.grad_ranges(True, True)
    end = max(o + k for o, k in step.offsets.values())
    assert not step.grad[lo:hi].any() and step.grad[:end].any()
    same_on_all_ranks(step.grad[:end], "gradient from visual_features")
    # a frozen encoder: a second policy, as a trainer freezes it before it builds the agent
    pol2 = TP.make_policy("B", dev)
    for name, p in pol2.named_parameters():
        if name.startswith(ENCODER_PREFIX):
            p.requires_grad_(False)
    frozen = make_agent(pol2, R)
    assert frozen.train_step.train_encoder is False
    frozen.init_distributed()
    rec2 = Recorder(frozen)
    update_piecewise(frozen, obs, hidden, prev, masks, actions, li, R)
    ranges = rec2.take()
    check_ranges(frozen.train_step, ranges, others, "B1, frozen encoder")
    assert ranges == frozen.grad_ranges() == frozen.grad_ranges(False, False)
    g = (frozen.train_step.grad[:frozen.train_step.n_params] * (1.0 / world)).cpu().double().numpy()
    assert not g[lo:hi].any()
    want = {k: (np.zeros_like(v) if k.startswith(R.ENC) else v) for k, v in ref["grads"].items()}
    errs = TP.grad_errors(frozen.train_step, g, want, f"B1, frozen encoder, rank {rank}")
    assert max(errs.values()) <= TP.GRAD_TOL, sorted(errs.items(), key=lambda kv: -kv[1])[:5]


def update_mode(rank, world, dev):
    c = Q.CASES["RGBD"]
    T, N, H, W, Hd = 3, 2, c["H"], c["W"], c["hidden"]
    pol = TQ.make_policy("RGBD").to(dev)
    S = pol.net.num_recurrent_layers
    agent = DDPPO(pol, Q.CLIP, 2, 1, Q.VALUE_COEF, Q.ENTROPY_COEF, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM,
                  use_clipped_value_loss=True, use_normalized_advantage=True)
    agent.init_distributed()
    space = TQ.Space({"depth": TQ.Box((H, W, 1)), "rgb": TQ.Box((H, W, 3)), GOAL: TQ.Box((2,))})
    st = RolloutStorage(T, N, space, TQ.ActionSpace(c["A"]), Hd, S, sensors=["rgb", "depth", GOAL])
    st.to(dev)
    steps = synth.make_policy_rgbd_inputs(H, W, N, T + 1, 91 + rank, c["A"])
    frame = lambda t: {"rgb": torch.from_numpy(steps[t][0]).float().to(dev), "depth": torch.from_numpy(steps[t][1]).to(dev),
                       GOAL: torch.from_numpy(steps[t][2]).to(dev)}
    for k, v in frame(0).items():
        st.observations[k][0].copy_(v)
    st.masks[0].zero_()
    n_steps = T if rank == 0 else T - 1                                # rank 1's rollout ended early (a pre-empted straggler)
    pol.eval()                                                         # the trainer collects in eval mode: no statistics, no collective
    for t in range(n_steps):
        obs = {k: v[st.step] for k, v in st.observations.items()}
        value, action, logp, hidden = pol.act(obs, st.recurrent_hidden_states[st.step], st.prev_actions[st.step], st.masks[st.step])
        rewards = torch.tensor([[0.25 * (t + 1) + rank], [-0.5 + 0.125 * t]])
        st.insert(frame(t + 1), hidden, action, logp, value, rewards, torch.from_numpy(steps[t + 1][4]).view(N, 1))
    obs = {k: v[st.step] for k, v in st.observations.items()}
    st.compute_returns(pol.get_value(obs, st.recurrent_hidden_states[st.step], st.prev_actions[st.step], st.masks[st.step]), True, 0.99, 0.95)
    pol.train()
    # ---- get_advantages, normalised over both ranks (equal sizes: the storage's T x N slots on every rank)
    adv = agent.get_advantages(st)
    raw = (st.returns[:-1] - st.value_preds[:-1]).cpu()
    parts = [torch.empty_like(raw) for _ in range(world)]
    dist.all_gather(parts, raw)
    both = torch.cat(parts).double().numpy()
    want = (raw.double().numpy() - both.mean()) / (both.std() + EPS_PPO)        # numpy's population std of the concatenation
    # float32 mean and variance of 2 x 6 values and the normalisation: a dozen roundings of values of this size
    tol = 16 * 2.0 ** -24 * max(1.0, np.abs(want).max()) * max(1.0, np.abs(both).max() / both.std())
    assert np.abs(adv.cpu().double().numpy() - want).max() <= tol, (np.abs(adv.cpu().double().numpy() - want).max(), tol)
    # ---- the whole update: M = 6 rows on rank 0, 4 on rank 1; the collectives do not depend on it
    step = agent.train_step
    before = step.flat[:step.n_params].clone()
    count0 = float(TQ.buffers(pol)["_count"])
    losses = agent.update(st)
    torch.cuda.synchronize()
    print(f"[update, rank {rank}] steps {n_steps}, losses {losses}")
    assert len(losses) == 3 and all(isinstance(x, float) and np.isfinite(x) for x in losses)
    assert step.step_count == 2 and not torch.equal(before, step.flat[:step.n_params])
    assert float(TQ.buffers(pol)["_count"]) == count0 + 2 * (T + T - 1) * N    # two epochs of every rank's rows, merged on both
    for t, what in ((step.flat[:step.n_params], "parameters"), (step.exp_avg, "exp_avg"), (step.exp_avg_sq, "exp_avg_sq")):
        same_on_all_ranks(t, what)
    for k, b in TQ.buffers(pol).items():
        assert torch.isfinite(b).all()
        same_on_all_ranks(b, k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["C", "B1", "RGBD", "update"])
    ap.add_argument("--shared-gpu", action="store_true")
    a = ap.parse_args()
    rank, world, lr = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ["LOCAL_RANK"])
    if a.shared_gpu:
        lr = 0
    torch.cuda.set_device(lr)
    dev = torch.device("cuda", lr)
    torch.set_num_threads(8)                                           # the float64 reference runs on the CPU, once per rank
    if a.shared_gpu:
        dist.init_process_group("gloo")
    else:
        dist.init_process_group("nccl", device_id=dev)
    assert world == 2
    if a.mode == "update":
        update_mode(rank, world, dev)
    else:
        case_mode(a.mode, rank, world, dev)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
