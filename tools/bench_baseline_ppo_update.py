#!/usr/bin/env python3
"""One PPO minibatch update of the baseline navigation policy (PointNavBaselinePolicy: SimpleCNN + GRU), per phase, on the MI355X.

    python tools/bench_baseline_ppo_update.py [--frames 256x256 341x192] [--rows 5x1 128x1 128x2] [--iters 20] [--warmup 3]
                                               [--out profiles/baseline_ppo_update.json]

One update = evaluate_actions + ppo_loss + backward + clip_grad_norm + Adam + refresh on rgb-d uint8 frames, hidden 512.  Rows M = T x N:
5 x 1 is the reference's default plain-PPO minibatch (config/rl_config/default.py: num_steps 5, 16 environments in 16 minibatches);
128 x 1 and 128 x 2 are DD-PPO-sized rollouts.  The HIP path (pointnav_vo_amd.ppo.BaselineTrainStep) is timed as a whole with HIP events
on the stream, and per phase with the events the library records (pnvo_baseline_train_timing: encoder forward, GRU forward + heads,
loss, heads + BPTT + d embed, encoder backward) plus one pair around clip + Adam + refresh.

Beside it, in the same process on the same GPU, alternated run by run: the same module built from torch.nn in float32 eager with
autograd and torch.optim.Adam (Sequential convs and Linear, nn.GRU run over the segments between episode starts as the reference's
RNNStateEncoder does, the PPO loss lines, clip_grad_norm_), started from the same weights.  --warmup runs of each side first, then the
median of --iters; the spread is the wider of the two sides' p10 .. p90 ranges, and the HIP path counts as faster where the eager
median exceeds the HIP median by more than that spread.  Nothing here is a threshold: the record says which side wins.

At M = 5 the update is bound by traffic on the Linear's weight (51 MB at 341 x 192): the bytes counted below against the whole
update's time give the fraction of the HBM rate reached.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIDDEN, ACTIONS = 512, 4
CLIP, VALUE_COEF, ENTROPY_COEF, LR, EPS, MAX_GRAD_NORM = 0.2, 0.5, 0.01, 2.5e-4, 1e-5, 0.2
GOAL = "pointgoal_with_gps_compass"
HBM_PEAK = 8.0e12                                           # bytes / s, the specified rate
# passes over the Linear's weight in one update: forward read, dgrad read, wgrad write, clipping (1 read + 1 read-write), Adam (4 reads
# + 3 writes: parameter, gradient and two moments in, parameter and two moments out), the re-lay (1 read + 1 write)
WEIGHT_PASSES = {"forward read": 1, "dgrad read": 1, "wgrad write": 1, "clip": 3, "adam": 7, "re-lay": 2}


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class Act:
    def __init__(self, n):
        self.n = n


def make_batch(H, W, T, N, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    M = T * N
    masks = torch.ones(T, N)
    masks[0] = 0                                            # every rollout starts an episode ...
    if T > 16:
        for n in range(N):                                  # ... and each environment resets once more somewhere inside
            masks[int(torch.randint(8, T - 8, (1,), generator=g)), n] = 0
    b = dict(rgb=torch.randint(0, 256, (M, H, W, 3), generator=g, dtype=torch.uint8), depth=torch.rand(M, H, W, 1, generator=g),
             goal=torch.rand(M, 2, generator=g) * 3, prev=torch.zeros(M, 1, dtype=torch.int64), masks=masks.reshape(M, 1),
             actions=torch.randint(0, ACTIONS, (M, 1), generator=g), hidden=torch.rand(1, N, HIDDEN, generator=g) - 0.5,
             old=-1.386 + 0.2 * torch.randn(M, 1, generator=g), adv=torch.randn(M, 1, generator=g),
             vp=torch.randn(M, 1, generator=g) * 0.3)
    b["ret"] = b["vp"] + b["adv"]
    return {k: v.to(dev) for k, v in b.items()}


# ---------------------------------------------------------------------------------------------------------------- torch eager side
class _Holder(nn.Module):
    pass


class EagerBaseline(nn.Module):
    """PointNavBaselinePolicy from torch.nn, with the reference's parameter names (so the HIP policy's state_dict loads)."""

    def __init__(self, H, W, hidden):
        super().__init__()
        h, w = H, W
        for k, s in ((8, 4), (4, 2), (3, 1)):
            h, w = (h - k) // s + 1, (w - k) // s + 1
        self.net = _Holder()
        self.net.visual_encoder = _Holder()
        self.net.visual_encoder.cnn = nn.Sequential(nn.Conv2d(4, 32, 8, 4), nn.ReLU(True), nn.Conv2d(32, 64, 4, 2), nn.ReLU(True),
                                                    nn.Conv2d(64, 32, 3, 1), nn.Flatten(), nn.Linear(32 * h * w, hidden), nn.ReLU(True))
        self.net.state_encoder = _Holder()
        self.net.state_encoder.rnn = nn.GRU(hidden + 2, hidden, 1)
        self.action_distribution = _Holder()
        self.action_distribution.linear = nn.Linear(hidden, ACTIONS)
        self.critic = _Holder()
        self.critic.fc = nn.Linear(hidden, 1)

    def evaluate_actions(self, b, T, N):
        x = torch.cat([b["rgb"].float() / 255.0, b["depth"]], dim=3).permute(0, 3, 1, 2)
        x = torch.cat([self.net.visual_encoder.cnn(x), b["goal"]], dim=1).view(T, N, -1)
        masks = b["masks"].view(T, N)
        # RNNStateEncoder.seq_forward: one nn.GRU call per segment between steps at which any environment resets
        starts = [0] + (masks[1:] == 0).any(dim=1).nonzero().flatten().add(1).tolist() + [T]
        h, outs = b["hidden"], []
        for a, e in zip(starts[:-1], starts[1:]):
            o, h = self.net.state_encoder.rnn(x[a:e], h * masks[a].view(1, N, 1))
            outs.append(o)
        feat = torch.cat(outs).view(T * N, -1)
        logits = self.action_distribution.linear(feat)
        value = self.critic.fc(feat)
        lp = torch.log_softmax(logits, dim=-1)
        logp = lp.gather(-1, b["actions"])
        entropy = -(lp.exp() * lp).sum(-1).mean()
        return value, logp, entropy


def eager_update(model, opt, b, T, N):
    values, logp, entropy = model.evaluate_actions(b, T, N)
    ratio = torch.exp(logp - b["old"])
    surr1, surr2 = ratio * b["adv"], torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP) * b["adv"]
    action_loss = -torch.min(surr1, surr2).mean()
    vclip = b["vp"] + (values - b["vp"]).clamp(-CLIP, CLIP)
    value_loss = 0.5 * torch.max((values - b["ret"]).pow(2), (vclip - b["ret"]).pow(2)).mean()
    opt.zero_grad()
    (value_loss * VALUE_COEF + action_loss - entropy * ENTROPY_COEF).backward()
    nn.utils.clip_grad_norm_(model.parameters(), MAX_GRAD_NORM)
    opt.step()


# ---------------------------------------------------------------------------------------------------------------- HIP side
def hip_update(step, b, ev):
    obs = {"rgb": b["rgb"], "depth": b["depth"], GOAL: b["goal"]}
    step.evaluate_actions(obs, b["hidden"], b["prev"], b["masks"], b["actions"])
    step.ppo_loss(b["old"], b["adv"], b["vp"], b["ret"], CLIP, VALUE_COEF, ENTROPY_COEF, True)
    step.backward()
    ev[0].record()
    step.clip_grad_norm()
    step.optimizer_step()
    ev[1].record()


def timed(fn):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    e.record()
    e.synchronize()
    return a.elapsed_time(e)


def spread(xs):
    q = statistics.quantiles(xs, n=10)
    return q[-1] - q[0]


def run(H, W, T, N, iters, warmup, dev):
    from pointnav_vo_amd import PointNavBaselinePolicy
    from pointnav_vo_amd.ppo import BaselineTrainStep
    torch.manual_seed(0)
    space = Space({"rgb": Box((H, W, 3)), "depth": Box((H, W, 1)), GOAL: Box((2,))})
    pol = PointNavBaselinePolicy(space, Act(ACTIONS), GOAL, HIDDEN)
    eager = EagerBaseline(H, W, HIDDEN)
    eager.load_state_dict(pol.state_dict())                 # the same weights on both sides
    eager = eager.to(dev)
    opt = torch.optim.Adam(eager.parameters(), lr=LR, eps=EPS)
    pol = pol.to(dev)
    step = BaselineTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    step.timing(True)
    b = make_batch(H, W, T, N, dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    hip, eag, phases = [], [], []
    for i in range(warmup + iters):                         # alternated: both sides see the same neighbours on the machine
        th = timed(lambda: hip_update(step, b, ev))
        te = timed(lambda: eager_update(eager, opt, b, T, N))
        if i >= warmup:
            hip.append(th)
            eag.append(te)
            phases.append(dict(step.phase_ms(), clip_adam_refresh=ev[0].elapsed_time(ev[1])))
    med = {k: statistics.median(p[k] for p in phases) for k in phases[0]}
    sp = max(spread(hip), spread(eag))
    F = step.offsets["net.visual_encoder.cnn.6.weight"][1]
    rec = dict(frame=f"{W}x{H}", T=T, N=N, M=T * N, hip_ms=statistics.median(hip), eager_ms=statistics.median(eag),
               hip_p10_p90=spread(hip), eager_p10_p90=spread(eag), spread_ms=sp, phases_ms=med,
               hip_faster_beyond_spread=statistics.median(eag) - statistics.median(hip) > sp,
               linear_weight_bytes=4 * F)
    if T * N <= 8:                                          # the weight-traffic bound of the small minibatch
        passes = sum(WEIGHT_PASSES.values())
        rec["weight_traffic_bytes"] = passes * 4 * F
        rec["weight_traffic_passes"] = WEIGHT_PASSES
        rec["hbm_fraction_of_8TBps"] = passes * 4 * F / (rec["hip_ms"] * 1e-3) / HBM_PEAK
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", nargs="+", default=["256x256", "341x192"], help="WxH")
    ap.add_argument("--rows", nargs="+", default=["5x1", "128x1", "128x2"], help="TxN")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool needs the MI355X"
    dev = torch.device("cuda", 0)
    out = []
    for fr in a.frames:
        W, H = (int(v) for v in fr.split("x"))
        for rw in a.rows:
            T, N = (int(v) for v in rw.split("x"))
            rec = run(H, W, T, N, a.iters, a.warmup, dev)
            out.append(rec)
            ph = "  ".join(f"{k} {v:.3f}" for k, v in rec["phases_ms"].items())
            print(f"{rec['frame']:8s} M = {rec['M']:3d} (T {T}, N {N}): HIP {rec['hip_ms']:.3f} ms  eager {rec['eager_ms']:.3f} ms  "
                  f"spread {rec['spread_ms']:.3f} ms  HIP faster beyond the spread: {rec['hip_faster_beyond_spread']}", flush=True)
            print(f"         phases (ms): {ph}", flush=True)
            if "hbm_fraction_of_8TBps" in rec:
                print(f"         Linear weight traffic counted {rec['weight_traffic_bytes'] / 1e6:.0f} MB -> "
                      f"{100 * rec['hbm_fraction_of_8TBps']:.1f} % of 8 TB/s over the whole update", flush=True)
            torch.cuda.empty_cache()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
