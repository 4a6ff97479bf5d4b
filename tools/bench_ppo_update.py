#!/usr/bin/env python3
"""One PPO minibatch update of the navigation policy at the reference's shape, per phase, on the MI355X.

    python tools/bench_ppo_update.py [--n 2 4] [--steps 128] [--iters 12] [--warmup 3] [--out profiles/ppo_update.md] [--no-eager]
                                      [--rnn {LSTM,GRU}] [--visual-types depth | rgb depth | rgb] [--rgb-dtype {uint8,float32}]

Shape: configs/rl/ddppo_pointnav.yaml — num_steps T = 128, N environments per minibatch, 341 x 192 depth, hidden 512, 2-layer LSTM,
train_encoder.  The HIP path (pointnav_vo_amd.ppo.PolicyTrainStep) is timed per phase with HIP events recorded inside the library
(pnvo_policy_train_timing: encoder forward, LSTM forward + heads, loss, heads + BPTT + embeddings backward, encoder backward) and
with torch events around clip + Adam + refresh and around the whole update; medians over --iters after --warmup.

Beside it, in the same run on the same GPU: the same update in plain torch eager ops with autograd (an nn.Module restatement of the
policy with random weights: GroupNorm-ResNet18 encoder, nn.LSTM run over the segments between episode starts as the reference's
RNNStateEncoder does, Categorical heads, the PPO loss, clip_grad_norm_, torch.optim.Adam).  It is the only comparison there is: the
project could not do this update at all before.  No threshold: the record says which side wins, phase by phase.
--rnn GRU runs both sides with the GRU state encoder (state [LAYERS, N, HIDDEN]); the phase keys keep their names.
--visual-types with rgb times the HIP path alone on an rgb / rgb-d policy built as the reference trainers build it
(normalize_visual_inputs on) in training mode: the encoder-forward phase then holds the input stage (rgb / 255, pool, the batch
moments) and RunningMeanAndVar's update; --rgb-dtype says how the minibatch holds rgb (float32 is what RolloutStorage hands out).

    python tools/bench_ppo_update.py --static-encoder [--n 2 8] [--out profiles/static_encoder.md]

The frozen encoder (RL.DDPPO.train_encoder False) two ways, in one process on one GPU, on the same rollout and the same policy, the two
updates alternating iteration by iteration: frames in (observations['depth'], train_encoder=False: the encoder's train-mode forward runs
over all T * N frames and the backward stops behind visual_fc) against features in (observations['visual_features'], computed once by
policy.net.visual_encoder: visual_fc's GEMM is all that is left of the encoder).  Then one full recurrent_generator pass (two minibatches
of N environments each, every tensor gathered, waited for) of a RolloutStorage holding frames against one holding features only.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, HIDDEN, LAYERS, ACTIONS = 192, 341, 512, 2, 4
CLIP, VALUE_COEF, ENTROPY_COEF, LR, EPS, MAX_GRAD_NORM = 0.2, 0.5, 0.01, 2.5e-4, 1e-5, 0.2
GOAL = "pointgoal_with_gps_compass"


def make_batch(T, N, dev, seed=0, rnn="LSTM"):
    g = torch.Generator().manual_seed(seed)
    M = T * N
    masks = torch.ones(T, N)
    masks[0] = 0                                            # every rollout starts an episode ...
    for n in range(N):                                      # ... and each environment resets once more somewhere inside
        masks[int(torch.randint(8, T - 8, (1,), generator=g)), n] = 0
    b = dict(depth=torch.rand(M, H, W, 1, generator=g), goal=torch.rand(M, 2, generator=g) * 3,
             prev=torch.randint(0, ACTIONS, (M, 1), generator=g), masks=masks.reshape(M, 1),
             actions=torch.randint(0, ACTIONS, (M, 1), generator=g), hidden=torch.rand(2 * LAYERS, N, HIDDEN, generator=g) - 0.5,       # a GRU keeps the h blocks
             old=-1.386 + 0.2 * torch.randn(M, 1, generator=g), adv=torch.randn(M, 1, generator=g),
             vp=torch.randn(M, 1, generator=g) * 0.3)
    b["ret"] = b["vp"] + b["adv"]
    if rnn == "GRU":
        b["hidden"] = b["hidden"][:LAYERS].contiguous()
    return {k: v.to(dev) for k, v in b.items()}


class Timer:
    def __init__(self):
        self.t = {}

    def span(self, name):
        timer = self

        class _S:
            def __enter__(s):
                s.a, s.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.a.record()

            def __exit__(s, *exc):
                s.b.record()
                timer.t.setdefault(name, []).append((s.a, s.b))
        return _S()

    def medians(self, skip):
        torch.cuda.synchronize()
        return {k: statistics.median([a.elapsed_time(b) for a, b in v][skip:]) for k, v in self.t.items()}


# ---------------------------------------------------------------------------------------------------------------- HIP path
def bench_hip(T, N, iters, warmup, dev, rnn="LSTM", visual_types=("depth",), rgb_dtype="uint8"):
    from pointnav_vo_amd.policy import PointNavResNetPolicy
    from pointnav_vo_amd.ppo import PolicyTrainStep

    class Box:
        def __init__(self, shape):
            self.shape = shape

    class Space:
        def __init__(self, d):
            self.spaces = d

    class Act:
        n = ACTIONS

    torch.manual_seed(0)
    vis = [k for k in ("rgb", "depth") if k in visual_types]
    plain = vis == ["depth"]
    pol = PointNavResNetPolicy(observation_space=Space({"depth": Box((H, W, 1)), "rgb": Box((H, W, 3)), GOAL: Box((2,))}),
                               action_space=Act(), hidden_size=HIDDEN, num_recurrent_layers=LAYERS, rnn_type=rnn, backbone="resnet18",
                               normalize_visual_inputs=not plain, obs_transform=None, vis_types=vis).to(dev)
    pol.train(not plain)
    step = PolicyTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    step.timing(True)
    b = make_batch(T, N, dev, rnn=rnn)
    obs = {GOAL: b["goal"]}
    if "depth" in vis:
        obs["depth"] = b["depth"]
    if "rgb" in vis:
        rgb = torch.randint(0, 256, (T * N, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
        obs["rgb"] = (rgb if rgb_dtype == "uint8" else rgb.float()).to(dev)
    tm, phases = Timer(), []
    for _ in range(warmup + iters):
        with tm.span("whole update"):
            step.evaluate_actions(obs, b["hidden"], b["prev"], b["masks"], b["actions"])
            step.ppo_loss(b["old"], b["adv"], b["vp"], b["ret"], CLIP, VALUE_COEF, ENTROPY_COEF, True)
            step.backward()
            with tm.span("clip + Adam + refresh"):
                step.clip_grad_norm()
                step.optimizer_step()
        phases.append(step.phase_ms())
    out = {k: statistics.median([p[k] for p in phases[warmup:]]) for k in phases[0]}
    out.update(tm.medians(warmup))
    return out


# ---------------------------------------------------------------------------------------------------------------- frozen encoder
def bench_static_encoder(T, N, iters, warmup, dev, rnn="LSTM"):
    from pointnav_vo_amd.policy import FEATURES_KEY, PointNavResNetPolicy
    from pointnav_vo_amd.ppo import PolicyTrainStep
    from pointnav_vo_amd.rollout_storage import RolloutStorage

    class Box:
        def __init__(self, shape):
            self.shape = shape

    class Space:
        def __init__(self, d):
            self.spaces = d

    class ActionSpace:
        n = ACTIONS

    torch.manual_seed(0)
    pol = PointNavResNetPolicy(observation_space=Space({"depth": Box((H, W, 1)), GOAL: Box((2,))}), action_space=ActionSpace(),
                               hidden_size=HIDDEN, num_recurrent_layers=LAYERS, rnn_type=rnn, backbone="resnet18",
                               normalize_visual_inputs=False, obs_transform=None, vis_types=["depth"]).to(dev)
    enc = pol.net.visual_encoder
    step = PolicyTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM, train_encoder=False)
    step.timing(True)
    b = make_batch(T, N, dev, rnn=rnn)
    tm = Timer()
    for _ in range(2):                                          # the first pass grows the workspaces; the second is the figure
        with tm.span("encode"):
            feats = torch.cat([enc({"depth": b["depth"][i:i + 64]}) for i in range(0, T * N, 64)])
    inputs = {"frames": {"depth": b["depth"], GOAL: b["goal"]}, "features": {FEATURES_KEY: feats, GOAL: b["goal"]}}
    phases = {"frames": [], "features": []}
    for _ in range(warmup + iters):
        for kind, obs in inputs.items():                        # alternating: both see the same machine state
            with tm.span(kind + ": whole update"):
                step.evaluate_actions(obs, b["hidden"], b["prev"], b["masks"], b["actions"])
                step.ppo_loss(b["old"], b["adv"], b["vp"], b["ret"], CLIP, VALUE_COEF, ENTROPY_COEF, True)
                step.backward()
                with tm.span(kind + ": clip + Adam + refresh"):
                    step.clip_grad_norm()
                    step.optimizer_step()
            phases[kind].append(step.phase_ms())
    out = {kind: {k: statistics.median([p[k] for p in ph[warmup:]]) for k in ph[0]} for kind, ph in phases.items()}
    # ---- the generator pass: 2 N environments, two minibatches
    envs = 2 * N
    S = (2 if rnn == "LSTM" else 1) * LAYERS
    space = Space({"depth": Box((H, W, 1)), FEATURES_KEY: Box(tuple(enc.output_shape)), GOAL: Box((2,))})
    adv = torch.zeros(T, envs, 1, device=dev)
    stored = {}
    for kind, sensor in (("frames", "depth"), ("features", FEATURES_KEY)):
        st = RolloutStorage(T, envs, space, ActionSpace(), HIDDEN, S, sensors=[sensor, GOAL])
        st.to(dev)
        st.observations[sensor].uniform_()
        st.step = T
        stored[kind] = sum(v.numel() * 4 for v in st.observations.values())
        for _ in range(warmup + iters):
            with tm.span(kind + ": generator pass"):
                for sample in st.recurrent_generator(adv, 2):
                    pass
        del st
        torch.cuda.empty_cache()
    torch.cuda.synchronize()
    for kind in inputs:
        for k in ("whole update", "clip + Adam + refresh", "generator pass"):
            out[kind][k] = statistics.median([x.elapsed_time(y) for x, y in tm.t[f"{kind}: {k}"]][warmup:])
        out[kind]["stored observation MB"] = stored[kind] / 1e6
    out["encode_ms"] = tm.t["encode"][1][0].elapsed_time(tm.t["encode"][1][1])
    return out


STATIC_ORDER = ["encoder_forward", "lstm_forward", "loss", "bptt", "encoder_backward", "clip + Adam + refresh", "whole update",
                               "generator pass", "stored observation MB"]


def static_encoder_report(a, dev):
    lines = ["# Frozen-encoder PPO update: frames in against features in", "",
             f"`tools/bench_ppo_update.py --static-encoder`: T = {a.steps}, 341 x 192 depth, hidden 512, 2-layer {a.rnn}, 4 actions, "
             f"train_encoder False; median of {a.iters} iterations after {a.warmup} warm-up, HIP events, one process, one policy and one "
             f"rollout for both columns, the two updates alternating, {torch.cuda.get_device_name(0)}.  Milliseconds unless named otherwise.",
             "", "frames in: `observations['depth']` (the encoder's train-mode forward over all T * N frames, the backward stops behind "
             "visual_fc).  features in: `observations['visual_features']` from `policy.net.visual_encoder` (visual_fc's GEMM is what "
             "`encoder forward` holds, its backward what `encoder backward` holds).  generator pass: one `recurrent_generator` pass "
             "over 2 N environments in two minibatches of a storage that holds the frames, or the features only.", ""]
    record = {}
    for N in a.n:
        r = bench_static_encoder(a.steps, N, a.iters, a.warmup, dev, a.rnn)
        torch.cuda.empty_cache()
        record[f"N={N}"] = r
        lines += [f"## N = {N}  (M = {a.steps * N} rows per minibatch)", "", "| phase | frames in | features in | frames / features |",
                  "|---|---:|---:|---:|"]
        for k in STATIC_ORDER:
            f, g = r["frames"][k], r["features"][k]
            lines.append(f"| {LABEL.get(k, k).replace('LSTM', a.rnn)} | {f:.3f} | {g:.3f} | {f / g if g > 0 else float('nan'):.2f} |")
        ok = r["features"]["whole update"] <= r["frames"]["whole update"]
        lines += ["", f"Encoding the {a.steps * N} frames (in batches of 64, once, not part of either update; a trainer encodes N frames per "
                  f"rollout step instead): {r['encode_ms']:.3f} ms.",
                  f"Whole update, features in at or below frames in: {'yes' if ok else 'NO - to be explained'}.", ""]
    return lines, record


# ---------------------------------------------------------------------------------------------------------------- eager torch
def gn_conv(cin, cout, k, stride, groups):
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride, k // 2, bias=False), nn.GroupNorm(groups, cout))


class Block(nn.Module):
    def __init__(self, cin, cout, stride, groups):
        super().__init__()
        self.a, self.b = gn_conv(cin, cout, 3, stride, groups), gn_conv(cout, cout, 3, 1, groups)
        self.ds = gn_conv(cin, cout, 1, stride, groups) if (stride != 1 or cin != cout) else None

    def forward(self, x):
        r = x if self.ds is None else self.ds(x)
        return F.relu(self.b(F.relu(self.a(x))) + r)


class EagerPolicy(nn.Module):
    """The depth-only resnet18 + LSTM (or GRU) policy (baseplanes 32, GroupNorm of baseplanes / 2 groups, 2048-float compression)."""

    def __init__(self, rnn="LSTM"):
        super().__init__()
        self.gru = rnn == "GRU"
        bp, g = 32, 16
        self.stem = gn_conv(1, bp, 7, 2, g)
        blocks, cin = [], bp
        for li in range(4):
            for bi in range(2):
                cout = bp << li
                blocks.append(Block(cin, cout, 2 if (li > 0 and bi == 0) else 1, g))
                cin = cout
        self.blocks = nn.Sequential(*blocks)
        h, w = H // 2, W // 2
        for _ in range(5):
            h, w = (h + 1) // 2, (w + 1) // 2
        comp = int(round(2048 / (h * w)))
        self.comp = nn.Sequential(nn.Conv2d(cin, comp, 3, 1, 1, bias=False), nn.GroupNorm(1, comp))
        self.fc = nn.Linear(comp * h * w, HIDDEN)
        self.tgt = nn.Linear(3, 32)
        self.emb = nn.Embedding(ACTIONS + 1, 32)
        self.rnn = getattr(nn, rnn)(HIDDEN + 64, HIDDEN, LAYERS)
        self.actor, self.critic = nn.Linear(HIDDEN, ACTIONS), nn.Linear(HIDDEN, 1)

    def encode(self, depth):
        x = F.avg_pool2d(depth.permute(0, 3, 1, 2), 2)
        x = F.max_pool2d(F.relu(self.stem(x)), 3, 2, 1)
        x = F.relu(self.comp(self.blocks(x)))
        return F.relu(self.fc(x.flatten(1)))

    def recur(self, visual, b, T, N):
        goal, masks = b["goal"], b["masks"].view(T, N)
        g3 = torch.stack([goal[:, 0], torch.cos(-goal[:, 1]), torch.sin(-goal[:, 1])], -1)
        idx = ((b["prev"].float() + 1) * b["masks"]).long().squeeze(-1)
        x = torch.cat([visual, self.tgt(g3), self.emb(idx)], 1).view(T, N, -1)
        h, c = b["hidden"][:LAYERS], b["hidden"][LAYERS:]
        state = h if self.gru else (h, c)
        starts = sorted(set([0] + (masks == 0).any(1).nonzero().flatten().tolist() + [T]))   # segments between episode starts
        outs = []
        for s, e in zip(starts[:-1], starts[1:]):
            m = masks[s].view(1, N, 1)
            o, state = self.rnn(x[s:e], state * m if self.gru else (state[0] * m, state[1] * m))
            outs.append(o)
        feat = torch.cat(outs).view(T * N, -1)
        dist = torch.distributions.Categorical(logits=self.actor(feat))
        return self.critic(feat), dist.log_prob(b["actions"].squeeze(-1)).unsqueeze(-1), dist.entropy().mean()


def bench_eager(T, N, iters, warmup, dev, rnn="LSTM"):
    torch.manual_seed(0)
    pol = EagerPolicy(rnn).to(dev)
    opt = torch.optim.Adam(pol.parameters(), lr=LR, eps=EPS)
    b = make_batch(T, N, dev, rnn=rnn)
    tm = Timer()
    for _ in range(warmup + iters):
        with tm.span("whole update"):
            with tm.span("encoder_forward"):
                visual = pol.encode(b["depth"])
            vis = visual.detach().requires_grad_(True)
            with tm.span("lstm_forward"):
                value, logp, entropy = pol.recur(vis, b, T, N)
            with tm.span("loss"):
                ratio = torch.exp(logp - b["old"])
                action_loss = -torch.min(ratio * b["adv"], torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * b["adv"]).mean()
                vclip = b["vp"] + (value - b["vp"]).clamp(-CLIP, CLIP)
                value_loss = 0.5 * torch.max((value - b["ret"]).pow(2), (vclip - b["ret"]).pow(2)).mean()
                total = value_loss * VALUE_COEF + action_loss - entropy * ENTROPY_COEF
            opt.zero_grad()
            with tm.span("bptt"):
                total.backward()
            with tm.span("encoder_backward"):
                visual.backward(vis.grad)
            with tm.span("clip + Adam + refresh"):
                nn.utils.clip_grad_norm_(pol.parameters(), MAX_GRAD_NORM)
                opt.step()
    return tm.medians(warmup)


ORDER = ["encoder_forward", "lstm_forward", "loss", "bptt", "encoder_backward", "clip + Adam + refresh", "whole update"]
LABEL = {"encoder_forward": "encoder forward", "lstm_forward": "LSTM forward + heads", "loss": "loss",
         "bptt": "heads + BPTT + embeddings backward", "encoder_backward": "encoder backward",
         "clip + Adam + refresh": "clip + Adam (+ operand refresh)", "whole update": "whole update (host-timed, events)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--rnn", choices=["LSTM", "GRU"], default="LSTM")
    ap.add_argument("--static-encoder", action="store_true", help="frozen encoder: frames in against features in (see the docstring)")
    ap.add_argument("--visual-types", nargs="+", choices=["rgb", "depth"], default=["depth"])
    ap.add_argument("--rgb-dtype", choices=["uint8", "float32"], default="uint8")
    a = ap.parse_args()
    with_rgb = "rgb" in a.visual_types
    if with_rgb and a.static_encoder:
        raise SystemExit("--static-encoder measures the depth-only policy")
    if not torch.cuda.is_available():
        raise SystemExit("bench_ppo_update.py measures on an MI355X: no GPU here, nothing measured")
    if a.iters < 10:
        raise SystemExit("--iters must be at least 10 (median of >= 10 timed iterations)")
    dev = torch.device("cuda", 0)
    if a.static_encoder:
        lines, record = static_encoder_report(a, dev)
        finish(a, lines, record)
        return
    lines = ["# PPO minibatch update of the navigation policy: HIP path vs torch eager", "",
             f"`tools/bench_ppo_update.py`: T = {a.steps}, 341 x 192 {' + '.join(k for k in ('rgb', 'depth') if k in a.visual_types)}"
             f"{' (rgb as ' + a.rgb_dtype + ', normalize_visual_inputs, training mode)' if with_rgb else ''}, hidden 512, 2-layer {a.rnn}, "
             "4 actions, train_encoder; "
             f"median of {a.iters} iterations after {a.warmup} warm-up, HIP events, one process, {torch.cuda.get_device_name(0)}.",
             f"The eager column is the same update in torch-ROCm eager ops with autograd (nn.{a.rnn} over the segments between episode "
             "starts, as the reference's RNNStateEncoder), random weights.  Milliseconds.", ""]
    record = {}
    for N in a.n:
        hip = bench_hip(a.steps, N, a.iters, a.warmup, dev, a.rnn, a.visual_types, a.rgb_dtype)
        torch.cuda.empty_cache()
        eager = None
        if not a.no_eager and not with_rgb:                            # (the eager restatement is the depth-only policy)
            try:
                eager = bench_eager(a.steps, N, a.iters, a.warmup, dev, a.rnn)
            except Exception as e:                                    # the record then says so instead of a number
                eager = {"error": f"{type(e).__name__}: {e}"}
            torch.cuda.empty_cache()
        record[f"N={N}"] = {"hip": hip, "eager": eager}
        lines += [f"## N = {N}  (M = {a.steps * N} frames)", "", "| phase | HIP path | torch eager | eager / HIP |", "|---|---:|---:|---:|"]
        for k in ORDER:
            e = eager.get(k) if eager and "error" not in eager else None
            lines.append(f"| {LABEL[k].replace('LSTM', a.rnn)} | {hip[k]:.3f} | {'%.3f' % e if e is not None else 'not measured'} | "
                         f"{'%.2f' % (e / hip[k]) if e is not None else '-'} |")
        if eager and "error" in eager:
            lines += ["", f"torch eager failed: `{eager['error']}`"]
        lines.append("")
    finish(a, lines, record)


def finish(a, lines, record):
    text = "\n".join(lines)
    print(text)
    print(json.dumps(record))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
