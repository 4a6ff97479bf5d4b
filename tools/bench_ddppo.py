#!/usr/bin/env python3
"""What one box can measure of the data-parallel PPO update (pointnav_vo_amd.ddppo): a functional record, not evidence of overlap.

    python tools/bench_ddppo.py --clip [--world 2] [--iters 50]
        pnvo_policy_clip_grad_norm_scaled(1 / world) against `grad /= world` followed by pnvo_policy_clip_grad_norm on the same
        gradient buffer (the policy at the reference's sizes): median of HIP-event timings.
    python -m torch.distributed.run --nproc-per-node 2 tools/bench_ddppo.py --ranks [--shared-gpu] [--steps 128] [--n 2] [--iters 12]
        one DDPPO minibatch update per rank (T = 128, N environments per rank, 341 x 192 depth, hidden 512, 2-layer LSTM) with the
        bucketed and with the flat all-reduce schedule: medians of backward + all-reduce wait, mean + clip + Adam, the whole update.
        --shared-gpu: both ranks on cuda:0 over gloo (collectives through the host: says nothing about exposed time over xGMI).
Prints one JSON line (rank 0).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_ppo_update as B  # noqa: E402   (the shapes, the batch and the event timer of the single-process bench)


def make_policy(dev):
    from pointnav_vo_amd.policy import PointNavResNetPolicy

    class Box:
        def __init__(self, shape):
            self.shape = shape

    class Space:
        def __init__(self, d):
            self.spaces = d

    class Act:
        n = B.ACTIONS

    torch.manual_seed(0)
    return PointNavResNetPolicy(observation_space=Space({"depth": Box((B.H, B.W, 1)), B.GOAL: Box((2,))}), action_space=Act(),
                                hidden_size=B.HIDDEN, num_recurrent_layers=B.LAYERS, backbone="resnet18", normalize_visual_inputs=False,
                                obs_transform=None, vis_types=["depth"]).to(dev)


def bench_clip(a, dev):
    from pointnav_vo_amd import _lib
    from pointnav_vo_amd.ppo import PolicyTrainStep
    pol = make_policy(dev)
    step = PolicyTrainStep(pol, lr=B.LR, eps=B.EPS, max_grad_norm=B.MAX_GRAD_NORM)
    n = step.n_params
    g0 = torch.randn(n, device=dev) * 1e-2
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    norm = C.c_void_p(step._norm.data_ptr())
    tm = B.Timer()
    for _ in range(a.warmup + a.iters):
        step.grad[:n].copy_(g0)
        with tm.span("scaled clip"):
            _lib.check(_lib.lib.pnvo_policy_clip_grad_norm_scaled(pol._handle, 1.0 / a.world, B.MAX_GRAD_NORM, norm, stream))
        step.grad[:n].copy_(g0)
        with tm.span("grad /= world, then clip"):
            step.grad /= a.world
            _lib.check(_lib.lib.pnvo_policy_clip_grad_norm(pol._handle, B.MAX_GRAD_NORM, norm, stream))
    return dict(tm.medians(a.warmup), floats=n, world=a.world)


def bench_ranks(a, dev):
    from pointnav_vo_amd.ddppo import DDPPO
    pol = make_policy(dev)
    agent = DDPPO(pol, B.CLIP, 1, 1, B.VALUE_COEF, B.ENTROPY_COEF, lr=B.LR, eps=B.EPS, max_grad_norm=B.MAX_GRAD_NORM)
    agent.init_distributed()
    step = agent.train_step
    b = B.make_batch(a.steps, a.n, dev, seed=dist.get_rank())
    obs = {B.GOAL: b["goal"], "depth": b["depth"]}
    out = {"all_reduces_per_backward": [c * 4 for _, c in agent.grad_ranges(True, False)]}
    for bucketed in (True, False):
        agent.bucketed = bucketed
        tm = B.Timer()
        for _ in range(a.warmup + a.iters):
            with tm.span("whole update"):
                step.evaluate_actions(obs, b["hidden"], b["prev"], b["masks"], b["actions"])
                step.ppo_loss(b["old"], b["adv"], b["vp"], b["ret"], B.CLIP, B.VALUE_COEF, B.ENTROPY_COEF, True)
                with tm.span("backward + all-reduce"):
                    agent.before_backward(None)
                    step.backward()
                    agent.after_backward(None)
                with tm.span("mean + clip + Adam + refresh"):
                    agent.before_step()
                    step.optimizer_step()
        out["bucketed" if bucketed else "flat"] = tm.medians(a.warmup)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clip", action="store_true")
    ap.add_argument("--ranks", action="store_true")
    ap.add_argument("--shared-gpu", action="store_true")
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--n", type=int, default=2)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ddppo.py measures on an MI355X: no GPU here, nothing measured")
    if a.iters < 10:
        raise SystemExit("--iters must be at least 10 (median of >= 10 timed iterations)")
    if a.ranks:
        lr = 0 if a.shared_gpu else int(os.environ["LOCAL_RANK"])
        torch.cuda.set_device(lr)
        dev = torch.device("cuda", lr)
        if a.shared_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
        rec = {"ranks": dist.get_world_size(), "backend": "gloo, one shared GPU" if a.shared_gpu else "nccl", "T": a.steps, "N": a.n,
               **bench_ranks(a, dev)}
        if dist.get_rank() == 0:
            print(json.dumps(rec))
        dist.barrier()
        dist.destroy_process_group()
    else:
        print(json.dumps({"clip": bench_clip(a, torch.device("cuda", 0))}))


if __name__ == "__main__":
    main()
