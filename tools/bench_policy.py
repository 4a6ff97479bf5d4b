#!/usr/bin/env python
"""Per-step latency / throughput of the HIP navigation policy (PointNavResNetPolicy.act)
at the batch sizes a nav loop uses (B = environments per process), with the oracle port timed beside it.
    python tools/bench_policy.py [--envs 1 4 16 64] [--rnn {LSTM,GRU}] [--visual-types depth | rgb depth | rgb] [--rgb-dtype {uint8,float32}]
                                 [--backbone NAME] [--encode-frames N]
--backbone: any of model_spec.BACKBONES (resnet50 .. se_resneXt101; no oracle port of them: the CPU baseline is skipped).
--encode-frames N also times net.visual_encoder on N frames (the frozen-encoder collection's call shape).
--rnn GRU times the GRU state encoder instead (no oracle port of it: the CPU baseline is skipped).
--visual-types with rgb builds the policy as the reference trainers do (normalize_visual_inputs on, ddppo_trainer.py:118-132) and runs it
in training mode, as PPOTrainer's collection does: every act merges its batch into RunningMeanAndVar's buffers.  The input stage is
then also timed on its own with HIP events (pnvo_policy_input_stage): pool only, pool + moments fused (what act runs), and the
two-launch form (pool, then the moments from the pooled tensor), with the bandwidth against its algorithmic bytes (frames read once,
pooled tensor written once) and its share of the step."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointnav_vo_amd import _lib, synth  # noqa: E402
from pointnav_vo_amd.policy import PointNavResNetPolicy, policy_state_dict_spec  # noqa: E402

H, W = 192, 341


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class Act:
    n = 4


def input_stage(pol, obs, vis, B, dev, step_ms, reps=200):
    """HIP-event time of the input stage alone: {form: {us, GB/s against the algorithmic bytes, share of the step}}."""
    C_in = (3 if "rgb" in vis else 0) + (1 if "depth" in vis else 0)
    rgb, depth = obs.get("rgb"), obs.get("depth")
    pooled = torch.empty((B, H // 2, W // 2, 2 * C_in), device=dev)
    m12 = torch.zeros(2 * C_in, device=dev, dtype=torch.float64)
    center = pol.net.visual_encoder.running_mean_and_var._mean.reshape(-1).clone()
    nbytes = B * H * W * ((3 * rgb.element_size() if rgb is not None else 0) + (4 if depth is not None else 0)) + pooled.numel() * 4
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = {"algorithmic_bytes": nbytes}
    for mode, name in ((0, "pool_only"), (1, "fused_pool_moments"), (2, "two_launch_pool_then_moments")):
        call = lambda: _lib.check(_lib.lib.pnvo_policy_input_stage(pol._handle, p(rgb), int(rgb is not None and rgb.dtype == torch.uint8),
                                                                   p(depth), p(center), mode, B, p(pooled), p(m12), stream))
        for _ in range(10):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        e1.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / reps
        out[name] = {"us": us, "GB_per_s": nbytes / us * 1e-3, "share_of_step": us * 1e-3 / step_ms}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--rnn", choices=["LSTM", "GRU"], default="LSTM")
    ap.add_argument("--visual-types", nargs="+", choices=["rgb", "depth"], default=["depth"])
    ap.add_argument("--rgb-dtype", choices=["uint8", "float32"], default="uint8")
    ap.add_argument("--backbone", default="resnet18")
    ap.add_argument("--encode-frames", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    vis = [k for k in ("rgb", "depth") if k in a.visual_types]
    plain = vis == ["depth"]
    space = Space({"depth": Box((H, W, 1)), "rgb": Box((H, W, 3)), "pointgoal_with_gps_compass": Box((2,))})
    pol = PointNavResNetPolicy(observation_space=space, action_space=Act(), hidden_size=512, rnn_type=a.rnn,
                               num_recurrent_layers=2, backbone=a.backbone, vis_types=vis, normalize_visual_inputs=not plain)
    kw = {} if plain else dict(vis_types=tuple(vis), normalize_visual_inputs=True)
    kw["backbone"] = a.backbone
    sd = synth.make_state_dict(policy_state_dict_spec(width=W, height=H, rnn_type=a.rnn, **kw), seed=0)
    pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    pol = pol.to(dev).train(not plain)
    res = {"metric": "navigation-policy act() steps", "frame": f"{W}x{H} {'+'.join(vis)}", "dtype": "f32", "results": []}
    if a.rnn != "LSTM":
        res["rnn"] = a.rnn
    if a.backbone != "resnet18":
        res["backbone"] = a.backbone
    if not plain:
        res["rgb_dtype"], res["mode"] = a.rgb_dtype, "training (statistics updated at every act)"
    for B in a.envs:
        if plain:
            depth, goal, prev, mask = synth.make_policy_inputs(H, W, B, 1, 1)[0]
            obs = {"depth": torch.from_numpy(depth).to(dev)}
        else:
            rgb, depth, goal, prev, mask = synth.make_policy_rgbd_inputs(H, W, B, 1, 1)[0]
            rgb = torch.from_numpy(rgb)
            frames = {"rgb": (rgb if a.rgb_dtype == "uint8" else rgb.float()).to(dev), "depth": torch.from_numpy(depth).to(dev)}
            obs = {k: frames[k] for k in vis}
        obs["pointgoal_with_gps_compass"] = torch.from_numpy(goal).to(dev)
        hid = torch.zeros(pol.num_recurrent_layers, B, 512, device=dev)
        pa, mk = torch.from_numpy(prev).view(B, 1).to(dev), torch.ones(B, 1, device=dev)
        for _ in range(5):
            _, _, _, hid = pol.act(obs, hid, pa, mk, deterministic=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            _, act, _, hid = pol.act(obs, hid, pa, mk, deterministic=True)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        row = {"envs": B, "ms_per_step": dt * 1e3, "frames_per_s": B / dt}
        if not plain:
            row["input_stage"] = input_stage(pol, obs, vis, B, dev, dt * 1e3)
        res["results"].append(row)
    if a.encode_frames > 0:
        n = a.encode_frames
        frames = {k: (torch.from_numpy(synth.uniform(3, k, (n, H, W, 1), 0.0, 1.0).astype(np.float32)) if k == "depth" else
                      torch.from_numpy((synth.bits(3, k, n * H * W * 3) % np.uint64(256)).astype(np.uint8).reshape(n, H, W, 3))).to(dev)
                  for k in vis}
        enc = pol.net.visual_encoder
        for _ in range(3):
            enc(frames)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reps = max(3, a.steps // 5)
        for _ in range(reps):
            enc(frames)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        res["visual_encoder"] = {"frames": n, "ms": dt * 1e3, "frames_per_s": n / dt}
    if not a.no_cpu_baseline and a.rnn == "LSTM" and a.backbone == "resnet18":
        from oracle import oracle, policy_oracle
        B = 4
        depth, goal, prev, mask = synth.make_policy_inputs(H, W, B, 1, 1)[0]
        hid = np.zeros((4, B, 512), np.float32)
        policy_oracle.policy_step(sd, depth, goal, prev, mask, hid, dtype=np.float32)
        t0 = time.perf_counter()
        n = 3
        for _ in range(n):
            policy_oracle.policy_step(sd, depth, goal, prev, mask, hid, dtype=np.float32)
        dt = (time.perf_counter() - t0) / n
        res["cpu_baseline"] = {"envs": B, "ms_per_step": dt * 1e3, "frames_per_s": B / dt, "kind": "port",
                               "cores": oracle.usable_cores() if hasattr(oracle, "usable_cores") else None}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
