#!/usr/bin/env python
"""Per-step latency of the HIP baseline navigation policy (PointNavBaselinePolicy.act: SimpleCNN + GRU + heads) beside the same module
built from torch.nn in float32 with the same weights on the same GPU (torch eager).
    python tools/bench_baseline_policy.py [--envs 2 8 32] [--sizes 256x256 341x192] [--timed 20] [--hidden 512]
rgb-d frames (uint8 rgb, float32 depth), resident on the device before the clock starts; every call is timed on its own with HIP
events after 3 warm-up calls, and the median and the minimum over the timed calls are reported (ms).  Prints a table and one JSON line.
The Linear launch's time comes from a kernel trace in a run of its own (rocprofv3 --kernel-trace --stats -- python tools/... ;
kernel fc_splitk_kernel): `linear_weight_MB` is what that launch must read."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointnav_vo_amd import synth  # noqa: E402
from pointnav_vo_amd.baseline_policy import PointNavBaselinePolicy, baseline_state_dict_spec, simple_cnn_dims  # noqa: E402

GOAL = "pointgoal_with_gps_compass"
WARMUP = 3


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class Act:
    n = 4


class TorchBaseline(nn.Module):
    """The same computation from torch.nn (float32, eager): what a user of the reference runs on this GPU."""

    def __init__(self, H, W, hidden, sd):
        super().__init__()
        h, w = simple_cnn_dims(H, W)[-1]
        self.cnn = nn.Sequential(nn.Conv2d(4, 32, 8, 4), nn.ReLU(True), nn.Conv2d(32, 64, 4, 2), nn.ReLU(True), nn.Conv2d(64, 32, 3, 1),
                                 nn.Flatten(), nn.Linear(32 * h * w, hidden), nn.ReLU(True))
        self.rnn = nn.GRU(hidden + 2, hidden, 1)
        self.actor, self.critic = nn.Linear(hidden, Act.n), nn.Linear(hidden, 1)
        own = {"net.visual_encoder.cnn.": "cnn.", "net.state_encoder.rnn.": "rnn.", "action_distribution.linear.": "actor.", "critic.fc.": "critic."}
        mapped = {}
        for k, v in sd.items():
            pre = next(p for p in own if k.startswith(p))
            mapped[own[pre] + k[len(pre):]] = torch.from_numpy(np.array(v))
        self.load_state_dict(mapped)

    @torch.no_grad()
    def act(self, obs, hidden, prev_actions, masks):
        x = torch.cat([obs["rgb"].permute(0, 3, 1, 2) / 255.0, obs["depth"].permute(0, 3, 1, 2)], dim=1)
        x = torch.cat([self.cnn(x), obs[GOAL]], dim=1)
        x, hidden = self.rnn(x.unsqueeze(0), hidden * masks.unsqueeze(0))
        x = x.squeeze(0)
        logp_all = torch.log_softmax(self.actor(x), dim=-1)
        action = logp_all.exp().argmax(dim=-1, keepdim=True)
        return self.critic(x), action, logp_all.gather(-1, action), hidden


def time_calls(fn, timed):
    """[ms] of `timed` calls, each between two HIP events, after WARMUP untimed ones."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(timed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[2, 8, 32])
    ap.add_argument("--sizes", nargs="+", default=["256x256", "341x192"], help="frames as WxH")
    ap.add_argument("--timed", type=int, default=20)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--no-torch", action="store_true", help="time the HIP path alone (for a kernel trace)")
    a = ap.parse_args()
    assert a.timed >= 10, "at least 10 timed calls"
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    dev = torch.device("cuda", 0)
    res = {"metric": "baseline navigation-policy act() step, ms", "dtype": "f32", "visual": "rgb(uint8)+depth", "hidden": a.hidden,
           "warmup": WARMUP, "timed": a.timed, "results": []}
    for size in a.sizes:
        W, H = (int(v) for v in size.split("x"))
        space = Space({"rgb": Box((H, W, 3)), "depth": Box((H, W, 1)), GOAL: Box((2,))})
        sd = synth.make_state_dict(baseline_state_dict_spec(width=W, height=H, hidden=a.hidden), seed=0)
        pol = PointNavBaselinePolicy(space, Act(), GOAL, a.hidden)
        pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        pol = pol.to(dev).eval()
        ref = None if a.no_torch else TorchBaseline(H, W, a.hidden, sd).to(dev).eval()
        h, w = simple_cnn_dims(H, W)[-1]
        weight_mb = 32 * h * w * a.hidden * 4 / 1e6
        for B in a.envs:
            rgb, depth, goal, prev, _ = synth.make_policy_rgbd_inputs(H, W, B, 1, 1)[0]
            obs = {"rgb": torch.from_numpy(rgb).to(dev), "depth": torch.from_numpy(depth).to(dev), GOAL: torch.from_numpy(goal).to(dev)}
            hid = torch.full((1, B, a.hidden), 0.1, device=dev)
            pa, mk = torch.from_numpy(prev).view(B, 1).to(dev), torch.ones(B, 1, device=dev)
            row = {"size": size, "envs": B, "linear_weight_MB": weight_mb}
            hip = time_calls(lambda: pol.act(obs, hid, pa, mk, deterministic=True), a.timed)
            row["hip_ms_median"], row["hip_ms_min"] = float(np.median(hip)), float(np.min(hip))
            if ref is not None:
                fobs = dict(obs, rgb=obs["rgb"])                  # (torch divides the uint8 frame by 255.0 into float32 itself)
                tt = time_calls(lambda: ref.act(fobs, hid, pa, mk), a.timed)
                row["torch_ms_median"], row["torch_ms_min"] = float(np.median(tt)), float(np.min(tt))
                row["torch_over_hip"] = row["torch_ms_median"] / row["hip_ms_median"]
                v_h, a_h, _, h_h = pol.act(obs, hid, pa, mk, deterministic=True)
                v_t, a_t, _, h_t = ref.act(fobs, hid, pa, mk)
                row["max_abs_diff_hidden"] = float((h_h - h_t).abs().max())
                row["max_abs_diff_value"] = float((v_h - v_t).abs().max())
            res["results"].append(row)
        del pol, ref
    print("| frame | B | HIP ms (median / min) | torch eager ms (median / min) | torch / HIP |")
    print("|---|---|---|---|---|")
    for r in res["results"]:
        t = f"{r['torch_ms_median']:.3f} / {r['torch_ms_min']:.3f} | {r['torch_over_hip']:.2f}" if "torch_ms_median" in r else "- | -"
        print(f"| {r['size']} | {r['envs']} | {r['hip_ms_median']:.3f} / {r['hip_ms_min']:.3f} | {t} |")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
