#!/usr/bin/env python
"""VO.OBS_TRANSFORM cost on the MI355X.

    python tools/bench_obs_transform.py                 # kernel + boundary figures, one JSON line each
    python tools/bench_obs_transform.py --kernel-only   # the kernel launches only (run under rocprofv3 --kernel-trace --stats)

Kernel: pnvo_resize_area on 8 / 32 / 256 frame pairs from a 640x360 sensor (rgb uint8 + depth float32 -> float32 rgb / depth pairs
at 341x192), 'resize' and 'resize_crop', timed with device events.  Bytes are computed from the shapes: the input rows and columns
the output windows touch, read once, plus the float32 outputs written; achieved bytes/s is set against the 6.3 TB/s achievable
HBM bandwidth.  Boundary: compute_local_delta_states_batch from 640x360 with 'resize' against the same call from 341x192 sensors
with no transform (wall clock per call, the host staging included)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointnav_vo_amd import model_spec as ms, synth  # noqa: E402
from pointnav_vo_amd.obs_transforms import DIV_CHANNELS_LAST, launch_resize, transformed_size  # noqa: E402
from pointnav_vo_amd.trainer import AttrDict, BaseRLTrainerWithVO  # noqa: E402

W, H = 341, 192
HS, WS = 360, 640
HBM = 6.3e12
DEV = torch.device("cuda", 0)


def kernel_bytes(n, geom):
    rs_h, rs_w, cy, cx, oh, ow = geom
    rows = ((cy + oh) * HS + rs_h - 1) // rs_h - (cy * HS) // rs_h
    cols = ((cx + ow) * WS + rs_w - 1) // rs_w - (cx * WS) // rs_w
    return 2 * n * (rows * cols * (3 + 4) + oh * ow * 4 * 4)


def bench_kernel(n, mode, iters=50):
    geom = transformed_size(HS, WS, mode, (W, H))
    rgb = torch.randint(0, 256, (2 * n, HS, WS, 3), dtype=torch.uint8, device=DEV)
    dep = torch.rand((2 * n, HS, WS), device=DEV)
    out_rgb = torch.empty((n, H, W, 6), device=DEV)
    out_dep = torch.empty((n, H, W, 2), device=DEV)

    def once():
        launch_resize(rgb.data_ptr(), torch.uint8, 2 * n, HS, WS, 3, (HS * WS * 3, WS * 3, 3), geom, out_rgb.data_ptr(), 2,
                      (H * W * 6, 3, W * 6, 6), DIV_CHANNELS_LAST, DEV)
        launch_resize(dep.data_ptr(), torch.float32, 2 * n, HS, WS, 1, (HS * WS, WS, 1), geom, out_dep.data_ptr(), 2,
                      (H * W * 2, 1, W * 2, 2), DIV_CHANNELS_LAST, DEV)
    for _ in range(5):
        once()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        once()
    b.record()
    b.synchronize()
    ms_ = a.elapsed_time(b) / iters
    by = kernel_bytes(n, geom)
    return dict(what="resize_kernel", mode=mode, pairs=n, ms_per_call=round(ms_, 4), bytes=by, gbps=round(by / ms_ / 1e6, 1),
                frac_of_6p3TBs=round(by / (ms_ * 1e-3) / HBM, 3), launches_per_call=2, timed_by="device events (measured)")


def make_trainer(obs_transform):
    cfg = AttrDict(
        VO=dict(VO_TYPE="REGRESS", OBS_TRANSFORM=obs_transform, VIS_SIZE_W=W, VIS_SIZE_H=H,
                REGRESS_MODEL=dict(name="vo_cnn_rgb_d_dd_top_down", visual_backbone="resnet18", hidden_size=512,
                                   visual_type=["rgb", "depth", "discretized_depth", "top_down_view"], dropout_p=0.2,
                                   discretize_depth="hard", discretized_depth_channels=10, regress_type="sep_act", mode="det",
                                   rnd_mode_n=10, pretrained=False)),
        TASK_CONFIG=dict(SIMULATOR=dict(DEPTH_SENSOR=dict(MIN_DEPTH=0.1, MAX_DEPTH=10.0, HFOV=70))))
    t = BaseRLTrainerWithVO(cfg, DEV)
    t._set_up_vo_obs_transformer()
    t._setup_vo_model(cfg)
    for k in t.vo_model:
        sd = synth.make_state_dict(ms.state_dict_spec(t.vo_model[k].cfg), seed=1)
        t.vo_model[k].load_state_dict({n: torch.from_numpy(np.array(v)) for n, v in sd.items()})
    return t


def bench_boundary(n, iters=20):
    res = {}
    for label, tr, (h, w) in (("resize_from_640x360", "resize", (HS, WS)), ("none_from_341x192", "none", (H, W))):
        t = make_trainer(tr)
        obs = [synth.make_raw_obs(h, w, seed=3, index=i, depth_fp16=False) for i in range(n + 1)]
        acts = [1 + i % 3 for i in range(n)]
        for _ in range(3):
            t.compute_local_delta_states_batch(obs[:n], obs[1:], acts)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            t.compute_local_delta_states_batch(obs[:n], obs[1:], acts)
        res[label] = round((time.perf_counter() - t0) / iters * 1e3, 3)
    return dict(what="boundary_batch_ms", pairs=n, timed_by="wall clock per call (measured)", **res)


def main():
    kernel_only = "--kernel-only" in sys.argv
    for n in (8, 32, 256):
        for mode in ("resize", "resize_crop"):
            print(json.dumps(bench_kernel(n, mode, iters=10 if kernel_only else 50)), flush=True)
    if kernel_only:
        return
    for n in (8, 32):
        print(json.dumps(bench_boundary(n)), flush=True)


if __name__ == "__main__":
    main()
