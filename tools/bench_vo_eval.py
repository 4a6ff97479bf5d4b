#!/usr/bin/env python
"""Time of a VO evaluation pass (pointnav_vo_amd.evaluate.GeoInvarianceEvalStep; reference: VOCNNRegressionGeometricInvarianceEngine.eval,
pointnav_vo/vo/engine/vo_cnn_regression_geo_invariance_engine.py:1020-1257): 64 entries per batch (EVAL_BATCHSIZE) over the three
separate action models at 341x192, "inverse_joint_train" layout.

Two forms of the same pass, in alternating runs of one process:

    metrics    step() per batch (forwards, pnvo_vo_metrics, pnvo_geo_inverse_loss, totals on the device), result() at the end
    forwards   the forwards alone: per action model index_select, eval forward, predictions put back in batch order; one
               synchronisation at the end — what the package could do before the evaluation step existed

Each timed pass is a host clock around `--batches` batches that ends in a device synchronisation.  Prints one JSON line.
    python tools/bench_vo_eval.py [--batches 20] [--rounds 6] [--entries 64]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointnav_vo_amd import model_spec as ms, synth  # noqa: E402
from pointnav_vo_amd import vo_cnn  # noqa: E402,F401
from pointnav_vo_amd.evaluate import GeoInvarianceEvalStep  # noqa: E402
from pointnav_vo_amd.registry import baseline_registry  # noqa: E402

W, H = 341, 192
SPACE = ["rgb", "depth", "discretized_depth", "top_down_view"]
F, L, R = 1, 2, 3
NO_NOISE = {F: (0.0, -0.25, 0.0), L: (0.0, 0.0, np.radians(10.0)), R: (0.0, 0.0, -np.radians(10.0))}


def build_models(dev):
    models = {}
    for act in (F, L, R):
        m = baseline_registry.get_vo_model("vo_cnn_rgb_d_dd_top_down")(
            observation_space=SPACE, observation_size=(W, H), hidden_size=512, backbone="resnet18", normalize_visual_inputs=True,
            output_dim=3, dropout_p=0.2, discretized_depth_channels=10)
        sd = synth.make_state_dict(ms.state_dict_spec(m.cfg), seed=act)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        models[act] = m.to(dev).eval()
    return models


def make_batch(entries, seed, dev):
    """The joint layout: entries / 2 samples, each followed by its prev_rel_to_cur entry (a turn's with the opposite action)."""
    rng = np.random.RandomState(seed)
    acts = rng.choice([F, L, R], entries // 2)
    opp = {F: F, L: R, R: L}
    actions = np.array([x for a in acts for x in (a, opp[int(a)])], np.int64)
    dtypes = np.tile(np.array([0, 1], np.int64), entries // 2)
    base = synth.make_obs_pairs(8, H, W, observation_space=SPACE, dd_bins=10, seed=seed)      # 8 distinct pairs, repeated
    obs = {k: torch.from_numpy(v).to(dev).repeat((entries + 7) // 8, 1, 1, 1)[:entries].contiguous() for k, v in base.items()}
    targets = (np.array([NO_NOISE[int(a)] for a in actions]) + 1e-2 * rng.standard_normal((entries, 3))).astype(np.float32)
    mask = (rng.uniform(size=entries) < 0.7).astype(np.float32)
    return dict(obs=obs, actions=torch.from_numpy(actions), data_types=torch.from_numpy(dtypes), targets=torch.from_numpy(targets),
                mask=torch.from_numpy(mask))


def pass_metrics(ev, batches, n):
    ev.reset()
    for i in range(n):
        b = batches[i % len(batches)]
        ev.step(b["obs"], b["actions"], b["data_types"], b["targets"], dz_regress_masks=b["mask"])
    return ev.result()


def pass_forwards(models, batches, n, dev):
    with torch.no_grad():
        for i in range(n):
            b = batches[i % len(batches)]
            preds = torch.zeros((b["actions"].numel(), 3), device=dev)
            for act, model in models.items():
                idx = torch.nonzero(b["actions"] == act, as_tuple=True)[0]
                if idx.numel() == 0:
                    continue
                di = idx.pin_memory().to(dev, non_blocking=True)
                preds.index_copy_(0, di, model({k: v.index_select(0, di) for k, v in b["obs"].items()}))
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--entries", type=int, default=64)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vo_eval.py needs the MI355X"
    dev = torch.device("cuda", 0)
    models = build_models(dev)
    batches = [make_batch(a.entries, 100 + k, dev) for k in range(2)]
    ev = GeoInvarianceEvalStep(models, ("inverse_joint_train",), loss_inv_weight=1.0)
    for _ in range(2):                                   # warm both forms at the timed shapes
        res = pass_metrics(ev, batches, len(batches))
        pass_forwards(models, batches, len(batches), dev)
    times = {"metrics": [], "forwards": []}
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = pass_metrics(ev, batches, a.batches)
        times["metrics"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        pass_forwards(models, batches, a.batches, dev)
        times["forwards"].append((time.perf_counter() - t0) * 1e3)
    out = {"metric": "VO evaluation pass, three action models, inverse_joint_train", "frame": f"{W}x{H}", "dtype": "f32",
           "entries_per_batch": a.entries, "batches_per_pass": a.batches, "rounds": a.rounds, "unit": "ms per pass"}
    for k, v in times.items():
        out[k] = {"mean": float(np.mean(v)), "min": float(np.min(v)), "max": float(np.max(v)), "runs": [round(x, 3) for x in v],
                  "ms_per_batch": float(np.mean(v)) / a.batches}
    out["difference_ms_per_batch"] = out["metrics"]["ms_per_batch"] - out["forwards"]["ms_per_batch"]
    out["objective"] = res["objective"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
