#!/usr/bin/env python3
"""CPU-only companion of tests/test_gpu_ppo.py: the figures its header quotes, from the reference model alone.

    python tools/ppo_grad_error_table.py            per-tensor relative L2 deviation of the float32 run of tests/ppo_reference.py from
                                                    its float64 self, cases A-C (GRAD_TOL = 10 x the worst), and the same for the
                                                    parameters after clip + Adam
    python tools/ppo_grad_error_table.py --seeds    the smallest loss-input seed per case whose branch census meets the test
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ppo_reference as R  # noqa: E402


def census_ok(case, s, v, margin, need=1e-6):
    if (margin <= need).any():
        return False
    if case == "A":      # every cell of {surrogate clipped, not} x {value clipped, not} holds two elements
        return all(int((s == a)[v == b].sum()) >= 2 for a in (True, False) for b in (True, False))
    return min(int(s.sum()), int((~s).sum()), int(v.sum()), int((~v).sum())) >= 2   # M = 4 / 6: two per branch of each clamp


def seeds():
    import torch
    for case in R.CASES:
        with torch.no_grad():
            v, lp = (t.numpy() for t in R.forward(R.leaves(R.state_dict(case), torch.float64), R.rollout(case), torch.float64)[:2])
        for seed in range(1000):
            li = R.loss_inputs(case, v, lp, seed=seed)
            s, vc, margin = R.branch_census(v, lp, li)
            if census_ok(case, s, vc, margin, need=1e-4):      # the test asks for 1e-6; keep well clear of it
                print(case, "seed", seed, "surrogate clipped", int(s.sum()), "value clipped", int(vc.sum()), "of", len(s),
                      "min margin %.2e" % margin.min())
                break


def table():
    worst = 0.0
    for case in R.CASES:
        for use_clipped in (True, False):
            r64, r32 = R.reference(case, "float64", use_clipped), R.reference(case, "float32", use_clipped)
            errs = {k: np.linalg.norm(r32["grads"][k] - g) / max(np.linalg.norm(g), 1e-12) for k, g in r64["grads"].items()}
            k = max(errs, key=errs.get)
            worst = max(worst, errs[k])
            print(f"case {case} clipped_value={use_clipped}: float32 vs float64 gradient, worst tensor {errs[k]:.2e} ({k}), "
                  f"median {np.median(list(errs.values())):.2e}; losses {np.abs(np.array(r32['losses']) - np.array(r64['losses'])).max():.1e}")
    print(f"worst over the cases: {worst:.2e}  ->  GRAD_TOL = 10 x = {10 * worst:.1e}")


if __name__ == "__main__":
    seeds() if "--seeds" in sys.argv else table()
