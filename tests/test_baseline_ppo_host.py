"""CPU: the float64 restatement of the baseline policy's PPO minibatch update (tests/baseline_ppo_reference.py), which the GPU tests
compare with, against the outputs recorded from the imported reference's own evaluate_actions, loss lines and backward
(tests/golden/baseline_ppo_*.npz, written by tests/golden/gen_golden_baseline_ppo.py); the branch census of the loss seeds; and the
float32 restatement's distance from the float64 one against the GPU test's tolerances."""
import os
import sys

import numpy as np
import pytest

import baseline_ppo_reference as P
from conftest import load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from gen_golden_baseline_ppo import GOLDEN_CASES, sample_index  # noqa: E402  (which entries the fixture keeps)

REL = 1e-9
TOL, LOSS_TOL, GRAD_TOL, STEP_ATOL = 2e-4, 1e-4, 7.55e-4, 7.94e-7     # tests/test_gpu_baseline_ppo.py's


def rel(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_restatement_matches_the_reference_update(case):
    rec = load_golden(f"baseline_ppo_{case}.npz")
    c = P.CASES[case]
    assert (int(rec["weight_seed"]), int(rec["input_seed"]), int(rec["loss_seed"])) == (c["wseed"], c["iseed"], P.LOSS_SEED[case])
    ref = P.reference(case)
    for k in ("value", "logp", "hidden"):
        assert rel(ref[k], rec[k + "64"]) < REL, (case, k, rel(ref[k], rec[k + "64"]))
    assert abs(ref["entropy"] - float(rec["entropy64"])) < REL * abs(float(rec["entropy64"]))
    for g, w in zip(ref["losses"], rec["losses64"]):
        assert abs(g - w) < REL * max(abs(w), 1e-300), (case, g, w)
    names = [str(n) for n in rec["grad_names"]]
    assert names == [n for n, _ in P.spec(case)]
    for n in names:
        g = ref["grads"][n].reshape(-1)
        norm = float(rec[f"grad_norm64/{n}"])
        assert norm > 0 and abs(np.linalg.norm(g) - norm) < REL * norm, (case, n)
        want = rec[f"grad_sample64/{n}"]
        assert np.abs(g[sample_index(g.size)] - want).max() < REL * np.abs(g).max(), (case, n)


@pytest.mark.parametrize("case", list(P.CASES))
def test_every_branch_of_both_losses_is_taken(case):
    """From the float64 side alone: at least one row in the clipped and one in the unclipped branch of the surrogate and of the value
    loss, both signs of the advantage, and no row within 1e-6 of a branch boundary."""
    ref = P.reference(case)
    s, v, margin = P.branch_census(ref["value"], ref["logp"], ref["loss_inputs"])
    assert margin.min() > 1e-6, (case, margin.min())
    adv = ref["loss_inputs"]["adv"]
    assert (adv > 0).any() and (adv < 0).any()
    assert min(int(s.sum()), int((~s).sum()), int(v.sum()), int((~v).sum())) >= 1, (case, s, v)


def test_float32_restatement_stays_inside_a_tenth_of_the_gpu_tolerances():
    tab = P.float32_error_table()
    for case, r in tab.items():
        worst = max(r["grads"], key=r["grads"].get)
        print(f"[{case}] gradients {r['grads'][worst]:.3e} ({worst}), forward {r['forward']:.2e}, losses {r['loss']:.2e}, step {r['step']:.2e}")
        assert r["forward"] <= TOL / 10 and r["loss"] <= LOSS_TOL / 10, (case, r["forward"], r["loss"])
        assert r["grads"][worst] <= GRAD_TOL / 10, (case, worst, r["grads"][worst])
        assert r["step"] <= STEP_ATOL / 10, (case, r["step"])

