"""GPU (-m gpu): the Adam kernel through the C ABI (`_lib.lib.pnvo_adam_step`) against torch.optim.Adam in float64 over WHOLE
trajectories — 40 steps (5 at a million elements), from step 1 and resumed at step 5001 from non-zero moments — where every other
optimiser check of the suite is a first step from zero moments, on which m / sqrt(v) = sign(g) whatever the kernel does with beta1,
beta2, the bias corrections or the accumulation.

Reference and criterion: tests/adam_reference.py (the real torch.optim.Adam on the CPU in float64, and in float32 as the yardstick:
err <= margin * d32 + floor, margins 4 / 8 / 3 for parameters / exp_avg / exp_avg_sq).  Per case: the parameters after EVERY step,
both moments after the last one, the gradient buffer and all guard floats around the four buffers bit-unchanged (64 sentinel floats
either side; the pointers start 0, 1 or 3 floats into the payload area: real ranges start at 4-float alignment, the frozen-encoder
split wherever a tensor ends).

Cases.  n = 4099 (16 blocks and a 3-element tail): every gradient class x betas (0.9, 0.999) and (0.5, 0.9) — a hard-coded default
fails the second — x eps 1e-8 (VO) and 1e-5 (PPO) x parameters from zero and from N(0,1) x first step 1 and 5001.  Parameters of
magnitude 1 hide the update's own rounding (one ulp of 1 is 5e-4 lr), the ones from zero do not.  n = 1, 255, 256, 257 (less than a
block, one short, exact, one over) x the three pointer shifts x both first steps, and n = 1 000 003 (3907 blocks), with `normal`.

What the kernel was before this module (b1 m + (1.f - b1) g, b2 v + (1.f - b2) g^2, lr / bc1 in float32, the bias corrections from
the float betas), on the MI355X, err / d32 against the bounds 4 / 8 / 3 (most cases with the default betas failed):
    exp_avg_sq, betas (0.9, 0.999)   38 - 48 in every class from step 1 (22 in zero_after_3, 39 resumed in `wide`), 142 at a million
                                     elements after 5 steps: err 1.26e-5 relative where torch's float32 run has 3.3e-7
    parameters from zero, resumed    13 - 175 (0.999f^5001 is not 0.999^5001: sqrt(bc2) off by 2e-7); 1.2 - 1.6 from step 1
    exp_avg                          2.8 - 6.4; 98 and 25 with one element
    betas (0.5, 0.9)                 all within the bounds (both complements are exact in float32) but `alternating` from zero
The cause is not the float32 subtraction (1.f - 0.999f is exact) but the float 0.999f itself: (float)(1.0 - (double)0.999f) is the
same 0.99998713e-3.  launch_adam now takes lr and the betas as the decimals their caller wrote and rounds every derived constant once.
Measured now, worst err / d32 per quantity over all 123 cases (d32 of the parameters: the largest so far in the trajectory):
    parameters 3.31 (alternating, betas (0.5, 0.9), eps 1e-8, from zero, resumed at 5001)   exp_avg 1.00   exp_avg_sq 1.03
    — the moments are torch's float32 ones to the last bit or two, the parameters bit-equal to torch's float32 run on a CPU without
    AVX-512 in `alternating` (see adam_reference.py on the two torch trajectories).
Mutations of the kernel, each run once against this module: beta2 = 0.99 in the kernel, eps under the square root, exp_avg_sq
overwritten instead of accumulated: 123 of 124 tests fail each; bias corrections from step - 1: 85 fail (every run from step 1, and the resumed ones that start from zero with the default betas); a grid
of n / 256 blocks: 117 fail (all but n = 256).
Wall time of the module on the MI355X host: 5.1 s for the 124 tests (the first one pays 2 s of start-up).
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import adam_reference as A
from pointnav_vo_amd import _lib

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GUARD = 64
SENTINEL = 0x7FC0BEEF                      # a quiet NaN with a payload: a kernel that reads a guard as data poisons its output
LR = 2.5e-4
BETAS = ((0.9, 0.999), (0.5, 0.9))
EPS = (1e-8, 1e-5)
SHIFTS = (0, 1, 3)
WORST = A.Worst()
PNVO_ERR_ARG = -1                          # include/pnvo.h


def guarded(payload, lo, rows=None):
    """A device buffer of GUARD + n + GUARD floats ([rows, ...] of them) filled with the sentinel, `payload` at float offset lo."""
    n = payload.shape[-1]
    shape = (GUARD + n + GUARD,) if rows is None else (rows, GUARD + n + GUARD)
    buf = torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    buf[..., lo:lo + n] = torch.from_numpy(np.array(payload, dtype=np.float32)).to(DEV)
    return buf


def guards_intact(buf, lo, n):
    bits = buf.view(torch.int32)
    return bool((bits[..., :lo] == SENTINEL).all()) and bool((bits[..., lo + n:] == SENTINEL).all())


def run_kernel(g, init, lr, betas, eps, first_step, shift):
    """T calls of pnvo_adam_step on guarded buffers -> (params after every step [T, n], exp_avg [n], exp_avg_sq [n]) as float64,
    after the bit checks on the gradient buffer and the guards."""
    T, n = g.shape
    lo = GUARD + shift
    total = GUARD + n + GUARD
    P, M, V = (guarded(a, lo) for a in init)
    G = guarded(g, lo, rows=T)                               # one guarded gradient buffer per step
    G0 = G.view(torch.int32).clone()
    rec = torch.empty((T, n), dtype=torch.float32, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    at = lambda buf, off=0: C.c_void_p(buf.data_ptr() + 4 * (off + lo))
    for t in range(T):
        _lib.check(_lib.lib.pnvo_adam_step(at(P), at(G, t * total), at(M), at(V), n, lr, betas[0], betas[1], eps, first_step + t, stream))
        rec[t].copy_(P[lo:lo + n])
    torch.cuda.synchronize()
    assert torch.equal(G.view(torch.int32), G0), "the gradient buffer (or a guard around it) was written"
    for name, buf in (("params", P), ("exp_avg", M), ("exp_avg_sq", V)):
        assert guards_intact(buf, lo, n), f"a guard float around {name} was written"
    return rec.cpu().double().numpy(), M[lo:lo + n].cpu().double().numpy(), V[lo:lo + n].cpu().double().numpy()


def run_case(kind, n, T, betas, eps, start, first_step, shift):
    g, init, ref64, ref32 = A.reference(kind, n, T, LR, betas, eps, start, first_step)
    got_p, got_m, got_v = run_kernel(g, init, LR, betas, eps, first_step, shift)
    what = f"{kind} n={n} betas={betas} eps={eps:g} p0={start} step {first_step}.. shift {shift}"
    bad = A.check_trajectory(what, got_p, got_m, got_v, ref64, ref32, WORST)
    print("worst err/d32 so far:", WORST)
    assert not bad, bad[:6]
    return got_p, ref64


FULL = [(k, b, e, s, f) for k, b, e, s, f in itertools.product(A.CLASSES, BETAS, EPS, ("zero", "normal"), (1, 5001))]


@pytest.mark.parametrize("idx", range(len(FULL)), ids=[f"{k}-b{b[0]}_{b[1]}-eps{e:g}-{s}-from{f}" for k, b, e, s, f in FULL])
def test_trajectory_of_4099_elements_follows_fp64_adam(idx):
    kind, betas, eps, start, first_step = FULL[idx]
    got_p, ref64 = run_case(kind, 4099, 40, betas, eps, start, first_step, SHIFTS[idx % 3])
    if kind == "zero_after_3":
        # The gradient is exactly zero from the fourth step on: the moments decay and are still applied, every step.  Wherever the
        # float64 step is larger than two float32 ulps of the parameter the kernel's parameter must have moved; with the default betas
        # (m / sqrt(v) decays as 0.9^t / 0.999^(t/2): 2 % of lr is left after 40 steps) that is nearly every element up to the last step.
        for t in range(3, got_p.shape[0]):
            before, after = ref64[0][t - 1], ref64[0][t]
            must_move = np.abs(after - before) > 2 * np.spacing(np.abs(before).astype(np.float32)).astype(np.float64)
            assert (got_p[t] != got_p[t - 1])[must_move].all(), t + 1
            if betas == BETAS[0] or t == 3:
                assert must_move.mean() > 0.9, (t + 1, float(must_move.mean()))


@pytest.mark.parametrize("first_step", [1, 5001])
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_sizes_around_one_block(n, shift, first_step):
    run_case("normal", n, 40, BETAS[0], EPS[0], "zero", first_step, shift)


@pytest.mark.parametrize("shift", SHIFTS)
def test_a_million_elements(shift):
    run_case("normal", 1_000_003, 5, BETAS[0], EPS[0], "zero", 1, shift)


def test_bad_arguments_are_refused_before_anything_is_launched():
    n = 257
    bufs = [guarded(np.full(n, 0.5 + i, np.float32), GUARD) for i in range(4)]
    before = [b.view(torch.int32).clone() for b in bufs]
    ptr = [C.c_void_p(b.data_ptr() + 4 * GUARD) for b in bufs]
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    args = (n, LR, 0.9, 0.999, 1e-8)
    assert _lib.lib.pnvo_adam_step(*ptr, *args, 0, stream) == PNVO_ERR_ARG          # steps count from 1
    for k in range(4):
        p = list(ptr)
        p[k] = None
        assert _lib.lib.pnvo_adam_step(*p, *args, 1, stream) == PNVO_ERR_ARG, k
    torch.cuda.synchronize()
    assert all(torch.equal(b.view(torch.int32), b0) for b, b0 in zip(bufs, before))
