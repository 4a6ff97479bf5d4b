"""CPU reference of the optimiser for tests/test_gpu_adam.py and tests/test_gpu_optimizer_steps.py (TEST INFRASTRUCTURE ONLY).

Three things, each in one place:

  grads(kind, T, n)      deterministic gradient sequences [T, n] float32 (numpy default_rng) for the regimes in which an Adam kernel can
                         go wrong: `normal` 1e-2 N(0,1); `tiny` 1e-8 N(0,1), where eps rules the denominator; `zero_after_3` N(0,1) for
                         three steps and exactly 0 from then on (the moments decay, the parameters keep moving); `sparse` 90 % exact zeros
                         per step; `wide` magnitudes 10^U(-12, 4) of either sign; `alternating` +-1e-3, the sign flipping with the step.
  trajectory(...)        parameters and both moments after EVERY step, from the real torch.optim.Adam on the CPU in float64 or float32;
                         a run that starts at step > 1 loads {step, exp_avg, exp_avg_sq} through Adam.load_state_dict, as a resumed
                         checkpoint does.  restatement_error() pins oracle.torch_train_ref.adam_step — the restatement every other
                         optimiser test goes through — to it (tests/test_adam_reference_host.py: 1e-12).
  close(...)             the one criterion: err = |got - ref64| against margin * d32 + floor, d32 = |ref32 - ref64| the deviation of
                         torch's own float32 Adam on the same gradients.  Max norm for the parameters, relative L2 for the moments.

                             quantity      margin   floor
                             parameters    4        one float32 ulp of max |p| (*)
                             exp_avg       8        2^-23 relative
                             exp_avg_sq    3        2^-23 relative

                         The margins: a plain float32 evaluation of b1 m + (1 - b1) g, b2 v + (1 - b2) g^2,
                         p - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps) with the complements rounded once from double sits at up to 2.1
                         (parameters), 4.9 (exp_avg: torch's lerp_ rounds differently) and 1.0 (exp_avg_sq) times torch's own float32
                         deviation over 40 steps (numpy, on the CPU); the project's usual 3 is kept where it fits.  The yardstick is
                         torch in float32, never the code under test.
                         (*) Over a trajectory both terms are taken UP TO the step that is compared, not of that step alone: the
                         largest |p| of the float64 trajectory so far, and the largest d32 so far.  Rounding errors stay in a parameter:
                         one committed while it was large is still there when it has come back towards zero, and the error of a float32
                         run is a random walk, not a monotone curve.  `alternating` from zero shows why: every element has the same
                         |g|, so d32 is ONE sample, it dips to 1e-12 (0.03 ulp of the step) at single steps, and where it dips depends
                         on the CPU that runs torch — the float32 trajectories of torch with and without AVX-512 lie 2 ulp of a step
                         apart (5.8e-11) from the fourth step on, so that either one fails a bound built from the other's d32 of that
                         step alone.  The HIP kernel is bit-equal to the one without.
"""
import functools

import numpy as np
import torch

from oracle import torch_train_ref as ttr

CLASSES = ("normal", "tiny", "zero_after_3", "sparse", "wide", "alternating")
MARGIN = {"param": 4.0, "exp_avg": 8.0, "exp_avg_sq": 3.0}
ULP32 = 2.0 ** -23


def grads(kind, T, n, seed=0):
    """[T, n] float32 of class `kind`; the same (kind, T, n, seed) always gives the same numbers."""
    rng = np.random.default_rng([seed, CLASSES.index(kind), T, n])
    z = rng.standard_normal((T, n))
    if kind == "normal":
        g = 1e-2 * z
    elif kind == "tiny":
        g = 1e-8 * z
    elif kind == "zero_after_3":
        g = z
        g[3:] = 0.0
    elif kind == "sparse":
        g = 1e-2 * z * (rng.random((T, n)) >= 0.9)
    elif kind == "wide":
        g = np.sign(z) * 10.0 ** rng.uniform(-12.0, 4.0, (T, n))
    elif kind == "alternating":
        g = 1e-3 * np.sign(z[0])[None, :] * ((-1.0) ** np.arange(T))[:, None]
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(g, dtype=np.float32)


def initial_state(n, start, first_step, seed=0):
    """(p0, m0, v0) float32 [n].  start: "zero" or "normal" (N(0,1)).  A run from step 1 has zero moments; a resumed one (first_step > 1)
    seeded non-zero ones, m0 ~ 1e-2 N(0,1), v0 ~ 1e-4 U(0,1)."""
    rng = np.random.default_rng([seed, 77, n, first_step])
    p0 = np.zeros(n) if start == "zero" else rng.standard_normal(n)
    if first_step > 1:
        m0, v0 = 1e-2 * rng.standard_normal(n), 1e-4 * rng.random(n)
    else:
        m0, v0 = np.zeros(n), np.zeros(n)
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (p0, m0, v0))


def trajectory(p0, m0, v0, g, lr, betas, eps, first_step=1, dtype=torch.float64):
    """torch.optim.Adam(weight_decay=0, amsgrad=False) on the CPU in `dtype` over the gradients g [T, n], the first of them taken at step
    count `first_step` -> (params, exp_avg, exp_avg_sq), each [T, n] float64: the state after every step."""
    g = np.asarray(g)
    T = g.shape[0]
    p = torch.nn.Parameter(torch.as_tensor(np.asarray(p0)).to(dtype).clone())
    opt = torch.optim.Adam([p], lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False)
    if first_step > 1:
        sd = opt.state_dict()
        sd["state"] = {0: {"step": torch.tensor(float(first_step - 1)), "exp_avg": torch.as_tensor(np.asarray(m0)).clone(),
                           "exp_avg_sq": torch.as_tensor(np.asarray(v0)).clone()}}
        opt.load_state_dict(sd)
    else:
        assert not np.any(m0) and not np.any(v0), "a run from step 1 starts from zero moments"
    out = [np.empty(g.shape, np.float64) for _ in range(3)]
    for t in range(T):
        p.grad = torch.as_tensor(g[t]).to(dtype)
        opt.step()
        st = opt.state[p]
        assert int(st["step"]) == first_step + t
        for dst, src in zip(out, (p.detach(), st["exp_avg"], st["exp_avg_sq"])):
            dst[t] = src.double().numpy()
    return tuple(out)


def restated_trajectory(p0, m0, v0, g, lr, betas, eps, first_step=1):
    """The same trajectory from oracle.torch_train_ref.adam_step iterated in float64."""
    p, m, v = (torch.as_tensor(np.asarray(a)).double() for a in (p0, m0, v0))
    out = [np.empty(np.shape(g), np.float64) for _ in range(3)]
    for t in range(np.shape(g)[0]):
        p, m, v = ttr.adam_step(p, torch.as_tensor(g[t]).double(), m, v, first_step + t, lr, betas[0], betas[1], eps)
        for dst, src in zip(out, (p, m, v)):
            dst[t] = src.numpy()
    return tuple(out)


def restatement_error(kind, n=257, T=12, lr=2.5e-4, betas=(0.9, 0.999), eps=1e-8, first_step=1, start="normal"):
    """Worst |restated - torch| / max |torch| over the three quantities and all steps, in float64."""
    p0, m0, v0 = initial_state(n, start, first_step)
    g = grads(kind, T, n)
    a = trajectory(p0, m0, v0, g, lr, betas, eps, first_step, torch.float64)
    b = restated_trajectory(p0, m0, v0, g, lr, betas, eps, first_step)
    return max(float(np.abs(x - y).max() / max(np.abs(x).max(), 1e-300)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------- the criterion
def _norms(got, ref64, ref32, rel_l2):
    got, ref64, ref32 = (np.asarray(a, np.float64).reshape(-1) for a in (got, ref64, ref32))
    if rel_l2:
        scale = max(float(np.linalg.norm(ref64)), 1e-300)
        return float(np.linalg.norm(got - ref64)) / scale, float(np.linalg.norm(ref32 - ref64)) / scale
    return float(np.abs(got - ref64).max()), float(np.abs(ref32 - ref64).max())


def close(got, ref64, ref32, margin, floor, rel_l2=False, d32_before=0.0):
    """-> (ok, err, d32): err <= margin * d32 + floor, in the max norm (parameters) or in relative L2 (rel_l2: the moments).
    d32_before: the largest d32 of the steps before this one (see the module docstring, (*)); the returned d32 is this step's own."""
    err, d32 = _norms(got, ref64, ref32, rel_l2)
    return bool(np.isfinite(err) and err <= margin * max(d32, d32_before) + floor), err, d32


def param_floor(ref64):
    """One float32 ulp of max |p| over everything given: ref64 [n] (one state) or [t, n] (the trajectory up to a step)."""
    return float(np.spacing(np.float32(np.abs(np.asarray(ref64)).max())))


def close_params(got, ref64, ref32, floor=None, d32_before=0.0):
    return close(got, ref64, ref32, MARGIN["param"], param_floor(ref64) if floor is None else floor, d32_before=d32_before)


def close_moment(which, got, ref64, ref32):
    return close(got, ref64, ref32, MARGIN[which], ULP32, rel_l2=True)


def ratio(err, d32):
    """err / d32 for the printout (nan where torch's float32 run is exact, so that the floor alone is the bound)."""
    return err / d32 if d32 > 0 else float("nan")


class Worst:
    """Collects the worst err / d32 per quantity over a module's cases, for the figures its docstring quotes."""

    def __init__(self):
        self.rows = {}

    def add(self, quantity, what, err, d32):
        r = ratio(err, d32)
        if np.isfinite(r) and r > self.rows.get(quantity, (-1.0, None))[0]:
            self.rows[quantity] = (r, what)
        return r

    def __str__(self):
        return "; ".join(f"{q} {r:.2f} ({w})" for q, (r, w) in sorted(self.rows.items()))


def check_trajectory(what, got_p, got_m, got_v, ref64, ref32, worst=None):
    """The assertions every optimiser test makes: after EVERY step the parameters are close to the float64 trajectory, after the last
    step both moments are.  got_p [T, n]; got_m, got_v [n].  Prints err / d32 per quantity and returns the list of failures."""
    bad, line = [], []
    rp = (-1.0, 0, 0.0, 0.0)
    peak = np.maximum.accumulate(np.abs(ref64[0]).max(axis=1))           # the largest |p| reached up to each step
    strayed = 0.0                                                        # the largest d32 up to each step
    for t in range(got_p.shape[0]):
        floor = float(np.spacing(np.float32(peak[t])))
        ok, err, d32 = close_params(got_p[t], ref64[0][t], ref32[0][t], floor, strayed)
        strayed = max(strayed, d32)
        if not ok:
            bad.append((what, "param", t + 1, err, strayed, floor))
        r = err / max(strayed, 1e-300)
        if r > rp[0]:
            rp = (r, t + 1, err, strayed)
    if worst is not None:
        worst.add("param", what, rp[2], rp[3])
    line.append(f"param {ratio(rp[2], rp[3]):.2f} (step {rp[1]}: err {rp[2]:.2e}, d32 {rp[3]:.2e})")
    for i, (which, got) in enumerate((("exp_avg", got_m), ("exp_avg_sq", got_v)), start=1):
        ok, err, d32 = close_moment(which, got, ref64[i][-1], ref32[i][-1])
        if not ok:
            bad.append((what, which, got_p.shape[0], err, d32, ULP32))
        if worst is not None:
            worst.add(which, what, err, d32)
        line.append(f"{which} {ratio(err, d32):.2f} (err {err:.2e}, d32 {d32:.2e})")
    print(f"[{what}] err/d32: " + " | ".join(line))
    return bad


@functools.lru_cache(maxsize=4)
def reference(kind, n, T, lr, betas, eps, start, first_step):
    """(g, (p0, m0, v0), float64 trajectory, float32 trajectory) of a case: computed once, shared by the tests that run it next to
    one another (the last few are kept: a 4099 x 40 case holds 8 MB, the million-element one 240 MB), read-only."""
    g = grads(kind, T, n)
    init = initial_state(n, start, first_step)
    ref64 = trajectory(*init, g, lr, betas, eps, first_step, torch.float64)
    ref32 = trajectory(*init, g, lr, betas, eps, first_step, torch.float32)
    for a in (g, *init, *ref64, *ref32):
        a.setflags(write=False)
    return g, init, ref64, ref32
