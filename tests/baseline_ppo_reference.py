"""CPU model of one PPO minibatch update of the baseline navigation policy, for tests/test_baseline_ppo_host.py and
tests/test_gpu_baseline_ppo.py (TEST INFRASTRUCTURE ONLY).

A float64 torch-autograd restatement built from pieces that exist: baseline_policy_reference.encode and gru_cell (both differentiable)
stepped over T with the mask applied to h, Linear heads, a Categorical's log-probabilities and entropy; ppo_reference's ppo_losses,
loss_inputs, branch_census and clip_and_adam are imported, not copied.  tests/golden/gen_golden_baseline_ppo.py pins it to the imported
reference's own evaluate_actions + loss + backward (tests/golden/baseline_ppo_*.npz hold outputs only).  float64 is the reference; the
same code in float32 gives the error of a float32 framework on the same weights and inputs (GRAD_TOL of the GPU test):

    python tests/baseline_ppo_reference.py            # the float32-against-float64 table per case and tensor
    python tests/baseline_ppo_reference.py --seeds    # how LOSS_SEED was picked
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import baseline_policy_reference as B
import ppo_reference as R
from ppo_reference import branch_census, clip_and_adam, ppo_losses  # noqa: F401  (shared, not copied)
from pointnav_vo_amd import synth

GOAL, CNN, RNN = B.GOAL, B.CNN, B.RNN
ENC = "net.visual_encoder."
N_ACTIONS = B.N_ACTIONS
CLIP, VALUE_COEF, ENTROPY_COEF = R.CLIP, R.VALUE_COEF, R.ENTROPY_COEF

# the smallest shapes at which each kernel can still go wrong: frame (H, W), visual types, hidden, T, N, mask rows (None: the
# generator's), weight seed, input seed.  B1 and Ap share a policy with B and A.
MASKS_A = {0: [0, 1, 1], 2: [1, 0, 1], 4: [0, 1, 0]}      # a start reset, one environment mid-sequence, two at once, carried state
CASES = {
    # 85x53 -> maps 12x20, 5x9, 3x7: conv1 drops a remainder row and column, no pixel count is a multiple of 16
    "A": dict(H=53, W=85, vis=("rgb", "depth"), hidden=128, T=5, N=3, masks=MASKS_A, wseed=51, iseed=61),
    # 64x64 -> 15, 6, 4: conv2 drops a row and a column of its input
    "B": dict(H=64, W=64, vis=("depth",), hidden=128, T=4, N=1, masks={}, wseed=52, iseed=62),
    "B1": dict(H=64, W=64, vis=("depth",), hidden=128, T=1, N=4, masks={}, wseed=52, iseed=63),
    "C": dict(H=53, W=85, vis=("rgb",), hidden=128, T=2, N=2, masks=None, wseed=53, iseed=64),
    # 36 wide, 37 high -> 8x8, 3x3, 1x1: the smallest frame, conv3 has one output row
    "D": dict(H=37, W=36, vis=("depth",), hidden=128, T=2, N=1, masks=None, wseed=54, iseed=65),
    "E": dict(H=0, W=0, vis=(), hidden=128, T=3, N=2, masks=None, wseed=55, iseed=66),
    # the reference's frame: F = 24 960, 33 K slices, a 51 MB Linear weight, conv2 drops a row
    "F": dict(H=192, W=341, vis=("rgb", "depth"), hidden=512, T=2, N=2, masks=None, wseed=56, iseed=67),
}
# seeds of ppo_reference.loss_inputs' draws, picked on the CPU (pick_loss_seeds below, float64 only) so that census_ok holds
LOSS_SEED = {"A": 1, "B": 3, "B1": 0, "C": 1, "D": 2, "E": 0, "F": 0}


def spec(case):
    return B.spec(CASES[case])


def state_dict(case):
    return B.state_dict(CASES[case], seed=CASES[case]["wseed"])


@functools.lru_cache(maxsize=None)
def rollout(case):
    """T-major inputs of a case: rgb [M,H,W,3] uint8 | None, depth [M,H,W,1] | None, goal [M,2], masks [M], actions [M],
    hidden [1,N,Hd] (non-zero), T, N (numpy; treat as read-only)."""
    c = CASES[case]
    T, N, Hd = c["T"], c["N"], c["hidden"]
    steps = B.inputs(dict(c, B=N, steps=T))
    cat = lambda i: None if steps[0][i] is None else np.concatenate([s[i] for s in steps])
    if c["masks"] is None:
        masks = cat(3)
    else:
        masks = np.ones((T, N), np.float32)
        for t, row in c["masks"].items():
            masks[t] = row
        masks = masks.reshape(-1)
    actions = (synth.bits(c["iseed"], "taken", T * N) % np.uint64(N_ACTIONS)).astype(np.int64)
    h0 = synth.uniform(c["iseed"], "h0", (1, N, Hd), -1.0, 1.0).astype(np.float32)
    return dict(rgb=cat(0), depth=cat(1), goal=cat(2), masks=masks.astype(np.float32), actions=actions, hidden=h0, T=T, N=N)


def forward(P, inp, dtype):
    """evaluate_actions on the leaves P -> (value [M], log pi(a) [M], mean entropy, hidden_out [1,N,Hd], logits [M,A])."""
    T, N = inp["T"], inp["N"]
    M = T * N
    x = torch.as_tensor(inp["goal"]).to(dtype)
    if inp["rgb"] is not None or inp["depth"] is not None:
        x = torch.cat([B.encode(P, inp["rgb"], inp["depth"], dtype), x], dim=1)
    h = torch.as_tensor(inp["hidden"]).to(dtype)[0]
    masks = torch.as_tensor(inp["masks"]).to(dtype)
    outs = []
    for t in range(T):
        h = B.gru_cell(P, x[t * N:(t + 1) * N], h, masks[t * N:(t + 1) * N])
        outs.append(h)
    feat = torch.cat(outs)
    logits = F.linear(feat, P["action_distribution.linear.weight"], P["action_distribution.linear.bias"])
    value = F.linear(feat, P["critic.fc.weight"], P["critic.fc.bias"]).view(M)
    lp = torch.log_softmax(logits, dim=-1)
    logp = lp.gather(-1, torch.as_tensor(inp["actions"]).view(M, 1)).view(M)
    entropy = -(lp.exp() * lp).sum(-1).mean()
    return value, logp, entropy, h[None], logits


def loss_inputs(case, value64, logp64, seed=None):
    """ppo_reference.loss_inputs' draws for M rows of this module's cases (its own takes the shapes from ppo_reference.CASES: the
    case's T, N and seed are handed to it under a scratch name)."""
    c = CASES[case]
    key = "_baseline_" + case
    R.CASES[key] = dict(T=c["T"], N=c["N"], iseed=c["iseed"])
    try:
        return R.loss_inputs(key, value64, logp64, seed=LOSS_SEED[case] if seed is None else seed)
    finally:
        del R.CASES[key]


def update(params, inp, li, dtype="float64", use_clipped=True):
    """One minibatch in `dtype` on the parameters `params` (name -> ndarray): forward, loss, gradients (float64 ndarrays)."""
    dt = getattr(torch, dtype)
    P = R.leaves(params, dt)
    value, logp, entropy, hidden, logits = forward(P, inp, dt)
    t = lambda k: torch.as_tensor(li[k]).to(dt)
    vl, al, ent, total = ppo_losses(value, logp, entropy, t("old"), t("adv"), t("vp"), t("ret"), use_clipped=use_clipped)
    total.backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().double().numpy() for k, p in P.items()}
    return dict(value=value.detach().double().numpy(), logp=logp.detach().double().numpy(), entropy=float(entropy.detach()),
                hidden=hidden.detach().double().numpy(), logits=logits.detach().double().numpy(),
                losses=(float(vl.detach()), float(al.detach()), float(ent.detach())), total=float(total.detach()), grads=grads,
                loss_inputs=li, params={k: p.detach().double().numpy() for k, p in P.items()})


def evaluate(params, inp, dtype="float64"):
    """Forward only -> (value [M], log pi(a) [M], entropy, hidden_out, logits) as float64 ndarrays."""
    with torch.no_grad():
        out = forward(R.leaves(params, getattr(torch, dtype)), inp, getattr(torch, dtype))
    return tuple(o.double().numpy() for o in out)


@functools.lru_cache(maxsize=None)
def reference(case, dtype="float64", use_clipped=True):
    """update() of a case on its synthetic weights, computed once and shared (treat the result as read-only).  The loss inputs always
    come from the float64 forward."""
    inp = rollout(case)
    sd = state_dict(case)
    v64, lp64 = evaluate(sd, inp)[:2]
    return update(sd, inp, loss_inputs(case, v64, lp64), dtype, use_clipped)


def census_ok(case, value, logp, li, need=1e-6):
    """Every clipped / unclipped branch of both losses is taken by at least one row, no row lies within `need` of a branch boundary,
    and both signs of the advantage occur (float64 side only)."""
    s, v, margin = branch_census(value, logp, li)
    if not (margin.min() > need and (li["adv"] > 0).any() and (li["adv"] < 0).any()):
        return False
    return min(int(s.sum()), int((~s).sum()), int(v.sum()), int((~v).sum())) >= 1


def pick_loss_seeds(limit=500):
    """The first seed per case whose loss inputs pass census_ok on the float64 forward with every row at least 1e-4 from a branch
    boundary (the test asks for 1e-6: kept well clear of it).  How LOSS_SEED was filled."""
    out = {}
    for case in CASES:
        v, lp = evaluate(state_dict(case), rollout(case))[:2]
        out[case] = next(s for s in range(limit) if census_ok(case, v, lp, loss_inputs(case, v, lp, seed=s), need=1e-4))
    return out


LR, EPS, MAX_GRAD_NORM = 2.5e-4, 1e-5, 0.2                # the shipped optimiser settings


def float32_error_table():
    """Per case: {tensor: relative L2 of this model's float32 gradient against its float64 one} (tensors whose float64 gradient is
    exactly zero left out), the forward's worst error of scale, the losses' worst |difference| / max(1, |x|), and the worst parameter
    difference after one clip + Adam step on the shipped settings."""
    table = {}
    for case in CASES:
        r64, r32 = reference(case), reference(case, "float32")
        errs = {k: float(np.linalg.norm(r32["grads"][k] - g) / max(np.linalg.norm(g), 1e-12)) for k, g in r64["grads"].items() if g.any()}
        fwd = max(B.rel_err(r32[k], r64[k]) for k in ("value", "logp", "hidden"))
        loss = max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(r32["losses"], r64["losses"]))
        p64 = clip_and_adam(r64["params"], r64["grads"], lr=LR, eps=EPS, max_norm=MAX_GRAD_NORM)[0]
        p32 = clip_and_adam(r64["params"], r32["grads"], lr=LR, eps=EPS, max_norm=MAX_GRAD_NORM)[0]
        step = max(float(np.abs(p64[n] - p32[n]).max()) for n in p64)
        table[case] = dict(grads=errs, forward=fwd, loss=loss, step=step)
    return table


if __name__ == "__main__":
    import sys
    if "--seeds" in sys.argv:
        print("LOSS_SEED =", pick_loss_seeds())
    else:
        tab = float32_error_table()
        for case, r in tab.items():
            for k, e in r["grads"].items():
                print(f"{case:3s} {k:45s} float32 vs float64 gradient, relative L2 {e:.3e}")
            k = max(r["grads"], key=r["grads"].get)
            print(f"{case:3s} worst gradient tensor {r['grads'][k]:.3e} ({k}), median {np.median(list(r['grads'].values())):.2e}; "
                  f"forward {r['forward']:.2e} of scale; losses {r['loss']:.2e}; after clip + Adam {r['step']:.2e}")
        print(f"worst gradient tensor over the cases {max(max(r['grads'].values()) for r in tab.values()):.3e}; "
              f"worst parameter difference after clip + Adam {max(r['step'] for r in tab.values()):.2e}")
