"""CPU model of the GRU navigation policy — the act step and one PPO minibatch update — for tests/test_policy_gru_host.py,
tests/test_gpu_policy_gru.py and tests/test_gpu_ppo_gru.py (TEST INFRASTRUCTURE ONLY).

Built as tests/ppo_reference.py builds the LSTM one, from the same pieces: oracle.torch_train_ref's encoder and Adam, and
ppo_reference's rollout inputs, loss, loss inputs, branch census and clip + Adam, all imported, none copied.  What differs is the
recurrent core: torch.nn.GRU stepped one t at a time with the mask applied to h, and a packed state of [L, N, Hd] (h only; the
initial state is the first L blocks of ppo_reference.rollout(case)["hidden"]).  Weights come from synth.make_state_dict, whose
biases are non-zero: with a zero bias_hh the placement of b_hn (inside the product with r) would be invisible.  float64 is the
reference; the same code in float32 gives the error of a float32 framework (GRAD_TOL of tests/test_gpu_ppo_gru.py).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import ppo_reference as R
from oracle import torch_train_ref as ttr
from ppo_reference import branch_census, clip_and_adam, loss_inputs, ppo_losses, rollout  # noqa: F401  (shared, not copied)
from pointnav_vo_amd import synth
from pointnav_vo_amd.policy import policy_state_dict_spec

GOAL, RNN, ENC = R.GOAL, R.RNN, R.ENC
CASES = R.CASES                                           # the GRU twins keep the LSTM cases' shapes, masks and seeds
CLIP, VALUE_COEF, ENTROPY_COEF = R.CLIP, R.VALUE_COEF, R.ENTROPY_COEF

# seeds of ppo_reference.loss_inputs picked on the CPU (pick_loss_seeds below, float64 only) so that the branch census of
# tests/test_gpu_ppo_gru.py holds on the GRU's own forward.  The search was run afresh and lands on the LSTM's seeds: the loss inputs
# are offsets from the model's own values and log-probabilities, so which branch an element takes hardly depends on the core
LOSS_SEED = {"A": 0, "B": 5, "B1": 21, "C": 9}


def spec(*, H, W, hidden, A, L, baseplanes=32):
    return policy_state_dict_spec(width=W, height=H, baseplanes=baseplanes, hidden=hidden, n_actions=A, rnn_layers=L, rnn_type="GRU")


def state_dict(case):
    c = CASES[case]
    return synth.make_state_dict(spec(H=c["H"], W=c["W"], hidden=c["hidden"], A=c["A"], L=c["L"]), seed=c["wseed"])


@functools.lru_cache(maxsize=None)
def gru_rollout(case, iseed=None):
    """ppo_reference.rollout with the GRU's state: hidden [L, N, Hd] = the first L blocks of the LSTM case's [2L, N, Hd]."""
    inp = rollout(case, iseed)
    return dict(inp, hidden=np.ascontiguousarray(inp["hidden"][:CASES[case]["L"]]))


def forward(P, inp, dtype):
    """evaluate_actions on the leaves P -> (value [M], log pi(a) [M], mean entropy, hidden_out [L,N,Hd], logits [M,A], features)."""
    T, N = inp["T"], inp["N"]
    M = T * N
    Hd = P["critic.fc.weight"].shape[1]
    L = sum(1 for k in P if k.startswith(RNN + "weight_hh_l"))
    depth = torch.as_tensor(inp["depth"]).to(dtype).permute(0, 3, 1, 2)
    pooled = F.avg_pool2d(depth, 2).permute(0, 2, 3, 1)
    obs = {"depth": torch.cat([pooled, torch.zeros_like(pooled)], dim=-1)}
    ep = {}
    for k, v in P.items():
        if k == ENC + "backbone.conv1.0.weight":
            ep["visual_encoder.backbone.conv1.0.weight"] = torch.cat([v, torch.zeros_like(v)], dim=1)
        elif k.startswith(ENC):
            ep["visual_encoder." + k[len(ENC):]] = v
    ep["visual_fc.2.weight"], ep["visual_fc.2.bias"] = P["net.visual_fc.1.weight"], P["net.visual_fc.1.bias"]
    ep["output_head.1.weight"], ep["output_head.1.bias"] = torch.eye(Hd, dtype=dtype), torch.zeros(Hd, dtype=dtype)
    rmv = "visual_encoder.running_mean_and_var."
    buffers = {rmv + "_mean": torch.zeros(1, 2, 1, 1, dtype=dtype), rmv + "_var": torch.ones(1, 2, 1, 1, dtype=dtype),
               rmv + "_count": torch.ones((), dtype=dtype)}
    baseplanes = P[ENC + "backbone.conv1.0.weight"].shape[0]
    visual, _ = ttr.forward(ep, buffers, obs, ngroups=baseplanes // 2, train=False, dtype=dtype)
    goal = torch.as_tensor(inp["goal"]).to(dtype)
    g3 = torch.stack([goal[:, 0], torch.cos(-goal[:, 1]), torch.sin(-goal[:, 1])], -1)
    tgt = F.linear(g3, P["net.tgt_embeding.weight"], P["net.tgt_embeding.bias"])
    masks = torch.as_tensor(inp["masks"]).to(torch.float32)
    idx = ((torch.as_tensor(inp["prev"]).to(torch.float32) + 1.0) * masks).long()
    emb = F.embedding(idx, P["net.prev_action_embedding.weight"])
    x = torch.cat([visual, tgt, emb], dim=1).view(T, N, -1)
    rnn = torch.nn.GRU(Hd + 64, Hd, L).to(dtype)
    for l in range(L):
        for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            del rnn._parameters[f"{nm}_l{l}"]
            setattr(rnn, f"{nm}_l{l}", P[f"{RNN}{nm}_l{l}"])       # plain tensors: the module computes on the leaves themselves
    rnn._flat_weights = [getattr(rnn, n) for n in rnn._flat_weights_names]
    h = torch.as_tensor(inp["hidden"]).to(dtype)
    assert tuple(h.shape) == (L, N, Hd), tuple(h.shape)
    md = masks.to(dtype).view(T, 1, N, 1)
    outs = []
    for t in range(T):
        o, h = rnn(x[t:t + 1], h * md[t])
        outs.append(o)
    feat = torch.cat(outs).view(M, Hd)
    logits = F.linear(feat, P["action_distribution.linear.weight"], P["action_distribution.linear.bias"])
    value = F.linear(feat, P["critic.fc.weight"], P["critic.fc.bias"]).view(M)
    lp = torch.log_softmax(logits, dim=-1)
    logp = lp.gather(-1, torch.as_tensor(inp["actions"]).view(M, 1)).view(M)
    entropy = -(lp.exp() * lp).sum(-1).mean()
    return value, logp, entropy, h, logits, feat


def policy_step(sd, depth, goal, prev, mask, hidden, dtype="float64"):
    """One act step of B environments -> dict(features [B,Hd], hidden [L,B,Hd], logits [B,A], value [B,1]) as float64 ndarrays."""
    B = depth.shape[0]
    inp = dict(depth=depth, goal=goal, prev=prev, masks=np.asarray(mask, np.float32), actions=np.zeros(B, np.int64),
               hidden=np.asarray(hidden), T=1, N=B)
    with torch.no_grad():
        value, _, _, h, logits, feat = forward(R.leaves(sd, getattr(torch, dtype)), inp, getattr(torch, dtype))
    f = lambda t: t.double().numpy()
    return dict(features=f(feat), hidden=f(h), logits=f(logits), value=f(value).reshape(B, 1))


def update(params, inp, li, dtype="float64", use_clipped=True):
    """One minibatch in `dtype` on the parameters `params` (name -> ndarray): forward, loss, gradients (float64 ndarrays)."""
    dt = getattr(torch, dtype)
    P = R.leaves(params, dt)
    value, logp, entropy, hidden, logits, _ = forward(P, inp, dt)
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
        out = forward(R.leaves(params, getattr(torch, dtype)), inp, getattr(torch, dtype))[:5]
    return tuple(o.double().numpy() for o in out)


@functools.lru_cache(maxsize=None)
def reference(case, dtype="float64", use_clipped=True, iseed=None):
    """update() of a case on its synthetic weights, computed once and shared (treat the result as read-only).  The loss inputs always
    come from the float64 forward."""
    inp = gru_rollout(case, iseed)
    sd = state_dict(case)
    v64, lp64 = evaluate(sd, inp)[:2]
    return update(sd, inp, loss_inputs(case, v64, lp64, seed=LOSS_SEED[case], iseed=iseed), dtype, use_clipped)


def census_ok(case, value, logp, li, need=1e-6):
    """The requirement of tests/test_gpu_ppo.py's assert_every_branch_is_live, as a predicate (float64 side only)."""
    s, v, margin = branch_census(value, logp, li)
    if not (margin.min() > need and (li["adv"] > 0).any() and (li["adv"] < 0).any()):
        return False
    if case == "A":
        return min(int(((s == a) & (v == b)).sum()) for a in (True, False) for b in (True, False)) >= 2
    return min(int(s.sum()), int((~s).sum()), int(v.sum()), int((~v).sum())) >= 2


def pick_loss_seeds(limit=200):
    """The first seed per case whose loss inputs pass census_ok on the float64 GRU forward, with every element at least 1e-4 from a
    branch boundary (the test asks for 1e-6: kept well clear of it).  How LOSS_SEED was filled."""
    out = {}
    for case in CASES:
        v, lp = evaluate(state_dict(case), gru_rollout(case))[:2]
        out[case] = next(s for s in range(limit) if census_ok(case, v, lp, loss_inputs(case, v, lp, seed=s), need=1e-4))
    return out


def float32_error_table():
    """Worst per-tensor relative L2 of this model's float32 gradients against its float64 ones, and the worst parameter difference
    after one clip + Adam step on the shipped settings, over the cases (where GRAD_TOL and the step's atol come from)."""
    worst_g, worst_p = {}, 0.0
    for case in CASES:
        r64, r32 = reference(case), reference(case, "float32")
        errs = {k: np.linalg.norm(r32["grads"][k] - g) / max(np.linalg.norm(g), 1e-12) for k, g in r64["grads"].items() if g.any()}
        k = max(errs, key=errs.get)
        worst_g[case] = (errs[k], k, float(np.median(list(errs.values()))))
        p64 = clip_and_adam(r64["params"], r64["grads"], lr=2.5e-4, eps=1e-5, max_norm=0.2)[0]
        p32 = clip_and_adam(r64["params"], r32["grads"], lr=2.5e-4, eps=1e-5, max_norm=0.2)[0]
        worst_p = max(worst_p, max(np.abs(p64[n] - p32[n]).max() for n in p64))
    return worst_g, worst_p


if __name__ == "__main__":
    import sys
    if "--seeds" in sys.argv:
        print("LOSS_SEED =", pick_loss_seeds())
    else:
        table, wp = float32_error_table()
        for case, (e, k, med) in table.items():
            print(f"{case}: worst float32 gradient tensor {e:.3e} ({k}), median {med:.2e}")
        print(f"worst parameter difference after clip + Adam, float32 vs float64 gradients: {wp:.2e}")
