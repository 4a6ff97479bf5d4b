"""CPU model of the navigation policy with rgb / rgb-d input and RunningMeanAndVar — the act step and one PPO minibatch update — for
tests/test_policy_rgbd_host.py, tests/test_gpu_policy_rgbd.py and tests/test_gpu_ppo_rgbd.py (TEST INFRASTRUCTURE ONLY).

Built as tests/ppo_reference.py and tests/gru_reference.py build theirs, from the same pieces, imported and not copied:
oracle.torch_train_ref.forward (train=True runs RunningMeanAndVar's update, running_stats_update, before it whitens) and Adam,
ppo_reference's loss, loss inputs, branch census and clip + Adam.  What differs is the encoder's input: rgb / 255 and depth
concatenated in that order (resnet_policy.py:150-167), optionally area-resized and center-cropped per sensor (RL.OBS_TRANSFORM, :164-165),
F.avg_pool2d(x, 2), then the C pooled channels followed by C zero channels with zero stem weights and statistics (mean 0, variance 1):
the oracle's one 'depth' modality of 2C channels, which keeps the reference's channel order.  The statistics of the C real channels
come back as the new buffers.  The recurrent core is torch.nn.LSTM or torch.nn.GRU stepped one t at a time with the masks applied to
the state.  tests/test_policy_rgbd_host.py pins this model to the reference policy's recorded outputs
(tests/golden/policy_rgbd_128x96_h128_b2.npz).  float64 is the reference; the same code in float32 gives the error of a float32
framework (GRAD_TOL and STAT_TOL of the GPU tests).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import ppo_reference as R
from oracle import torch_train_ref as ttr
from ppo_reference import branch_census, clip_and_adam, ppo_losses  # noqa: F401  (shared, not copied)
from pointnav_vo_amd import synth
from pointnav_vo_amd.obs_transforms import transformed_size
from pointnav_vo_amd.policy import RMV_PREFIX, policy_state_dict_spec

GOAL, RNN, ENC = R.GOAL, R.RNN, R.ENC
CLIP, VALUE_COEF, ENTROPY_COEF = R.CLIP, R.VALUE_COEF, R.ENTROPY_COEF
STATS = ("_mean", "_var", "_count")

# the update cases (frames 96 x 128, hidden 128, 2 layers, 4 actions): rgb + depth on the LSTM with a start reset and a mid-sequence
# reset of one environment; rgb alone on the GRU in the M == N single-step form
CASES = {
    "RGBD": dict(vis=("rgb", "depth"), rnn="LSTM", H=96, W=128, hidden=128, L=2, A=4, T=3, N=2, masks={0: [0, 0], 1: [1, 0]}, wseed=21, iseed=41),
    "RGB": dict(vis=("rgb",), rnn="GRU", H=96, W=128, hidden=128, L=2, A=4, T=1, N=3, masks={}, wseed=22, iseed=42),
}
# seeds of loss_inputs picked on the CPU (python tests/rgbd_policy_reference.py --seeds, float64 only) so that the branch census of
# tests/test_gpu_ppo_rgbd.py holds
LOSS_SEED = {"RGBD": 0, "RGB": 0}


def spec(*, H, W, hidden, A, L, rnn, vis, normalize=True):
    return policy_state_dict_spec(width=W, height=H, hidden=hidden, n_actions=A, rnn_layers=L, rnn_type=rnn, vis_types=tuple(vis),
                                  normalize_visual_inputs=normalize)


def split(sd):
    """state_dict -> (parameters, the three statistics buffers or None)."""
    params = {k: v for k, v in sd.items() if not k.startswith(RMV_PREFIX)}
    bufs = {k[len(RMV_PREFIX):]: np.asarray(v) for k, v in sd.items() if k.startswith(RMV_PREFIX)}
    return params, (bufs or None)


def state_dict(case, zero_stats=True):
    c = CASES[case]
    sd = synth.make_state_dict(spec(H=c["H"], W=c["W"], hidden=c["hidden"], A=c["A"], L=c["L"], rnn=c["rnn"], vis=c["vis"]), seed=c["wseed"])
    if zero_stats:
        for k in sd:
            if k.startswith(RMV_PREFIX):
                sd[k] = np.zeros_like(sd[k])
    return sd


@functools.lru_cache(maxsize=None)
def rollout(case, call=0):
    """T-major inputs of a case: rgb [M,H,W,3] uint8, depth [M,H,W,1], goal, prev, masks, actions, hidden (numpy).  `call` > 0 draws the
    frames of a later evaluate_actions call (other frames, the same state and actions)."""
    c = CASES[case]
    T, N, Hd, L = c["T"], c["N"], c["hidden"], c["L"]
    steps = synth.make_policy_rgbd_inputs(c["H"], c["W"], N, T, c["iseed"] + 100 * call, c["A"])
    cat = lambda i: np.concatenate([s[i] for s in steps])
    masks = np.ones((T, N), np.float32)
    for t, row in c["masks"].items():
        masks[t] = row
    actions = (synth.bits(c["iseed"], "taken", T * N) % np.uint64(c["A"])).astype(np.int64)
    h0 = synth.uniform(c["iseed"], "h0", (L, N, Hd), -1.0, 1.0)
    c0 = synth.uniform(c["iseed"], "c0", (L, N, Hd), -3.0, 3.0)
    hidden = np.concatenate([h0, c0]) if c["rnn"] == "LSTM" else h0
    inp = dict(goal=cat(2), prev=cat(3), masks=masks.reshape(-1), actions=actions, hidden=hidden.astype(np.float32), T=T, N=N)
    if "rgb" in c["vis"]:
        inp["rgb"] = cat(0)
    if "depth" in c["vis"]:
        inp["depth"] = cat(1)
    return inp


def area_transform(x, mode, size):
    """ResizeCenterCropper / Resizer on a contiguous NCHW tensor (misc_utils.py:241-318): area interpolation of the shortest edge, then
    the center crop."""
    rs_h, rs_w, cy, cx, oh, ow = transformed_size(x.shape[2], x.shape[3], mode, size)
    return F.interpolate(x, size=(rs_h, rs_w), mode="area")[:, :, cy:cy + oh, cx:cx + ow]


def pooled_input(inp, dtype, transform=None):
    """ResNetEncoder.forward up to running_mean_and_var (resnet_policy.py:150-168) -> [M, C, H/2, W/2]."""
    parts = []
    if "rgb" in inp:
        parts.append(torch.as_tensor(np.asarray(inp["rgb"])).to(dtype).permute(0, 3, 1, 2).contiguous() / 255.0)
    if "depth" in inp:
        parts.append(torch.as_tensor(np.asarray(inp["depth"])).to(dtype).permute(0, 3, 1, 2).contiguous())
    if transform is not None:
        parts = [area_transform(p, *transform) for p in parts]
    return F.avg_pool2d(torch.cat(parts, dim=1), 2)


def forward(P, bufs, inp, dtype, rnn_type, train, transform=None):
    """evaluate_actions on the leaves P with the statistics `bufs` ({'_mean', '_var', '_count'} or None: no normalisation) ->
    (value [M], log pi(a) [M], mean entropy, hidden_out, logits [M,A], features [M,Hd], new statistics)."""
    T, N = inp["T"], inp["N"]
    M = T * N
    Hd = P["critic.fc.weight"].shape[1]
    L = sum(1 for k in P if k.startswith(RNN + "weight_hh_l"))
    pooled = pooled_input(inp, dtype, transform).permute(0, 2, 3, 1)
    C = pooled.shape[-1]
    obs = {"depth": torch.cat([pooled, torch.zeros_like(pooled)], dim=-1)}
    ep = {}
    for k, v in P.items():
        if k == ENC + "backbone.conv1.0.weight":
            assert v.shape[1] == C, (tuple(v.shape), C)
            ep["visual_encoder.backbone.conv1.0.weight"] = torch.cat([v, torch.zeros_like(v)], dim=1)
        elif k.startswith(ENC):
            ep["visual_encoder." + k[len(ENC):]] = v
    ep["visual_fc.2.weight"], ep["visual_fc.2.bias"] = P["net.visual_fc.1.weight"], P["net.visual_fc.1.bias"]
    ep["output_head.1.weight"], ep["output_head.1.bias"] = torch.eye(Hd, dtype=dtype), torch.zeros(Hd, dtype=dtype)
    rmv = "visual_encoder.running_mean_and_var."
    if bufs is None:
        buffers = {rmv + "_mean": torch.zeros(1, 2 * C, 1, 1, dtype=dtype), rmv + "_var": torch.ones(1, 2 * C, 1, 1, dtype=dtype),
                   rmv + "_count": torch.ones((), dtype=dtype)}
        train = False
    else:
        b = {k: torch.as_tensor(np.asarray(bufs[k])).to(dtype) for k in STATS}
        buffers = {rmv + "_mean": torch.cat([b["_mean"], torch.zeros_like(b["_mean"])], dim=1),
                   rmv + "_var": torch.cat([b["_var"], torch.ones_like(b["_var"])], dim=1), rmv + "_count": b["_count"]}
    baseplanes = P[ENC + "backbone.conv1.0.weight"].shape[0]
    visual, nb = ttr.forward(ep, buffers, obs, ngroups=baseplanes // 2, train=bool(train), dtype=dtype)
    new_bufs = None if bufs is None else {"_mean": nb[rmv + "_mean"][:, :C], "_var": nb[rmv + "_var"][:, :C], "_count": nb[rmv + "_count"]}
    goal = torch.as_tensor(inp["goal"]).to(dtype)
    g3 = torch.stack([goal[:, 0], torch.cos(-goal[:, 1]), torch.sin(-goal[:, 1])], -1)
    tgt = F.linear(g3, P["net.tgt_embeding.weight"], P["net.tgt_embeding.bias"])
    masks = torch.as_tensor(inp["masks"]).to(torch.float32)
    idx = ((torch.as_tensor(inp["prev"]).to(torch.float32) + 1.0) * masks).long()
    emb = F.embedding(idx, P["net.prev_action_embedding.weight"])
    x = torch.cat([visual, tgt, emb], dim=1).view(T, N, -1)
    rnn = (torch.nn.LSTM if rnn_type == "LSTM" else torch.nn.GRU)(Hd + 64, Hd, L).to(dtype)
    for l in range(L):
        for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            del rnn._parameters[f"{nm}_l{l}"]
            setattr(rnn, f"{nm}_l{l}", P[f"{RNN}{nm}_l{l}"])       # plain tensors: the module computes on the leaves themselves
    rnn._flat_weights = [getattr(rnn, n) for n in rnn._flat_weights_names]
    hid = torch.as_tensor(np.asarray(inp["hidden"])).to(dtype)
    md = masks.to(dtype).view(T, 1, N, 1)
    outs = []
    if rnn_type == "LSTM":
        h, c = hid[:L], hid[L:]
        for t in range(T):
            o, (h, c) = rnn(x[t:t + 1], (h * md[t], c * md[t]))
            outs.append(o)
        hidden = torch.cat([h, c])
    else:
        h = hid
        for t in range(T):
            o, h = rnn(x[t:t + 1], h * md[t])
            outs.append(o)
        hidden = h
    feat = torch.cat(outs).view(M, Hd)
    logits = F.linear(feat, P["action_distribution.linear.weight"], P["action_distribution.linear.bias"])
    value = F.linear(feat, P["critic.fc.weight"], P["critic.fc.bias"]).view(M)
    lp = torch.log_softmax(logits, dim=-1)
    logp = lp.gather(-1, torch.as_tensor(inp["actions"]).view(M, 1)).view(M)
    entropy = -(lp.exp() * lp).sum(-1).mean()
    return value, logp, entropy, hidden, logits, feat, new_bufs


def bufs_numpy(b):
    return None if b is None else {k: v.detach().double().numpy() for k, v in b.items()}


def policy_step(sd, frames, goal, prev, mask, hidden, rnn_type, train, dtype="float64", transform=None):
    """One act step of B environments on a whole state_dict (statistics included when the policy normalises); frames = dict with 'rgb'
    and / or 'depth' -> dict(features [B,Hd], hidden, logits [B,A], value [B,1], stats = the statistics after the step)."""
    B = len(goal)
    params, bufs = split(sd)
    inp = dict(frames, goal=goal, prev=prev, masks=np.asarray(mask, np.float32), actions=np.zeros(B, np.int64), hidden=np.asarray(hidden),
               T=1, N=B)
    dt = getattr(torch, dtype)
    with torch.no_grad():
        value, _, _, h, logits, feat, nb = forward(R.leaves(params, dt), bufs, inp, dt, rnn_type, train, transform)
    f = lambda t: t.double().numpy()
    return dict(features=f(feat), hidden=f(h), logits=f(logits), value=f(value).reshape(B, 1), stats=bufs_numpy(nb))


def loss_inputs(case, value64, logp64, seed=None):
    """ppo_reference.loss_inputs' recipe on this module's cases."""
    c = CASES[case]
    seed = c["iseed"] * 1000 + (LOSS_SEED[case] if seed is None else seed)
    M = c["T"] * c["N"]
    old = logp64 + synth.uniform(seed, "old", (M,), -0.4, 0.4)
    vp = value64 + synth.uniform(seed, "vp", (M,), -0.5, 0.5)
    adv = synth.uniform(seed, "adv", (M,), -1.0, 1.0)
    return dict(old=old.astype(np.float32), vp=vp.astype(np.float32), adv=adv.astype(np.float32), ret=(vp + adv).astype(np.float32))


def update(sd, inp, li, rnn_type, dtype="float64", train=True):
    """One minibatch in `dtype` on the state_dict `sd`: forward (the statistics updated first when `train`), loss, gradients."""
    dt = getattr(torch, dtype)
    params, bufs = split(sd)
    P = R.leaves(params, dt)
    value, logp, entropy, hidden, logits, _, nb = forward(P, bufs, inp, dt, rnn_type, train)
    t = lambda k: torch.as_tensor(li[k]).to(dt)
    vl, al, ent, total = ppo_losses(value, logp, entropy, t("old"), t("adv"), t("vp"), t("ret"))
    total.backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().double().numpy() for k, p in P.items()}
    return dict(value=value.detach().double().numpy(), logp=logp.detach().double().numpy(), entropy=float(entropy.detach()),
                hidden=hidden.detach().double().numpy(), logits=logits.detach().double().numpy(),
                losses=(float(vl.detach()), float(al.detach()), float(ent.detach())), grads=grads, loss_inputs=li,
                params={k: p.detach().double().numpy() for k, p in P.items()}, stats=bufs_numpy(nb))


def with_stats(sd, stats):
    out = dict(sd)
    for k in STATS:
        out[RMV_PREFIX + k] = np.asarray(stats[k])
    return out


@functools.lru_cache(maxsize=None)
def reference(case, dtype="float64"):
    """update() of a case from zero-initialised statistics in training mode, computed once and shared (read-only).  The loss inputs
    come from the float64 forward.  'stats2': the statistics after a SECOND evaluate_actions, on rollout(case, 1), in `dtype`."""
    c = CASES[case]
    sd = state_dict(case)
    r64 = update(sd, rollout(case), loss_inputs(case, np.zeros(c["T"] * c["N"]), np.zeros(c["T"] * c["N"])), c["rnn"])
    li = loss_inputs(case, r64["value"], r64["logp"])
    out = update(sd, rollout(case), li, c["rnn"], dtype)
    second = update(with_stats(sd, out["stats"]), rollout(case, 1), li, c["rnn"], dtype)
    out["stats2"] = second["stats"]
    return out


def stats_error(stats_list64, stats_list32):
    """Worst |float32 - float64| of _mean and of _var over a list of recorded statistics, each relative to the largest |value| of the
    float64 tensor."""
    worst = {"_mean": 0.0, "_var": 0.0}
    for s64, s32 in zip(stats_list64, stats_list32):
        for k in worst:
            worst[k] = max(worst[k], float(np.abs(s32[k] - s64[k]).max() / np.abs(s64[k]).max()))
    return worst


STEM = ENC + "backbone.conv1.0.weight"


def with_stem_channels(grads):
    """The gradient tensors, plus each input channel of the stem weight [C0,C,7,7] as an entry of its own ('...weight[:, c]'): the C
    channels of the input (rgb, depth) are judged one by one, not only as a whole."""
    out = dict(grads)
    for c in range(grads[STEM].shape[1]):
        out[f"{STEM}[:, {c}]"] = grads[STEM][:, c]
    return out


def census_ok(value, logp, li, need=1e-6):
    s, v, margin = branch_census(value, logp, li)
    return bool(margin.min() > need and (li["adv"] > 0).any() and (li["adv"] < 0).any() and
                min(int(s.sum()), int((~s).sum()), int(v.sum()), int((~v).sum())) >= 1)


def pick_loss_seeds(limit=200):
    """The first seed per case whose loss inputs give every branch of each clamp an element, none within 1e-4 of a boundary."""
    out = {}
    for case, c in CASES.items():
        z = np.zeros(c["T"] * c["N"])
        r = update(state_dict(case), rollout(case), loss_inputs(case, z, z, seed=0), c["rnn"])
        out[case] = next(s for s in range(limit) if census_ok(r["value"], r["logp"], loss_inputs(case, r["value"], r["logp"], seed=s), 1e-4))
    return out


def float32_error_table():
    """Worst per-tensor relative L2 of this model's float32 gradients against its float64 ones, the worst parameter difference after
    one clip + Adam step on the shipped settings, and the worst statistics error after one and two calls (where GRAD_TOL, the step's
    atol and STAT_TOL of tests/test_gpu_ppo_rgbd.py come from)."""
    table, worst_p, worst_s = {}, 0.0, {"_mean": 0.0, "_var": 0.0}
    for case in CASES:
        r64, r32 = reference(case), reference(case, "float32")
        g64, g32 = with_stem_channels(r64["grads"]), with_stem_channels(r32["grads"])
        errs = {k: np.linalg.norm(g32[k] - g) / max(np.linalg.norm(g), 1e-12) for k, g in g64.items() if g.any()}
        k = max(errs, key=errs.get)
        table[case] = (errs[k], k, float(np.median(list(errs.values()))))
        p64 = clip_and_adam(r64["params"], r64["grads"], lr=2.5e-4, eps=1e-5, max_norm=0.2)[0]
        p32 = clip_and_adam(r64["params"], r32["grads"], lr=2.5e-4, eps=1e-5, max_norm=0.2)[0]
        worst_p = max(worst_p, max(np.abs(p64[n] - p32[n]).max() for n in p64))
        e = stats_error([r64["stats"], r64["stats2"]], [r32["stats"], r32["stats2"]])
        worst_s = {k: max(worst_s[k], e[k]) for k in worst_s}
    return table, worst_p, worst_s


if __name__ == "__main__":
    import sys
    if "--seeds" in sys.argv:
        print("LOSS_SEED =", pick_loss_seeds())
    else:
        table, wp, ws = float32_error_table()
        for case, (e, k, med) in table.items():
            print(f"{case}: worst float32 gradient tensor {e:.3e} ({k}), median {med:.2e}")
        print(f"worst parameter difference after clip + Adam, float32 vs float64 gradients: {wp:.2e}")
        print(f"worst float32 statistics error after one and two calls: mean {ws['_mean']:.2e}, var {ws['_var']:.2e}")
