"""CPU model of the Bottleneck / ResNeXt / SE-ResNeXt encoders (resnet.py:58-286) and of the navigation policy and VO model around
them, for tests/test_policy_backbones_host.py, tests/test_gpu_policy_backbones.py and the batch-regime modules
tests/test_gpu_backbone_regimes.py / tests/test_backbone_regimes_host.py (TEST INFRASTRUCTURE ONLY).

oracle.torch_train_ref.forward knows BasicBlock and the plain Bottleneck; it has no grouped conv and no squeeze-and-excite branch.
`encoder_forward` below restates the whole VO-model forward with both, from torch primitives alone (F.conv2d(groups=), F.group_norm,
F.linear): same signature, same input assembly and whitening (imported from the oracle module, not copied), the conv groups read off
the weight's shape ([planes, planes / cardinality, 3, 3]: the first block of each stage only, resnet.py:198-210), the SE branch
present where a block has `se.excite.*` tensors.  The recurrent core, the heads and the PPO pieces are those of
tests/rgbd_policy_reference.py (which builds on tests/ppo_reference.py and tests/gru_reference.py), imported and not copied: `policy`
runs that module's functions with this encoder in the oracle's place.  tests/test_policy_backbones_host.py pins the restatement to the
imported reference's recorded outputs (tests/golden/policy_backbones_136x104_h128_b2.npz).  float64 is the reference.
"""
import contextlib
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

import rgbd_policy_reference as G
from oracle import torch_train_ref as ttr
from pointnav_vo_amd import model_spec as ms
from pointnav_vo_amd import synth
from pointnav_vo_amd.policy import policy_state_dict_spec

GOAL, RNN, ENC = G.GOAL, G.RNN, G.ENC
H, W, HIDDEN, LAYERS, N_ACT = 104, 136, 128, 2, 4        # the fixture's geometry: stage maps 13x17, 7x9, 4x5, 2x3; compression 341
WEIGHT_SEED = 31
TAPS = ("layer3.0", "layer4.0")                          # + the last block: the block outputs the fixture records

# fixture cases: backbone, visual types, normalisation, recurrent core, act steps, input seed
CASES = {
    "a": dict(backbone="se_resneXt50", vis=("depth",), normalize=False, rnn="LSTM", steps=3, iseed=51),
    "b": dict(backbone="se_resnet50", vis=("rgb", "depth"), normalize=True, rnn="GRU", steps=2, iseed=52),
    "c": dict(backbone="resneXt50", vis=("depth",), normalize=False, rnn="LSTM", steps=1, iseed=53),
    "d": dict(backbone="resnet50", vis=("depth",), normalize=False, rnn="LSTM", steps=1, iseed=54),
    "e": dict(backbone="se_resneXt101", vis=("depth",), normalize=False, rnn="LSTM", steps=1, iseed=55),
    "f": dict(backbone="resnet101", vis=("depth",), normalize=False, rnn="LSTM", steps=1, iseed=56),
}
# the VO case: the VO base class (what vo_cnn constructs) on se_resneXt50 at the deeper-variant fixture's reduced frame size
VO = dict(backbone="se_resneXt50", W=64, H=48, B=2, hidden=512, seed=31, space=("rgb", "depth"), dd_bins=0)


TAP_SAMPLES = 1024


def tap_digest(name, arr):
    """What the fixture keeps of a block output [B,C,h,w] (the full float64 tensors of six models would not fit a 1 MiB fixture): its
    values at TAP_SAMPLES fixed pseudo-random positions of the flattened NCHW tensor, and (mean, rms, max |.|) over ALL of it."""
    flat = np.asarray(arr, np.float64).reshape(-1)
    idx = (synth.bits(1234, "tap:" + name, TAP_SAMPLES) % np.uint64(flat.size)).astype(np.int64)
    return flat[idx], np.array([flat.mean(), np.sqrt((flat ** 2).mean()), np.abs(flat).max()])


def last_tap(backbone):
    blocks = ms.BACKBONES[backbone][1]
    return f"layer4.{blocks[3] - 1}"


def spec(case=None, **kw):
    c = dict(CASES[case]) if case else {}
    c.update(kw)
    return policy_state_dict_spec(width=c.get("W", W), height=c.get("H", H), hidden=c.get("hidden", HIDDEN), n_actions=N_ACT,
                                  rnn_layers=LAYERS, rnn_type=c["rnn"], vis_types=tuple(c["vis"]),
                                  normalize_visual_inputs=c["normalize"], backbone=c["backbone"])


@functools.lru_cache(maxsize=None)
def _state_dict(backbone, vis, normalize, rnn):
    return synth.make_state_dict(spec(backbone=backbone, vis=vis, normalize=normalize, rnn=rnn), seed=WEIGHT_SEED)


def state_dict(case=None, **kw):
    """The synthetic weights of a fixture case, or of (backbone, vis, normalize, rnn) given as keywords; shared, read-only."""
    c = dict(CASES[case]) if case else {}
    c.update(kw)
    return _state_dict(c["backbone"], tuple(c["vis"]), bool(c["normalize"]), c["rnn"])


def step_inputs(case):
    """Per act step of a fixture case: (frames dict, goal, prev_actions, masks); step 0 starts every episode, step 2 resets one."""
    c = CASES[case]
    out = []
    for rgb, depth, goal, prev, mask in synth.make_policy_rgbd_inputs(H, W, 2, c["steps"], c["iseed"], N_ACT):
        frames = {}
        if "rgb" in c["vis"]:
            frames["rgb"] = rgb
        if "depth" in c["vis"]:
            frames["depth"] = depth
        out.append((frames, goal, prev, mask))
    return out


def se_gate(z, w1, b1, w2, b2):
    """SE.forward (resnet.py:82-88) on the block's last GroupNorm output z [B,C,h,w] -> gates [B,C]."""
    s = z.mean(dim=(2, 3))
    return torch.sigmoid(F.linear(F.relu(F.linear(s, w1, b1)), w2, b2))


def encoder_forward(params, buffers, obs, *, ngroups, train, dropout_p=0.0, dtype=torch.float64, drop_masks=None, actions=None,
                    relu=F.relu, record=None):
    """oracle.torch_train_ref.forward's contract (VO-model names) for every backbone of resnet.py:226-286, eval statistics only.
    `record`: a dict that receives 'layerS.B' block outputs, 'gates/layerS.B' and 'encoder' (the compression block's output)."""
    assert not train and dropout_p == 0.0 and drop_masks is None, "the backbone restatement is an inference model"
    g = lambda k: params[k]
    pre = "visual_encoder."
    x = ttr.assemble(obs, dtype)
    mean, var, count = (buffers[pre + "running_mean_and_var." + k].to(dtype) for k in ("_mean", "_var", "_count"))
    x = (x - mean) / torch.sqrt(torch.max(var, torch.full_like(var, 1e-2)))
    bb = pre + "backbone."
    gn = lambda t, name: F.group_norm(t, ngroups, g(name + ".weight"), g(name + ".bias"))
    x = F.max_pool2d(relu(gn(F.conv2d(x, g(bb + "conv1.0.weight"), stride=2, padding=3), bb + "conv1.1")), 3, 2, 1)
    for li in range(1, 5):
        bi = 0
        while (bb + f"layer{li}.{bi}.convs.0.weight") in params:
            p = bb + f"layer{li}.{bi}."
            stride = 2 if (li > 1 and bi == 0) else 1
            if (p + "convs.6.weight") in params:           # conv1x1 -> GN -> ReLU -> conv3x3(stride, groups) -> GN -> ReLU -> conv1x1 -> GN
                o = relu(gn(F.conv2d(x, g(p + "convs.0.weight")), p + "convs.1"))
                w3 = g(p + "convs.3.weight")
                o = relu(gn(F.conv2d(o, w3, stride=stride, padding=1, groups=o.shape[1] // w3.shape[1]), p + "convs.4"))
                o = gn(F.conv2d(o, g(p + "convs.6.weight")), p + "convs.7")
            else:
                o = relu(gn(F.conv2d(x, g(p + "convs.0.weight"), stride=stride, padding=1), p + "convs.1"))
                o = gn(F.conv2d(o, g(p + "convs.3.weight"), padding=1), p + "convs.4")
            if (p + "se.excite.0.weight") in params:       # out = se(out) * out, before the skip branch is added (resnet.py:131-140)
                gate = se_gate(o, g(p + "se.excite.0.weight"), g(p + "se.excite.0.bias"), g(p + "se.excite.2.weight"),
                               g(p + "se.excite.2.bias"))
                if record is not None:
                    record[f"gates/layer{li}.{bi}"] = gate
                o = gate[:, :, None, None] * o
            r = x
            if (p + "downsample.0.weight") in params:
                r = gn(F.conv2d(x, g(p + "downsample.0.weight"), stride=stride), p + "downsample.1")
            x = relu(o + r)
            if record is not None:
                record[f"layer{li}.{bi}"] = x
            bi += 1
    x = relu(F.group_norm(F.conv2d(x, g(pre + "compression.0.weight"), padding=1), 1, g(pre + "compression.1.weight"),
                          g(pre + "compression.1.bias")))
    if record is not None:
        record["encoder"] = x
    h = relu(F.linear(x.flatten(1), g("visual_fc.2.weight"), g("visual_fc.2.bias")))
    out = F.linear(h, g("output_head.1.weight"), g("output_head.1.bias"))
    return out, dict(buffers)


@contextlib.contextmanager
def policy(record=None):
    """tests/rgbd_policy_reference.py with this module's encoder where it calls the oracle's: inside the block G.forward,
    G.policy_step and G.update are the navigation policy on any backbone (in eval mode: `train` is dropped — these encoders run
    frozen and, in the cases here, on loaded statistics)."""
    shim = types.SimpleNamespace(
        forward=lambda ep, buffers, obs, *, ngroups, train, dtype: encoder_forward(ep, buffers, obs, ngroups=ngroups, train=False,
                                                                                 dtype=dtype, record=record),
        adam_step=ttr.adam_step)
    saved = G.ttr
    G.ttr = shim
    try:
        yield G
    finally:
        G.ttr = saved


def policy_step(sd, frames, goal, prev, mask, hidden, rnn_type, dtype="float64"):
    """One act step in eval mode -> dict(features, hidden, logits, value, encoder [B,C,fh,fw], taps {name: [B,C,h,w]}, gates)."""
    rec = {}
    with policy(rec) as g:
        out = g.policy_step(sd, frames, goal, prev, mask, hidden, rnn_type, train=False, dtype=dtype)
    f = lambda t: t.double().numpy()
    out["encoder"] = f(rec["encoder"])
    out["taps"] = {k: f(v) for k, v in rec.items() if k.startswith("layer")}
    out["gates"] = {k[6:]: f(v) for k, v in rec.items() if k.startswith("gates/")}
    return out


def run_case(case, dtype="float64"):
    """The act steps of a fixture case from a zero state -> list of policy_step results."""
    c = CASES[case]
    sd = state_dict(case)
    states = LAYERS * (2 if c["rnn"] == "LSTM" else 1)
    hidden = np.zeros((states, 2, HIDDEN), np.float32)
    out = []
    for frames, goal, prev, mask in step_inputs(case):
        r = policy_step(sd, frames, goal, prev, mask, hidden, c["rnn"], dtype)
        out.append(r)
        hidden = r["hidden"]
    return out


# ---- the frozen-encoder PPO update (tests/test_gpu_static_encoder.py's shape: T = 3, N = 2, a start reset and a mid-sequence reset)
PPO = dict(backbone="se_resneXt50", vis=("depth",), normalize=False, rnn="LSTM", T=3, N=2, masks={0: [0, 0], 1: [1, 0]}, iseed=61)
PPO_LOSS_SEED = 1          # picked on the CPU (python tests/backbone_reference.py --seeds, float64 only) so that G.census_ok holds


@functools.lru_cache(maxsize=None)
def ppo_rollout():
    T, N = PPO["T"], PPO["N"]
    steps = synth.make_policy_rgbd_inputs(H, W, N, T, PPO["iseed"], N_ACT)
    cat = lambda i: np.concatenate([s[i] for s in steps])
    masks = np.ones((T, N), np.float32)
    for t, row in PPO["masks"].items():
        masks[t] = row
    actions = (synth.bits(PPO["iseed"], "taken", T * N) % np.uint64(N_ACT)).astype(np.int64)
    h0 = synth.uniform(PPO["iseed"], "h0", (LAYERS, N, HIDDEN), -1.0, 1.0)
    c0 = synth.uniform(PPO["iseed"], "c0", (LAYERS, N, HIDDEN), -3.0, 3.0)
    return dict(depth=cat(1), goal=cat(2), prev=cat(3), masks=masks.reshape(-1), actions=actions,
                hidden=np.concatenate([h0, c0]).astype(np.float32), T=T, N=N)


def ppo_loss_inputs(value64, logp64, seed=None):
    seed = PPO["iseed"] * 1000 + (PPO_LOSS_SEED if seed is None else seed)
    M = PPO["T"] * PPO["N"]
    old = logp64 + synth.uniform(seed, "old", (M,), -0.4, 0.4)
    vp = value64 + synth.uniform(seed, "vp", (M,), -0.5, 0.5)
    adv = synth.uniform(seed, "adv", (M,), -1.0, 1.0)
    return dict(old=old.astype(np.float32), vp=vp.astype(np.float32), adv=adv.astype(np.float32), ret=(vp + adv).astype(np.float32))


@functools.lru_cache(maxsize=None)
def ppo_reference(dtype="float64"):
    """One minibatch update of the PPO case in `dtype` (forward, loss, gradients by autograd), computed once and shared (read-only).
    The loss inputs come from the float64 forward."""
    sd = state_dict(**{k: PPO[k] for k in ("backbone", "vis", "normalize", "rnn")})
    inp = ppo_rollout()
    z = np.zeros(PPO["T"] * PPO["N"])
    with policy() as g:
        r64 = g.update(sd, inp, ppo_loss_inputs(z, z), PPO["rnn"], train=False)
        return g.update(sd, inp, ppo_loss_inputs(r64["value"], r64["logp"]), PPO["rnn"], dtype, train=False)


# ---- the VO model
def vo_spec(backbone=None, W=None, H=None):
    cfg = ms.config_from_kwargs(observation_space=VO["space"], observation_size=(W or VO["W"], H or VO["H"]), hidden_size=VO["hidden"],
                                backbone=backbone or VO["backbone"], normalize_visual_inputs=True, output_dim=3,
                                discretized_depth_channels=VO["dd_bins"])
    return cfg, ms.state_dict_spec(cfg)


def vo_inputs():
    """(state_dict, observation pairs) of the VO case, as tests/golden/gen_golden.py's model fixtures draw them."""
    sd = synth.make_state_dict(vo_spec()[1], seed=VO["seed"])
    obs = synth.make_obs_pairs(VO["B"], VO["H"], VO["W"], observation_space=list(VO["space"]), dd_bins=max(VO["dd_bins"], 1), seed=VO["seed"])
    return sd, obs


def vo_forward(sd, obs, dtype="float64"):
    """vo_cnn's eval forward on a state_dict -> [B, 3] float64."""
    dt = getattr(torch, dtype)
    params = {k: torch.as_tensor(np.asarray(v)).to(dt) for k, v in sd.items()}
    cfg, _ = vo_spec()
    with torch.no_grad():
        out, _ = encoder_forward(params, params, {k: torch.as_tensor(v) for k, v in obs.items()}, ngroups=cfg.ngroups, train=False, dtype=dt)
    return out.double().numpy()


# ---- the batch-regime pool (tests/test_gpu_backbone_regimes.py and tests/test_backbone_regimes_host.py)
POOL_P, POOL_A = 31, 12                                   # a prime pool and a stride coprime to it
REGIME_TOL = 2e-4                                         # of each position's own scale (tests/test_gpu_policy.py's bound)
REF32_TOL = REGIME_TOL / 4                                # what the float32 restatement itself has to stay under on the pool
EVEN_H, EVEN_W = 128, 128                                 # policy frames with even maps all the way down: 16x16, 8x8, 4x4, 2x2
ZERO_BORDER = (3, 14, 22, 29)                             # pool samples with a zero border of 2, 4, 6, 8 pixels
FLAT = dict(constant=7, two_level=19, ripple=27)         # pool samples with (nearly) no variance: see _pool_edges
ZERO_MASK = (0, 5, 17, 26)                                # pool samples whose episode starts (mask 0) in the policy pool
VO_TAPS = ("layer1.0", "layer1.1", "layer2.0", "layer2.1", "layer3.0", "layer3.1", "layer4.0", "layer4.1")
POLICY_KEYS = ("encoder", "features", "hidden", "logits", "value")
POSITION_AXIS = {"hidden": 1}                             # the recurrent state is [states, B, hidden]; everything else [B, ...]


def positions(B):
    """Pool sample of every position of a batch of B: (A i + c_B) mod P.  Two positions closer than P hold different samples, and the
    offset c_B differs between any two batches the regime modules use."""
    return (POOL_A * np.arange(B) + 7 * B + 22 * (B // POOL_P)) % POOL_P


def _pool_edges(frames):
    """Zero borders and flat frames, in place, on {name: [P,H,W,C]} (depth in 0..1, rgb in 0..255).  Flat frames give tiny GroupNorm
    variances: one constant frame (depth 0.25, rgb 64), one of two constant halves, one with a 1 - 2 % ripple around a constant.
    (A constant frame is ill-conditioned at every level: the float32 restatement sits at 2e-5 .. 4e-4 of scale on it against 2 - 6e-6
    on a textured frame, depending on the level and the model; (0.25, 64) is the level that stays below 3e-5 on every model of the
    regime modules, the others were measured at 0, 0.1, 0.45, 0.6, 0.8 and 1.)"""
    for n, i in enumerate(ZERO_BORDER):
        z = 2 * (n + 1)
        for v in frames.values():
            v[i, :z] = 0
            v[i, -z:] = 0
            v[i, :, :z] = 0
            v[i, :, -2 * z:] = 0
    for k, v in frames.items():
        rgb = k == "rgb"
        half = v.shape[1] // 2
        v[FLAT["constant"]] = 64 if rgb else 0.25
        v[FLAT["two_level"], :half] = 60 if rgb else 0.3
        v[FLAT["two_level"], half:] = 200 if rgb else 0.7
        r = v[FLAT["ripple"]].astype(np.float64)
        v[FLAT["ripple"]] = (128 + 0.02 * (r - 128)) if rgb else (0.45 + 0.01 * (r - 0.5))


def policy_pool(H=H, W=W, seed=86):
    """POOL_P distinct act-step samples: rgb uint8 [P,H,W,3], depth [P,H,W,1], goal, prev, mask (zero at ZERO_MASK) and a non-zero
    incoming LSTM state [2 L, P, HIDDEN]; ZERO_BORDER frames with a zero border, FLAT frames flat.  The value is one number per
    position, judged on its own scale: the seed is the first of 81, 84, 85, 86, 87 (float64 restatement, CPU) with no position's
    |value| below 9e-3 on any model of the regime modules."""
    rgb, depth, goal, prev, _ = synth.make_policy_rgbd_inputs(H, W, POOL_P, 1, seed, N_ACT)[0]
    _pool_edges({"rgb": rgb, "depth": depth})
    mask = np.ones(POOL_P, np.float32)
    mask[list(ZERO_MASK)] = 0.0
    h0 = synth.uniform(seed, "h0", (LAYERS, POOL_P, HIDDEN), -1.0, 1.0)
    c0 = synth.uniform(seed, "c0", (LAYERS, POOL_P, HIDDEN), -3.0, 3.0)
    return dict(rgb=rgb, depth=depth, goal=goal, prev=prev, mask=mask, hidden=np.concatenate([h0, c0]).astype(np.float32))


def vo_pool(H, W, seed=82):
    """POOL_P distinct observation pairs of the VO case's modalities: float16-rounded depth in the first half, dense float32 depth in the
    second, the same edge frames as policy_pool."""
    half = POOL_P // 2
    a = synth.make_obs_pairs(half, H, W, observation_space=list(VO["space"]), dd_bins=1, seed=seed, depth_fp16=True)
    b = synth.make_obs_pairs(POOL_P - half, H, W, observation_space=list(VO["space"]), dd_bins=1, seed=seed, depth_fp16=False, start=half)
    pool = {k: np.concatenate([a[k], b[k]]) for k in a}
    _pool_edges(pool)
    return pool


@functools.lru_cache(maxsize=None)
def pool_state_dict(backbone, vis, normalize, H=H, W=W):
    """Synthetic LSTM-policy weights at a frame size of the regime modules; shared, read-only."""
    return synth.make_state_dict(spec(backbone=backbone, vis=tuple(vis), normalize=normalize, rnn="LSTM", H=H, W=W), seed=WEIGHT_SEED)


def position_err(got, want, axis=0):
    """max |got - want| / (max |want| + 1e-6) of every position along `axis`, each on its own scale -> float64 numpy [positions].
    Takes numpy arrays or torch tensors (computed where `want` lives); a non-finite value gives a non-finite error."""
    want = torch.as_tensor(want)
    got = torch.as_tensor(got).to(device=want.device, dtype=torch.float64).reshape(want.shape)
    want = want.to(torch.float64)
    d = (got - want).abs().movedim(axis, 0).reshape(want.shape[axis], -1).amax(1)
    s = want.abs().movedim(axis, 0).reshape(want.shape[axis], -1).amax(1)
    return (d / (s + 1e-6)).cpu().numpy()


def policy_pool_reference(sd, pool, vis, dtype="float64"):
    """One restatement act step over the pool (every sample is independent of the others: GroupNorm, the SE squeeze and the recurrent
    core work per sample) -> {POLICY_KEYS: float64 numpy}."""
    r = policy_step(sd, {k: pool[k] for k in vis}, pool["goal"], pool["prev"], pool["mask"], pool["hidden"], "LSTM", dtype)
    return {k: r[k] for k in POLICY_KEYS}


def vo_pool_reference(sd, cfg, pool, taps, dtype="float64"):
    """The VO restatement over the pool -> {'pose': [P,3], 'encoder' and each of `taps`: NHWC float64 numpy, as model.tap returns them}."""
    dt = getattr(torch, dtype)
    params = {k: torch.as_tensor(np.asarray(v)).to(dt) for k, v in sd.items()}
    rec = {}
    with torch.no_grad():
        out, _ = encoder_forward(params, params, {k: torch.as_tensor(v) for k, v in pool.items()}, ngroups=cfg.ngroups, train=False,
                                 dtype=dt, record=rec)
    res = {"pose": out.double().numpy()}
    for k in tuple(taps) + ("encoder",):
        res[k] = rec[k].permute(0, 2, 3, 1).double().contiguous().numpy()
    return res


def pool_sequence(pool, T=4, N=32, seed=83):
    """A T-major evaluate_actions input of T x N depth frames drawn from the pool by positions(T N): every episode starts at t = 0,
    every fifth environment resets again at t = T / 2; a non-zero incoming state."""
    M = T * N
    idx = positions(M)
    masks = np.ones((T, N), np.float32)
    masks[0] = 0.0
    masks[T // 2, 1::5] = 0.0
    h0 = synth.uniform(seed, "h0", (LAYERS, N, HIDDEN), -1.0, 1.0)
    c0 = synth.uniform(seed, "c0", (LAYERS, N, HIDDEN), -3.0, 3.0)
    return dict(depth=pool["depth"][idx], goal=pool["goal"][idx], prev=pool["prev"][idx], masks=masks.reshape(-1),
                actions=(synth.bits(seed, "taken", M) % np.uint64(N_ACT)).astype(np.int64),
                hidden=np.concatenate([h0, c0]).astype(np.float32), T=T, N=N)


def sequence_reference(sd, inp, dtype="float64"):
    """The restatement's evaluate_actions forward -> value [M], logp [M], entropy [1], hidden [2 L, N, HIDDEN] (float64 numpy)."""
    dt = getattr(torch, dtype)
    params, bufs = G.split(sd)
    with policy() as g, torch.no_grad():
        value, logp, entropy, hidden = g.forward(G.R.leaves(params, dt), bufs, inp, dt, "LSTM", False)[:4]
    f = lambda t: t.double().numpy()
    return dict(value=f(value), logp=f(logp), entropy=f(entropy).reshape(1), hidden=f(hidden))


def worst_ref32(ref64, ref32):
    """Worst per-position error of the float32 restatement against the float64 one over a pool reference -> {key: error}."""
    return {k: float(position_err(ref32[k], v, POSITION_AXIS.get(k, 0)).max()) for k, v in ref64.items()}


if __name__ == "__main__":
    import sys
    if "--seeds" in sys.argv:
        sd = state_dict(**{k: PPO[k] for k in ("backbone", "vis", "normalize", "rnn")})
        z = np.zeros(PPO["T"] * PPO["N"])
        with policy() as g:
            r = g.update(sd, ppo_rollout(), ppo_loss_inputs(z, z), PPO["rnn"], train=False)
        print("PPO_LOSS_SEED =", next(s for s in range(200) if G.census_ok(r["value"], r["logp"], ppo_loss_inputs(r["value"], r["logp"], seed=s), 1e-4)))
    else:
        for case in CASES:
            r64, r32 = run_case(case), run_case(case, "float32")
            worst = max(float(np.abs(a[k] - b[k]).max() / np.abs(a[k]).max()) for a, b in zip(r64, r32)
                        for k in ("features", "hidden", "logits", "value", "encoder"))
            print(f"{case} ({CASES[case]['backbone']}): float32 restatement vs float64, worst error / scale {worst:.2e}")
