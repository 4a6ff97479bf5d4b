"""GPU (-m gpu): the default inference forward at 341x192 against the fp64 oracle at EVERY position of batches on both sides of
every batch-size threshold of the kernel selection — pose and the 512-wide hidden features (pnvo_forward_features, what the
navigation policy consumes) — plus the dual bf16 forward at 256 pairs (BASELINE configs[2]) at every position of both outputs.

Pool.  P = 61 distinct pairs (a prime: no power of two is a multiple of it), uploaded once: float16-rounded and dense float32
depth, zero-bordered frames, near-empty and dense top-down views.  Position i of a batch of B pairs holds pool pair
(A i + c_B) mod P with A = 23 (coprime to P): two positions closer than P hold different pairs, so a tile, band, workgroup or
sample stride of 1, 2, 4, ... 32 that reads or writes the wrong sample changes the pair a position is compared against.  Each
pool pair's fp64 pose and hidden vector is computed once per module (oracle.forward_pairs_parallel, one pair per host thread).

Batches (default options, num_cus = 256 on the MI355X; the predicates in pointnav-vo_amd/csrc):
    1 2 3 | 4        pnvo_small_usable: the persistent small-batch kernel up to small_max = 3 pairs (48 x 86 pooled map)
    5 7 | 8 9        stem_rs_takes: 96 x 171 stem output = 132 tiles of 8 x 16 per pair, resident weights from
                     4 tiles x 256 workgroups = 1024 tiles: 8 pairs on
    16 17 32 33      fine plans (conv_x3_plan: regular plan < 224 workgroups; fine plan >= 48 workgroups), K split behind
                     >= 128 input channels (x3_ksplit): the deep stages of 6-48 pairs
    48 | 49          fc_rows_usable: the hidden layer and the head on fc_rows.hip up to 48 samples
    63 | 64 65       conv_rows32_candidate: layer1's 32 -> 32 convs on the row-streaming kernel once B * bands >= 256 (48-row maps:
                     up to 4 bands of 12 rows: 64 pairs on), 2 bands at 128, 1 band at 256
    100 128 129      conv_x3 on every 3x3 conv (>= 192 workgroups), fused pool and block tails, downsample rides
    199 | 200        the eight-wave (3,1) tiles of the 256-channel 6 x 11 convs (one tile per pair: ntiles >= 200)
    255 256          configs[1]'s batch and one short of it (a partial last band / tile row at every stage)
The sweep must reach the smallnet, x2 and an fp32 family (pnvo_layer_kernel); the coverage test fails if a threshold moves
so that it no longer does.

Criteria per batch: every position's pose within 1e-4 of the fp64 norm (pair_rel_err, the project's contract); every position's
hidden vector within FEAT_TOL relative L2 of the fp64 vector; a second call bit-identical to the first (pose and features).
Measured on the MI355X (worst over all positions of all batches of the regime, relative to the fp64 norm):
    regime                              pose err   feature err
    1-3    persistent small-batch kernel 8.9e-7     9.3e-7
    4-48   per-layer, fine plans, fc_rows 2.7e-6     1.4e-6
    49-256 conv_x3 / conv_rows / 8 waves  4.0e-6     1.6e-6
FEAT_TOL = 1e-5: six times the worst measured feature error (an error confined to a few of the 512 channels shrinks on its way to
the 3-wide pose; the feature bound sees it at full size).  Dual bf16 at 256: ||out - ref|| <= 1e-2 + 4e-2 ||ref|| per pair per
model (tests/test_gpu_bf16.py's criterion; worst pair measured at 0.92 of it); model A's output equals its single bf16 forward
bit for bit.
Wall time of the module on the MI355X host (16 CPUs): 7 s, the fp64 oracle of the 2 x 61 pool pairs included.

Mutations this module was checked against (in bounds, not committed): (1) one channel in 32 of the eight-wave 256-channel convs
scaled by 1 + 1e-3 for pairs 128 on: fails batches 255 and 256 (pose 1.0e-3, features 3.2e-4); (2) the epilogue of conv_rows32's
second band scaled by 1 + 1e-3: fails batches 64-255; (3) the hidden rows of samples 5 and 37 swapped in fc_rows: fails batch 48.
(A uniform scale of a whole per-sample conv output is not a usable mutation: the GroupNorm behind it cancels it.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import pair_rel_err
from oracle import oracle
from pointnav_vo_amd import _lib, model_spec as ms, synth, vo_cnn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the headline model and its options)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

P, A = 61, 23
BATCHES = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 32, 33, 48, 49, 63, 64, 65, 100, 128, 129, 199, 200, 255, 256]
POSE_TOL = 1e-4
FEAT_TOL = 1e-5
BF16_ABS, BF16_REL = 1e-2, 4e-2


def positions(B):
    """Pool pair of every position of a batch of B: (A i + c_B) mod P, the offset c_B differing from batch to batch."""
    return (A * np.arange(B) + 7 * B) % P


def make_pool():
    """P distinct pairs: float16-rounded depth (dataset-style) and dense float32 depth (simulator-style), four of them with a zero
    border in depth and rgb (depth 0: the one-hot's first bin), four with a near-empty top-down view and two with a dense one."""
    H, W, S = bench.H, bench.W, bench.SPACE
    half = P // 2
    a = synth.make_obs_pairs(half, H, W, observation_space=S, dd_bins=bench.BINS, seed=31, depth_fp16=True)
    b = synth.make_obs_pairs(P - half, H, W, observation_space=S, dd_bins=bench.BINS, seed=32, depth_fp16=False, start=half)
    pool = {k: np.concatenate([a[k], b[k]]) for k in a}
    for n, i in enumerate((3, 20, 41, 57)):                        # zero borders of 2..8 pixels, prev and cur frame
        z = 2 * (n + 1)
        for k in ("depth", "rgb"):
            v = pool[k][i]
            v[:z] = 0
            v[-z:] = 0
            v[:, :z] = 0
            v[:, -2 * z:] = 0
        d = pool["depth"][i]
        pool["discretized_depth"][i] = np.concatenate([synth.onehot_depth(d[..., 0], bench.BINS),
                                                       synth.onehot_depth(d[..., 1], bench.BINS)], axis=-1)
    sparse = synth.make_obs_pairs(4, H, W, observation_space=S, dd_bins=bench.BINS, seed=33, tdv_sparsity=0.995)
    dense = synth.make_obs_pairs(2, H, W, observation_space=S, dd_bins=bench.BINS, seed=34, tdv_sparsity=0.0)
    for j, i in enumerate((9, 30, 44, 52)):
        pool["top_down_view"][i] = sparse["top_down_view"][j]
    for j, i in enumerate((13, 47)):
        pool["top_down_view"][i] = dense["top_down_view"][j]
    return pool


def reference(sd, pool, ngroups, taps=("hidden",)):
    """fp64 oracle pose (and taps) of every pool pair, one pair per host thread."""
    return oracle.forward_pairs_parallel(sd, pool, ngroups=ngroups, threads=min(oracle.usable_cores(), 16), dtype=np.float64,
                                         taps=taps)


@pytest.fixture(scope="module")
def ctx():
    pool = make_pool()
    model, sd = bench.build_model(DEV, seed=0)
    pose, taps = reference(sd, pool, model.cfg.ngroups)
    dpool = {k: torch.from_numpy(v).to(DEV) for k, v in pool.items()}
    return dict(pool=pool, dpool=dpool, model=model, sd=sd, pose=pose, hidden=taps["hidden"])


def batch_of(dpool, idx):
    it = torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(DEV)
    return {k: v.index_select(0, it).contiguous() for k, v in dpool.items()}


def features(model, obs):
    """pnvo_forward_features: the forward stopped behind visual_fc's Linear + ReLU -> [B, hidden]."""
    model._ensure_handle(DEV)
    model._sync_weights()
    ptrs, B, keep = vo_cnn._obs_ptrs(model, obs, DEV)
    hid = torch.empty((B, model.cfg.hidden), device=DEV, dtype=torch.float32)
    with torch.cuda.device(DEV):
        stream = torch.cuda.current_stream(DEV).cuda_stream
        _lib.check(_lib.lib.pnvo_forward_features(model._handle, ptrs[0], ptrs[1], ptrs[2], ptrs[3], None, int(B),
                                                  C.c_void_p(hid.data_ptr()), C.c_void_p(stream)), model._handle)
    return hid


def conv_names(model):
    return [n[:-len(".weight")] for n, s in ms.state_dict_spec(model.cfg)
            if ".backbone.layer" in n and n.endswith(".weight") and len(s) == 4]


@pytest.mark.parametrize("B", BATCHES)
def test_every_position_matches_the_fp64_oracle(ctx, B):
    model = ctx["model"]
    idx = positions(B)
    assert len(set(idx[: min(B, P)].tolist())) == min(B, P)
    obs = batch_of(ctx["dpool"], idx)
    with torch.no_grad():
        out = [model(obs).clone() for _ in range(2)]
        hid = [features(model, obs).clone() for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[1]) and torch.equal(hid[0], hid[1]), "a repeated call is not bit-identical"
    pose_err = pair_rel_err(out[0].cpu().numpy(), ctx["pose"][idx])
    ref_h = ctx["hidden"][idx]
    feat_err = np.linalg.norm(hid[0].double().cpu().numpy() - ref_h, axis=1) / np.maximum(np.linalg.norm(ref_h, axis=1), 1e-30)
    fams = sorted({model.layer_kernel(n, B)[0] for n in conv_names(model)})
    print(f"B={B:4d} pose err max {pose_err.max():.2e} (pos {int(pose_err.argmax())}) | feature err max {feat_err.max():.2e} "
          f"(pos {int(feat_err.argmax())}) median {np.median(feat_err):.2e} | conv families {','.join(fams)}")
    assert np.isfinite(pose_err).all() and np.isfinite(feat_err).all()
    bad = np.flatnonzero(pose_err >= POSE_TOL)
    assert bad.size == 0, ("pose", B, bad.tolist()[:16], float(pose_err.max()))
    bad = np.flatnonzero(feat_err >= FEAT_TOL)
    assert bad.size == 0, ("features", B, bad.tolist()[:16], float(feat_err.max()))


def test_the_sweep_covers_every_conv_family():
    """The batches above reach the persistent small-batch kernel, the float16-piece conv_x3 family and a float32 family
    (pnvo_layer_kernel); if a threshold moves so that the sweep stops reaching one, this fails instead of testing less."""
    model, _ = bench.build_model(DEV, seed=0)
    seen = {}
    for B in BATCHES:
        for n in conv_names(model):
            seen.setdefault(model.layer_kernel(n, B)[0], set()).add(B)
    print("families:", {k: sorted(v) for k, v in seen.items()})
    assert "smallnet" in seen and "x2" in seen, seen.keys()
    assert any(k.startswith("fp32") for k in seen), seen.keys()


ENGAGING = [7, 8, 16, 48, 64, 128, 200, 256]      # per-layer kernels, resident stem, fine plans, last fc_rows batch, rows form, conv_x3 everywhere, eight waves, configs[1]


def test_layer_families_are_what_the_planner_describes(ctx):
    """At each regime's engaging batch: the family pnvo_layer_kernel reports for every residual-stage conv is the one the conv_x3
    planner takes for that layer's problem (pnvo_conv_x3_describe), and that line is the one recorded in
    tests/golden/conv_x3_plans.txt from the planner before the problem -> plan -> table refactor.  No forward runs."""
    import test_conv_x3_plan as plans
    model = ctx["model"]
    lines, index = plans.read_golden()
    grid = plans.grid()
    pieces = int(model.get_option("pieces"))
    convs = ms.conv_plan(model.cfg)
    for B in ENGAGING:
        assert B in plans.BATCHES and B in BATCHES
        for i, cd in enumerate(convs):
            if i == 0:
                continue
            fam = model.layer_kernel(cd.name, B)[0]
            np_ = 3 if fam == "x3" else pieces

            def line_of(c, ds):
                H, W, CIN, Ho, Wo, COUTP, ks, stride, _ = plans.fwd_shape(c)
                q = plans.problem_of(B=B, H=H, W=W, CIN=CIN, Ho=Ho, Wo=Wo, COUTP=COUTP, ks=ks, stride=stride, np=np_, ds=ds)
                line = plans.describe(q)
                assert line == plans.golden_line(lines, index, grid, q), (cd.name, B, line)
                return line

            want = None
            if cd.k == 1:                               # a downsample conv (plan order c1, c2, downsample): rides on c1 where c1 carries it
                if line_of(convs[i - 2], 1) != "none" and np_ == 2:
                    want = "x2-rides"
            if want is None:
                want = "fp32" if line_of(cd, 0) == "none" else ("x2" if np_ == 2 else "x3")
            assert fam == want or (want == "fp32" and fam.startswith("fp32")), (cd.name, B, fam, want)


def test_dual_bf16_forward_at_256_every_position(ctx):
    """configs[2]: two action models (seeds 0 and 1) in one bf16 dual forward over 256 pairs of the pool layout; model B sees
    the swapped pair.  Every position of both outputs within the bf16 criterion of the fp64 oracle; model A's output equals
    its single bf16 forward bit for bit."""
    ma, _ = bench.build_model(DEV, seed=0)
    mb, sdb = bench.build_model(DEV, seed=1)
    ma.set_precision("bfloat16")
    mb.set_precision("bfloat16")
    swapped = {k: np.concatenate([v[..., v.shape[-1] // 2:], v[..., : v.shape[-1] // 2]], axis=-1) for k, v in ctx["pool"].items()}
    ref_b = reference(sdb, swapped, mb.cfg.ngroups, taps=None)
    B = 256
    idx = positions(B)
    obs = batch_of(ctx["dpool"], idx)
    with torch.no_grad():
        oa, ob = vo_cnn.dual_forward(ma, mb, obs)
        single = ma(obs)
    torch.cuda.synchronize()
    assert torch.equal(oa, single)
    worst = 0.0
    for name, got, want in (("A", oa, ctx["pose"][idx]), ("B", ob, ref_b[idx])):
        err = np.linalg.norm(got.double().cpu().numpy() - want, axis=1)
        bound = BF16_ABS + BF16_REL * np.linalg.norm(want, axis=1)
        worst = max(worst, float((err / bound).max()))
        bad = np.flatnonzero(~(err <= bound))
        assert bad.size == 0, (name, bad.tolist()[:16], float((err / bound).max()))
    print(f"dual bf16 at 256: worst err / bound {worst:.3f}")
