"""GPU (-m gpu): the Bottleneck / ResNeXt / SE-ResNeXt backbones at the batch sizes where their dense convs leave the fp32-MFMA family
for conv_x3's three-bf16-piece form, every position of every batch against the float64 restatement of tests/backbone_reference.py.
Why.  tests/test_gpu_policy_backbones.py runs these models at 2, 5 and 9 frames, where every dense conv is on the fp32-MFMA family.  The
frozen-encoder PPO update encodes T N frames in one call and profiles/policy_backbones.md times a 256-frame encoder: there the dense
3x3 convs, the 1x1 stride-2 downsample convs (CIN 512 / 1024, COUTP up to 1024: wider than anything resnet18 has) and the compression
conv run on conv_x3_kernel in the three-piece form (x3_two_pieces is false for every bottleneck model), the 1x1 stride-1 convs on
conv_mfma.hip with K up to 1024, and conv_group_kernel / se_gate_kernel over thousands of workgroups.

Pool (tests/backbone_reference.py, shared with tests/test_backbone_regimes_host.py).  P = 31 distinct samples, uploaded once; position
i of a batch of B holds pool sample (12 i + c_B) mod 31 with a different offset c_B for every batch used here, so a wrong sample,
tile, slab or slot stride changes what a position is compared against.  Four frames carry a zero border; three are flat (one
constant, one of two constant halves, one with a 1 - 2 % ripple): tiny GroupNorm variances.  (A constant frame is ill-conditioned: the
float32 restatement alone sits at 2e-5 .. 4e-4 of scale on one, depending on its level; the pool keeps the level that stays below
3e-5 on every model here, and the host module fails if the float32 restatement leaves a quarter of the bound on the committed pool.)
The float64 restatement (BR.encoder_forward / BR.policy_step) is computed once per pool sample per backbone per model, never per batch.

  (a) VO model (the handle with layer_kernel and tap), rgb + depth frames of 68 x 52 — the policy's maps behind the stem, 13x17, 7x9,
      4x5, 2x3 — at BATCHES for resnet50, resneXt50 and se_resneXt50, at 64 and 256 for resnet101, se_resnet50 and se_resneXt101: the
      pose, the block taps layer1.0 .. layer4.1 and the last block, and the compression output at every position; the second call
      bit-identical; the kernel families printed per batch.
  (b) Coverage: on the default options every dense 3x3 and 1x1 stride-2 conv reports x3 at 256 and an fp32 family at 9, its first x3
      batch of the sweep follows a batch where it is not on x3, the four grouped convs report `group`.  First planned batches at 256
      CUs: layer4.0.downsample 24; layer3.0.downsample and resneXt's layer4.1/4.2 48; compression 64; layer1.*, layer2.0.downsample,
      resnet50's layer4.* and resneXt's layer3.* 96; every other dense 3x3 192.  No option is set anywhere in this module.
  (c) Policy on frames of 104 x 136 at 32, 64, 128 and 256: resnet50 and se_resneXt50 on depth, se_resneXt50 on uint8 rgb + depth with
      normalize_visual_inputs — encoder, features, hidden, logits and value at every position, a non-zero incoming state, zero masks
      at four pool samples; and a frozen-encoder se_resneXt50 evaluate_actions with T = 4, N = 32 (128 frames in one encode, every
      episode starting at t = 0, every fifth one again at t = 2): value, logp, entropy and the outgoing state.
  (d) Even maps: policy frames of 128 x 128 (16x16, 8x8, 4x4, 2x2: the grouped convs' pixel counts 256, 64, 16 and 4 are whole slots,
      one whole tile and less than a tile; every stride-2 conv reads an even input) on se_resneXt50 and resneXt50 at 3 and 64, and the
      VO model at 64 x 64 with the taps layer1.0 .. layer4.0.  The library serves this geometry (nothing is refused).

Criterion: every position on its own scale, max |got - want| / (max |want| + 1e-6) < 2e-4 over that position's tensor (the bound of
tests/test_gpu_policy.py), taps included; no position skipped or masked; non-finite values fail.  Measured on the MI355X, worst
position over the batches of the regime, next to the float32 restatement's own error on the same pool (pose / worst tap / encoder):
    VO 68x52       none on x3 (9, 23)       some on x3 (24 .. 191)    all on x3 (192 .. 256)    float32 restatement
    resnet50       1.8e-6 2.8e-6 1.9e-6     3.3e-6 5.7e-6 4.7e-6      3.7e-6 5.7e-6 5.1e-6      1.9e-5 2.9e-5 2.5e-5
    resneXt50      1.4e-6 1.5e-6 1.6e-6     2.4e-6 3.8e-6 3.5e-6      2.6e-6 3.2e-6 3.3e-6      8.6e-6 1.6e-5 9.3e-6
    se_resneXt50   1.7e-6 1.3e-6 1.6e-6     4.1e-6 2.5e-6 3.1e-6      4.1e-6 2.5e-6 3.1e-6      6.5e-6 1.6e-5 8.2e-6
    resnet101      -                        2.7e-6 5.7e-6 4.0e-6      3.5e-6 6.3e-6 5.3e-6      1.3e-5 3.1e-5 2.1e-5
    se_resnet50    -                        5.6e-6 3.5e-6 3.5e-6      6.5e-6 4.1e-6 3.7e-6      1.9e-5 1.9e-5 1.8e-5
    se_resneXt101  -                        2.5e-6 2.1e-6 2.6e-6      3.0e-6 2.3e-6 2.8e-6      3.1e-6 1.6e-5 6.7e-6
    VO 64x64 se_resneXt50: B = 3 9.5e-7 1.3e-6 1.0e-6, B = 64 4.2e-6 1.8e-6 2.3e-6 (float32 9.6e-6 1.4e-5 7.5e-6);
             resneXt50:    B = 3 1.6e-6 1.5e-6 1.2e-6, B = 64 5.6e-6 2.8e-6 2.1e-6 (float32 1.3e-5 1.0e-5 6.7e-6)
    policy (worst of B = 32 .. 256; encoder / features / hidden / logits / value, float32 restatement in brackets)
    resnet50 104x136               5.6e-6 5.3e-6 7.6e-6 4.5e-6 1.3e-5   (1.9e-5 9.9e-6 1.3e-5 6.7e-6 1.1e-5)
    se_resneXt50 104x136           3.0e-6 2.6e-6 3.8e-6 5.2e-6 4.7e-6   (7.3e-6 2.5e-6 6.4e-6 3.6e-6 3.2e-6)
    se_resneXt50 rgb+depth         3.7e-6 2.5e-6 3.9e-6 8.7e-6 8.9e-6   (1.2e-5 2.4e-6 4.5e-6 7.6e-6 3.2e-6)
    se_resneXt50 128x128 (3, 64)   3.1e-6 1.4e-6 2.9e-6 5.0e-6 2.5e-5   (6.3e-6 2.5e-6 4.7e-6 6.3e-6 8.4e-6)
    resneXt50 128x128 (3, 64)      2.8e-6 1.9e-6 3.5e-6 5.6e-6 4.6e-6   (9.3e-6 3.8e-6 4.9e-6 8.3e-6 1.4e-5)
    evaluate_actions T = 4, N = 32: value 3.1e-6, logp 4.3e-7, entropy 1.2e-8, hidden 2.8e-6 (9.3e-6 6.6e-7 1.2e-8 8.8e-6)
The device sits at or below the float32 restatement everywhere but on single numbers judged on their own scale (the value: one
scalar per position, 2.5e-5 at the position whose |value| is smallest); a later change can tighten against this record.  No bug was found.
Wall time of the module on the MI355X host (16 CPUs): 12.5 s for its 90 tests, the float64 and float32 references included (the
resnet18 module: 7 s for 27); the slowest test takes 1.0 s.

Mutations this module was checked against (in bounds, one at a time, not committed):
  1. one output channel in 32 of conv_x3_kernel's three-piece epilogue scaled by 1 + 1e-3 for samples 64 on: every batch above 64 fails
     on all six backbones (VO 65 .. 256, pose 1.2 - 7.4e-4, taps 5.3 - 8.6e-4), the policy at 128 and 256 and the 128-frame
     evaluate_actions; every batch up to 64 passes.
  2. the second pixel tile's accumulator of conv_group_kernel scaled by 1 + 1e-3 for slot >= 1: every batch of every ResNeXt model
     fails, 3 and 9 included, on both geometries (taps 1.0 - 1.5e-3); resnet50, resnet101 and se_resnet50 pass.
  3. the last pixel slice dropped from se_gate_kernel's squeeze for samples 32 on (where the squeeze has more than one slice): every SE
     model fails from 33 on (VO), at 64, 128, 256 (policy), at 64 (even maps) and in evaluate_actions (errors 0.15 - 0.55 of scale);
     9 .. 32 and the models without SE pass.
(A uniform scale of a whole per-sample conv output is not a usable mutation: the GroupNorm behind it cancels it.)
"""
import time

import numpy as np
import pytest
import torch

import backbone_reference as BR
import test_conv_x3_plan as plans
import test_gpu_policy_backbones as PB
from pointnav_vo_amd import model_spec as ms, synth
from pointnav_vo_amd.vo_cnn import VisualOdometryCNNBase

pytestmark = pytest.mark.gpu
DEV = PB.DEV
GOAL = BR.GOAL
TOL = BR.REGIME_TOL

FULL = ("resnet50", "resneXt50", "se_resneXt50")           # swept over BATCHES
SPOT = ("resnet101", "se_resnet50", "se_resneXt101")       # at SPOT_BATCHES only
# 9 | 23 24 | 31 32 33 | 47 48 | 63 64 65 | 95 96 | 127 128 129 | 191 192 | 255 256: both sides of the first planned batch of every
# conv (24, 48, 96, 192 at 256 CUs: tests/test_backbone_regimes_host.py reads them off the planner) and of every power of two
BATCHES = [9, 23, 24, 31, 32, 33, 47, 48, 63, 64, 65, 95, 96, 127, 128, 129, 191, 192, 255, 256]
SPOT_BATCHES = (64, 256)
VO_W, VO_H = 68, 52                                        # the policy's maps behind the stem: 13x17, 7x9, 4x5, 2x3
EVEN_VO = 64                                               # 16x16, 8x8, 4x4, 2x2
EVEN_BATCHES = (3, 64)
POLICY_BATCHES = (32, 64, 128, 256)
POLICY_CASES = [("resnet50", False), ("se_resneXt50", False), ("se_resneXt50", True)]
EVEN_POLICY = ("se_resneXt50", "resneXt50")


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def fmt(errs, ref32):
    return "  ".join(f"{k} {float(np.max(e)):.1e} (f32 {ref32[k]:.1e})" for k, e in errs.items())


def judge(what, errs):
    """Every position of every output below TOL of its own scale; none skipped, non-finite values fail."""
    for k, e in errs.items():
        e = np.asarray(e)
        bad = np.flatnonzero(~(np.isfinite(e) & (e < TOL)))
        assert bad.size == 0, (what, k, "positions", bad.tolist()[:16], "worst", float(np.nanmax(e)) if np.isfinite(e).any() else None)


# ---------------------------------------------------------------------------------------------------------------- fixtures
class VoCase:
    """A VO model of one backbone at one frame size, its float64 pool reference on the device, and the float32 restatement's error."""

    def __init__(self, backbone, W, H, taps, pool):
        self.backbone, self.taps = backbone, tuple(taps)
        self.cfg, spec = BR.vo_spec(backbone, W, H)
        sd = synth.make_state_dict(spec, seed=BR.VO["seed"])
        ref = BR.vo_pool_reference(sd, self.cfg, pool, self.taps)
        self.ref32 = BR.worst_ref32(ref, BR.vo_pool_reference(sd, self.cfg, pool, self.taps, "float32"))
        assert max(self.ref32.values()) < BR.REF32_TOL, (backbone, self.ref32)
        v = BR.VO
        model = VisualOdometryCNNBase(observation_space=list(v["space"]), observation_size=(W, H), hidden_size=v["hidden"], backbone=backbone,
                                      normalize_visual_inputs=True, output_dim=3, discretized_depth_channels=v["dd_bins"])
        assert list(model.state_dict().keys()) == list(sd.keys())
        model.load_state_dict({k: torch.from_numpy(np.array(t)) for k, t in sd.items()})
        self.model = model.to(DEV).eval()
        self.dref = {k: gpu(t) for k, t in ref.items()}
        self.dpool = {k: gpu(t) for k, t in pool.items()}
        self.convs = [cd for cd in ms.conv_plan(self.cfg)[1:]]

    def families(self, B):
        return {cd.name: self.model.layer_kernel(cd.name, B)[0] for cd in self.convs}


class PolicyCase:
    """A navigation policy of one backbone at one frame size with its float64 pool reference on the device."""

    def __init__(self, backbone, rgbd, H, W, pool):
        self.vis, self.normalize = (("rgb", "depth"), True) if rgbd else (("depth",), False)
        self.sd, self.pool = BR.pool_state_dict(backbone, self.vis, self.normalize, H, W), pool
        ref = BR.policy_pool_reference(self.sd, pool, self.vis)
        self.ref32 = BR.worst_ref32(ref, BR.policy_pool_reference(self.sd, pool, self.vis, "float32"))
        assert max(self.ref32.values()) < BR.REF32_TOL, (backbone, rgbd, self.ref32)
        self.pol = PB.make_policy(self.sd, backbone, self.vis, "LSTM", self.normalize, H=H, W=W)
        self.dref = {k: gpu(t) for k, t in ref.items()}
        self.dpool = {k: gpu(t) for k, t in pool.items()}


@pytest.fixture(scope="module")
def cases():
    """Models and references, built on first use and kept for the module: one reference per pool sample per backbone per model."""
    made, pools, t0 = {}, {}, time.time()

    def pool_of(kind, H, W):
        if (kind, H, W) not in pools:
            pools[(kind, H, W)] = BR.vo_pool(H, W) if kind == "vo" else BR.policy_pool(H, W)
        return pools[(kind, H, W)]

    def get(kind, backbone, *a):
        key = (kind, backbone) + a
        if key not in made:
            if kind == "vo":
                W, H = a
                taps = BR.VO_TAPS + (BR.last_tap(backbone),) if (W, H) == (VO_W, VO_H) else BR.VO_TAPS[:7]
                made[key] = VoCase(backbone, W, H, taps, pool_of("vo", H, W))
            else:
                rgbd, H, W = a
                made[key] = PolicyCase(backbone, rgbd, H, W, pool_of("policy", H, W))
        return made[key]

    yield get
    for c in made.values():
        (c.model if isinstance(c, VoCase) else c.pol)._release()
    print(f"\n[backbone regimes] wall time since the module's first test {time.time() - t0:.1f} s")


# ---------------------------------------------------------------------------------------------------------------- (a) VO sweep
def run_vo(case, B):
    model = case.model
    assert model._options == {}, "the sweep runs on the default options"
    idx = BR.positions(B)
    assert len(set(idx[: min(B, BR.POOL_P)].tolist())) == min(B, BR.POOL_P)
    it = gpu(idx.astype(np.int64))
    obs = {k: v.index_select(0, it).contiguous() for k, v in case.dpool.items()}
    want = lambda k: case.dref[k].index_select(0, it)
    with torch.no_grad():
        out = [model(obs).clone() for _ in range(2)]
        errs = {"pose": BR.position_err(out[0], want("pose"))}
        for name in case.taps:
            _, got = model.tap(name, obs)
            errs[name] = BR.position_err(got, want(name))
        comp = [model.tap("compression", obs)[1].clone() for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[1]) and torch.equal(comp[0], comp[1]), "a repeated call is not bit-identical"
    C = case.cfg.comp_channels
    assert not comp[0][..., C:].any(), "the compression output's pad channels are not zero"
    errs["encoder"] = BR.position_err(comp[0][..., :C].contiguous(), want("encoder"))
    fams = case.families(B)
    taps = max(float(errs[k].max()) for k in case.taps)
    print(f"[vo {case.backbone} {case.cfg.width}x{case.cfg.height}] B={B:3d} pose {errs['pose'].max():.1e} (f32 {case.ref32['pose']:.1e})  "
          f"taps {taps:.1e} (f32 {max(case.ref32[k] for k in case.taps):.1e})  encoder {errs['encoder'].max():.1e} "
          f"(f32 {case.ref32['encoder']:.1e}) | x3 convs {sum(f == 'x3' for f in fams.values())}/{len(x3_eligible(case))} | "
          f"families {','.join(sorted(set(fams.values())))}")
    judge((case.backbone, B), errs)


def x3_eligible(case):
    """The dense 3x3 (stride 1 or 2) and 1x1 stride-2 convs behind the stem, the compression conv among them."""
    return [cd.name for cd in case.convs if plans.eligible(cd) and cd.cgroups == 1]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("backbone", FULL)
def test_vo_sweep_every_position_matches_float64(cases, backbone, B):
    run_vo(cases("vo", backbone, VO_W, VO_H), B)


@pytest.mark.parametrize("B", SPOT_BATCHES)
@pytest.mark.parametrize("backbone", SPOT)
def test_vo_deeper_and_se_backbones_at_64_and_256(cases, backbone, B):
    run_vo(cases("vo", backbone, VO_W, VO_H), B)


# ---------------------------------------------------------------------------------------------------------------- (b) coverage
@pytest.mark.parametrize("backbone", FULL)
def test_the_sweep_reaches_the_regimes(cases, backbone):
    """Default options: at 256 every dense 3x3 and 1x1 stride-2 conv is on x3 and the grouped convs on conv_group; at 9 none is on a
    conv_x3 family; each conv's first x3 batch of the sweep follows a batch where it is not.  If a threshold moves, this fails."""
    case = cases("vo", backbone, VO_W, VO_H)
    assert case.model._options == {}
    eligible = x3_eligible(case)
    grouped = [cd.name for cd in case.convs if cd.cgroups > 1]
    assert len(grouped) == (4 if "neXt" in backbone else 0) and len(eligible) >= 13
    fams = {B: case.families(B) for B in BATCHES}
    assert BATCHES[0] == 9 and BATCHES[-1] == 256
    for n in eligible:
        assert fams[256][n] == "x3", (n, fams[256][n])
        assert not fams[9][n].startswith("x"), (n, fams[9][n])
        on = [fams[B][n] == "x3" for B in BATCHES]
        first = on.index(True)
        assert first > 0 and not on[first - 1] and all(on[first:]), (n, on)
    for n in grouped:
        assert {fams[B][n] for B in BATCHES} == {"group"}, n
    first_x3 = {n.split("backbone.")[-1]: next(B for B in BATCHES if fams[B][n] == "x3") for n in eligible}
    print(f"[{backbone}] first x3 batch of the sweep:", first_x3)
    print(f"[{backbone}] families at 9: {sorted(set(fams[9].values()))}; at 256: {sorted(set(fams[256].values()))}")
    assert any(f.startswith("fp32") for f in fams[256].values())          # the 1x1 stride-1 convs stay on the fp32-MFMA family


# ---------------------------------------------------------------------------------------------------------------- (c), (d) policy
def run_policy(case, B, tag):
    pol = case.pol
    idx = BR.positions(B)
    it = gpu(idx.astype(np.int64))
    sel = lambda k, axis=0: case.dpool[k].index_select(axis, it).contiguous()
    obs = {k: sel(k) for k in case.vis}
    obs[GOAL] = sel("goal")
    if "rgb" in case.vis:
        assert obs["rgb"].dtype == torch.uint8
    hin, pa, mk = sel("hidden", 1), sel("prev").view(B, 1), sel("mask").view(B, 1)
    first = (pol.net.visual_encoder(obs),) + tuple(pol.features_and_logits(obs, hin, pa, mk))
    again = (pol.net.visual_encoder(obs),) + tuple(pol.features_and_logits(obs, hin, pa, mk))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "a repeated call is not bit-identical"
    errs = {}
    for k, got in zip(BR.POLICY_KEYS, first):
        axis = BR.POSITION_AXIS.get(k, 0)
        errs[k] = BR.position_err(got.detach(), case.dref[k].index_select(axis, it), axis)
    print(f"[policy {tag}] B={B:3d} {fmt(errs, case.ref32)}")
    judge((tag, B), errs)


@pytest.mark.parametrize("B", POLICY_BATCHES)
@pytest.mark.parametrize("backbone,rgbd", POLICY_CASES)
def test_policy_every_position_matches_float64(cases, backbone, rgbd, B):
    run_policy(cases("policy", backbone, rgbd, BR.H, BR.W), B, f"{backbone}{' rgb+depth' if rgbd else ''} {BR.W}x{BR.H}")


def test_frozen_encoder_evaluate_actions_encodes_128_frames(cases):
    """se_resneXt50, T = 4, N = 32: 128 frames in one encode, every episode starting at t = 0 and every fifth one again at t = 2."""
    case = cases("policy", "se_resneXt50", False, BR.H, BR.W)
    pol = PB.make_policy(case.sd, "se_resneXt50")          # a policy of its own: the train step takes the weights over
    PB.frozen_agent(pol)
    inp = BR.pool_sequence(case.pool)
    M = inp["T"] * inp["N"]
    ref = BR.sequence_reference(case.sd, inp)
    ref32 = BR.worst_ref32(ref, BR.sequence_reference(case.sd, inp, "float32"))
    assert max(ref32.values()) < BR.REF32_TOL, ref32
    obs = {"depth": gpu(inp["depth"]), GOAL: gpu(inp["goal"])}
    value, logp, entropy, hout = pol.evaluate_actions(obs, gpu(inp["hidden"]), gpu(inp["prev"]).view(M, 1), gpu(inp["masks"]).view(M, 1),
                                                      gpu(inp["actions"]).view(M, 1))
    torch.cuda.synchronize()
    pol._release()
    got = dict(value=value, logp=logp, entropy=entropy.reshape(1), hidden=hout)
    errs = {k: BR.position_err(got[k].detach().cpu(), ref[k], BR.POSITION_AXIS.get(k, 0)) for k in ref}
    print(f"[evaluate_actions se_resneXt50 T=4 N=32] {fmt(errs, ref32)}")
    judge("evaluate_actions", errs)


# ---------------------------------------------------------------------------------------------------------------- (d) even maps
@pytest.mark.parametrize("B", EVEN_BATCHES)
@pytest.mark.parametrize("backbone", EVEN_POLICY)
def test_even_geometry_policy_every_position_matches_float64(cases, backbone, B):
    """Frames 128 x 128: maps 16x16, 8x8, 4x4, 2x2; the grouped convs' pixel counts 256, 64, 16, 4 are whole slots, one whole tile and
    less than a tile; every stride-2 conv reads an even input."""
    case = cases("policy", backbone, False, BR.EVEN_H, BR.EVEN_W)
    assert tuple(case.pol.net.visual_encoder.output_shape) == (512, 2, 2)
    run_policy(case, B, f"{backbone} {BR.EVEN_W}x{BR.EVEN_H}")


@pytest.mark.parametrize("B", EVEN_BATCHES)
@pytest.mark.parametrize("backbone", EVEN_POLICY)
def test_even_geometry_vo_taps_match_float64(cases, backbone, B):
    case = cases("vo", backbone, EVEN_VO, EVEN_VO)
    assert [case.cfg.layer_hw(li) for li in (1, 2, 3, 4)] == [(16, 16), (8, 8), (4, 4), (2, 2)]
    run_vo(case, B)
