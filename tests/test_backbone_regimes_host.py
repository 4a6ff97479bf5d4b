"""CPU: what tests/test_gpu_backbone_regimes.py rests on, checked without a device.

  - Planner coverage: every conv_x3-eligible dense conv (3x3 stride 1 / 2, 1x1 stride 2, the compression conv) of the six Bottleneck /
    ResNeXt / SE-ResNeXt backbones, at the sweep's geometry (maps 13x17 .. 2x3) and the even one (16x16 .. 2x2), through
    pnvo_conv_x3_describe with the handle's default options, 256 CUs and three operand pieces: it plans at 256 and plans `none` at 9,
    stays planned once it is, and the GPU module's batch list (imported, not copied) holds both the first planned batch and the one
    below it.
  - The pool: 31 distinct samples, the zero-bordered and flat ones where they are said to be; positions() gives distinct samples
    to positions closer than the pool and a different offset to every batch the GPU module uses.
  - The float32 restatement stays below a quarter of the GPU module's bound against the float64 one, per position, on the committed
    pool, for every reference that module builds: a bad pool fails here, before anyone books a device.
"""
import numpy as np
import pytest

import backbone_reference as BR
import test_conv_x3_plan as plans
import test_gpu_backbone_regimes as GR
from pointnav_vo_amd import model_spec as ms, synth

GEOMETRIES = {"odd": (GR.VO_W, GR.VO_H), "even": (GR.EVEN_VO, GR.EVEN_VO)}


def first_planned(cd, mode):
    """(first batch of 1..256 the planner takes the conv at, whether it keeps it from there on)."""
    H, W, CIN, Ho, Wo, COUTP, ks, stride, _ = plans.fwd_shape(cd)
    shape = dict(H=H, W=W, CIN=CIN, Ho=Ho, Wo=Wo, COUTP=COUTP, ks=ks, stride=stride)
    on = [plans.describe(plans.problem_of(B=B, np=3, mode=mode, **shape)) != "none" for B in range(1, 257)]
    first = on.index(True) + 1 if any(on) else None
    return first, first is not None and all(on[first - 1:])


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
@pytest.mark.parametrize("backbone", GR.FULL + GR.SPOT)
def test_planner_takes_every_dense_conv_inside_the_sweep(backbone, geometry):
    W, H = GEOMETRIES[geometry]
    cfg, _ = BR.vo_spec(backbone, W, H)
    convs = [cd for cd in ms.conv_plan(cfg)[1:] if plans.eligible(cd) and cd.cgroups == 1]
    assert len(convs) >= 13 and convs[-1].name == "visual_encoder.compression.0"
    assert [cfg.layer_hw(li) for li in (1, 2, 3, 4)] == ([(13, 17), (7, 9), (4, 5), (2, 3)] if geometry == "odd" else
                                                          [(16, 16), (8, 8), (4, 4), (2, 2)])
    seen = {}
    for cd in convs:
        first, kept = first_planned(cd, 1)              # (mode 1: the producer's GroupNorm applied on fetch, what these convs launch with)
        assert first_planned(cd, 0) == (first, kept), cd.name
        assert first is not None and 9 < first <= 256 and kept, (cd.name, first, kept)
        if geometry == "odd":                            # the sweep holds both sides of the conv's own threshold
            assert first in GR.BATCHES and first - 1 in GR.BATCHES, (cd.name, first)
        else:
            assert min(GR.EVEN_BATCHES) < first
        seen.setdefault(first, []).append(cd.name.split("backbone.")[-1])
    print(backbone, geometry, {k: len(v) for k, v in sorted(seen.items())})
    if geometry == "even":                               # at 64 some of the model's convs are on conv_x3 and some are not
        assert any(f <= max(GR.EVEN_BATCHES) for f in seen) and any(f > max(GR.EVEN_BATCHES) for f in seen)


def test_positions_and_batch_lists():
    P = BR.POOL_P
    used = sorted(set(GR.BATCHES) | set(GR.SPOT_BATCHES) | set(GR.EVEN_BATCHES) | set(GR.POLICY_BATCHES) | {128})
    for need in (9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256):
        assert need in GR.BATCHES
    offsets = {}
    for B in used:
        idx = BR.positions(B)
        assert idx.shape == (B,) and idx.min() >= 0 and idx.max() < P
        for i in range(B):                               # two positions closer than the pool hold different samples
            assert len(set(idx[i:i + P].tolist())) == min(P, B - i)
        offsets[B] = int(idx[0])
    assert len(set(offsets.values())) == len(offsets), offsets


@pytest.mark.parametrize("kind,H,W", [("policy", BR.H, BR.W), ("policy", BR.EVEN_H, BR.EVEN_W), ("vo", GR.VO_H, GR.VO_W),
                                      ("vo", GR.EVEN_VO, GR.EVEN_VO)])
def test_pool_holds_distinct_samples_and_the_edge_frames(kind, H, W):
    pool = BR.policy_pool(H, W) if kind == "policy" else BR.vo_pool(H, W)
    P = BR.POOL_P
    for k in ("rgb", "depth"):
        v = pool[k].reshape(P, -1)
        assert len({v[i].tobytes() for i in range(P)}) == P, k
        flat = {n: pool[k][i].astype(np.float64) for n, i in BR.FLAT.items()}
        assert np.ptp(flat["constant"]) == 0.0 and 0 < np.ptp(flat["ripple"]) <= 0.02 * (255 if k == "rgb" else 1)
        assert np.ptp(flat["two_level"][:H // 2]) == 0.0 and np.ptp(flat["two_level"][H // 2:]) == 0.0 and np.ptp(flat["two_level"]) > 0
        for n, i in enumerate(BR.ZERO_BORDER):
            z = 2 * (n + 1)
            f = pool[k][i]
            assert not f[:z].any() and not f[-z:].any() and not f[:, :z].any() and not f[:, -2 * z:].any() and f[z:-z, z:-2 * z].any()
    assert pool["depth"].min() >= 0.0 and pool["depth"].max() <= 1.0
    if kind == "policy":
        assert pool["rgb"].dtype == np.uint8 and sorted(np.flatnonzero(pool["mask"] == 0).tolist()) == sorted(BR.ZERO_MASK)
        assert pool["hidden"].any() and pool["hidden"].shape == (2 * BR.LAYERS, P, BR.HIDDEN)


def quarter(what, ref64, ref32):
    worst = BR.worst_ref32(ref64, ref32)
    print(f"[{what}] float32 restatement vs float64, worst position: " + "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for v in ref64.values():
        assert np.isfinite(v).all()
    assert max(worst.values()) < BR.REF32_TOL, (what, worst)


VO_REFS = [(b, GR.VO_W, GR.VO_H) for b in GR.FULL + GR.SPOT] + [(b, GR.EVEN_VO, GR.EVEN_VO) for b in GR.EVEN_POLICY]


@pytest.mark.parametrize("backbone,W,H", VO_REFS)
def test_float32_vo_restatement_stays_a_quarter_inside_the_bound(backbone, W, H):
    cfg, spec = BR.vo_spec(backbone, W, H)
    sd = synth.make_state_dict(spec, seed=BR.VO["seed"])
    pool = BR.vo_pool(H, W)
    taps = BR.VO_TAPS + (BR.last_tap(backbone),) if (W, H) == (GR.VO_W, GR.VO_H) else BR.VO_TAPS[:7]
    quarter(f"vo {backbone} {W}x{H}", BR.vo_pool_reference(sd, cfg, pool, taps), BR.vo_pool_reference(sd, cfg, pool, taps, "float32"))


POLICY_REFS = [(b, r, BR.H, BR.W) for b, r in GR.POLICY_CASES] + [(b, False, BR.EVEN_H, BR.EVEN_W) for b in GR.EVEN_POLICY]


@pytest.mark.parametrize("backbone,rgbd,H,W", POLICY_REFS)
def test_float32_policy_restatement_stays_a_quarter_inside_the_bound(backbone, rgbd, H, W):
    vis, normalize = (("rgb", "depth"), True) if rgbd else (("depth",), False)
    sd = BR.pool_state_dict(backbone, vis, normalize, H, W)
    pool = BR.policy_pool(H, W)
    quarter(f"policy {backbone} {vis} {W}x{H}", BR.policy_pool_reference(sd, pool, vis), BR.policy_pool_reference(sd, pool, vis, "float32"))
    if (backbone, rgbd, H) == ("se_resneXt50", False, BR.H):
        inp = BR.pool_sequence(pool)
        assert inp["T"] * inp["N"] == 128 and not inp["masks"][:32].any() and 0 < (inp["masks"][64:96] == 0).sum() < 32
        quarter("evaluate_actions T=4 N=32", BR.sequence_reference(sd, inp), BR.sequence_reference(sd, inp, "float32"))
