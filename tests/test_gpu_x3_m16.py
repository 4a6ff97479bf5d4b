"""GPU (-m gpu): option x3_m16 — the K loop of conv_x3_kernel on v_mfma_f32_16x16x32_f16, M padded to 16 rows instead of 32, on the
launches conv_x3_plan picks from their geometry: the 128-channel strips (12 x 22 maps) and the one-tile-per-sample 256-channel convs
(6 x 11 maps; eight-wave and four-wave form).  341x192 inputs give those maps.  Batches are the smallest at which each form engages,
READ FROM THE PLAN (layer_kernel's executed FLOPs with the option on and off): B3 for the strips, B4 for the one-tile launches — the
regular plan takes them from 200 tiles on, but below 224 workgroups the fine plan still goes first.  All batches are slices of ONE
input, and the fp64 oracle runs once over the pairs the tests look at."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L3 = "visual_encoder.backbone.layer3.1.convs.3"
L4 = "visual_encoder.backbone.layer4.1.convs.3"
_state = {}


def engages_at(model, layer):
    """Smallest batch (up to 256 pairs) at which option x3_m16 changes the form of `layer`."""
    flops = {}
    for v in ("off", "on"):
        model.set_option("x3_m16", v)
        flops[v] = [model.layer_kernel(layer, B)[1] for B in range(1, 257)]
    hits = [B for B in range(1, 257) if flops["on"][B - 1] != flops["off"][B - 1]]
    assert hits, f"x3_m16 never changes {layer} up to 256 pairs"
    assert hits == list(range(hits[0], 257)), (layer, hits)          # from there on: the geometry decides, nothing else
    return hits[0]


def boundary_batches(B4):
    return [199, 201, B4 - 1, B4 + 1]


def shared():
    """(model, pairs on the device, fp64 oracle poses of the pairs the tests look at, B3, B4) — built once per process."""
    if not _state:
        import bench
        from oracle import oracle
        dev = torch.device("cuda", 0)
        model, sd = bench.build_model(dev)
        B3, B4 = engages_at(model, L3), engages_at(model, L4)
        pairs = sorted({p for B in boundary_batches(B4) + [B4] for p in (0, B // 2, B - 1)})
        obs = bench.make_inputs(max(pairs) + 1, dev, 23)
        ref = oracle.forward(sd, {k: v[pairs].cpu().numpy() for k, v in obs.items()}, ngroups=model.cfg.ngroups, dtype=np.float64)
        _state.update(model=model, obs=obs, ref={p: ref[i] for i, p in enumerate(pairs)}, B3=B3, B4=B4)
        print(f"x3_m16 engages at {B3} pairs (strips) and {B4} pairs (one tile per sample)")
    return _state["model"], _state["obs"], _state["ref"]


def first(obs, B):
    return {k: v[:B] for k, v in obs.items()}


def oracle_err(out, ref, pairs):
    got = out[pairs].double().cpu().numpy()
    want = np.stack([ref[p] for p in pairs])
    return np.linalg.norm(got - want, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-2)


@pytest.fixture(autouse=True)
def default_options():
    yield
    if _state:
        for k, v in (("x3_m16", "on"), ("x3_w8", "on"), ("x3_rows", "on"), ("tail", "fused")):
            _state["model"].set_option(k, v)


def test_m16_changes_the_form_not_the_result():
    """on / off / on at B4 pairs (both forms engaged): on == on by bits; on vs off differ by float32 rounding only (another summation grouping inside the
    MFMA, another order of the statistics): relative pose difference non-zero and below 2e-5; the executed MFMA FLOPs that layer_kernel
    reports show that the option changed the form of both stages (272 instead of 288 rows, 80 instead of 96)."""
    model, obs, _ = shared()
    B4 = _state["B4"]
    assert _state["B3"] <= B4
    x = first(obs, B4)
    outs, flops = {}, {}
    with torch.no_grad():
        for v in ("on", "off", "on2"):
            model.set_option("x3_m16", v[:2] if v != "off" else "off")
            outs[v] = model(x).clone()
            flops[v] = [model.layer_kernel(n, B4) for n in (L3, L4)]
        torch.cuda.synchronize()
    assert torch.isfinite(outs["on"]).all() and torch.equal(outs["on"], outs["on2"])
    rel = float(((outs["on"] - outs["off"]).norm(dim=1) / outs["off"].norm(dim=1).clamp_min(1e-2)).max())
    print("relative pose difference on vs off:", rel, "| layer_kernel:", flops)
    assert 0 < rel < 2e-5, rel
    for k in range(2):
        assert flops["on"][k][0] == flops["off"][k][0] == "x2", flops
    assert flops["on"][0][1] * 288 == flops["off"][0][1] * 272, flops      # layer3: 17 sub-tiles of 16 rows against 9 M-tiles of 32
    assert flops["on"][1][1] * 96 == flops["off"][1][1] * 80, flops        # layer4: 5 against 3
    assert flops["on"] == flops["on2"]


def test_m16_block_output_taps_agree_at_every_position_and_channel():
    """Block outputs of layer3 and layer4, on vs off, over every position and channel: within float32 noise of the tap's range (the
    bound of tests/test_gpu_block_taps.py: 2e-5 of the largest magnitude).  A wrong row / column mapping in the 16 x 16 epilogue moves
    whole rows or channels — far outside that — where the pose alone could hide it."""
    model, obs, _ = shared()
    B4 = _state["B4"]
    assert _state["B3"] <= B4
    x = first(obs, B4)
    for name in ("layer3.0", "layer3.1", "layer4.0", "layer4.1"):
        taps = {}
        with torch.no_grad():
            for v in ("on", "off"):
                model.set_option("x3_m16", v)
                taps[v] = model.tap(name, x)[1].clone()
        scale = float(taps["off"].abs().max()) + 1e-6
        err = float((taps["on"] - taps["off"]).abs().max())
        print(f"{name}: shape {tuple(taps['on'].shape)} max|on - off| / max|off| = {err / scale:.3e}")
        assert torch.isfinite(taps["on"]).all()
        assert err / scale < 2e-5, (name, err, scale)


def test_m16_matches_the_fp64_oracle():
    """First, middle and last pair of the B4-pair batch against the fp64 oracle with the option on: float32-grade (2e-5)."""
    model, obs, ref = shared()
    with torch.no_grad():
        out = model(first(obs, _state["B4"]))
    err = oracle_err(out, ref, [0, _state["B4"] // 2, _state["B4"] - 1])
    print("rel err vs fp64 oracle:", err)
    assert err.max() < 2e-5, err


def test_m16_eight_and_four_wave_forms_are_bit_identical():
    """With the option on, x3_w8 on == off by bits at B4 pairs: 5 x 2 sub-tiles per wave on eight waves and 5 x 4 on four are the same
    MFMA chain per output and the same order of the statistics."""
    model, obs, _ = shared()
    B4 = _state["B4"]
    assert _state["B3"] <= B4
    x = first(obs, B4)
    outs = {}
    with torch.no_grad():
        for v in ("on", "off"):
            model.set_option("x3_w8", v)
            outs[v] = model(x).clone()
        torch.cuda.synchronize()
    assert torch.isfinite(outs["on"]).all() and torch.equal(outs["on"], outs["off"])


def test_m16_block_tail_in_the_stager_is_bit_identical_to_the_separate_pass():
    """With the option on, default == tail=separate by bits at B3 pairs (the strips' smallest regular-plan batch), one conv kernel
    family on both sides (x3_rows=off, as tests/test_gpu_fullsize.py does): stager modes 0 and 2 of a layer share the MFMA chain."""
    model, obs, _ = shared()
    B3 = _state["B3"]
    x = first(obs, B3)
    model.set_option("x3_rows", "off")
    assert model.layer_kernel(L3, B3)[1] == 3.0 * 2.0 * B3 * 272 * 128 * 128 * 9, "the strips are not on the 16-row form"
    outs = {}
    with torch.no_grad():
        for v in ("fused", "separate"):
            model.set_option("tail", v)
            outs[v] = model(x).clone()
        torch.cuda.synchronize()
    assert torch.isfinite(outs["fused"]).all() and torch.equal(outs["fused"], outs["separate"])


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_m16_next_to_the_tile_count_boundary(which):
    """One pair short of / past the 200 tiles from which the regular plan gives the one-tile-per-sample launches the 16-row form, and
    one short of / past B4, where that plan actually takes over from the fine plan: the executed FLOPs say which form runs, the forward
    is finite and matches the oracle on its first, middle and last pair."""
    model, obs, ref = shared()
    B = boundary_batches(_state["B4"])[which]
    fl = model.layer_kernel(L4, B)[1] / B
    assert fl == 3.0 * 2.0 * (80 if B >= _state["B4"] else 96) * 256 * 256 * 9, (B, fl)
    with torch.no_grad():
        out = model(first(obs, B))
    assert torch.isfinite(out).all()
    err = oracle_err(out, ref, [0, B // 2, B - 1])
    print(f"B {B}: rel err vs fp64 oracle:", err)
    assert err.max() < 2e-5, err
