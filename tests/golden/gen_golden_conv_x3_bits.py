#!/usr/bin/env python
"""Generate tests/golden/conv_x3_bits.txt on the MI355X: checksums of the BITS of what the conv_x3 kernels (csrc/conv_x3.hip:
conv_x3_kernel in all its flavours, conv_x3p_kernel) compute, case by case.

    python tests/golden/gen_golden_conv_x3_bits.py

tests/test_gpu_conv_x3_bits.py recomputes the table (table() below) and compares it line by line, so a change of those kernels that
moves one bit of one output, block output, pooled activation, hidden feature or training gradient fails there.  The file was written by
a build of commit 5c2043e ("Inference forwards: steps, one block walk, shared checks, bf16 requests"), the parent of the change that
moved conv_x3.hip's global-memory accesses onto buffer descriptors: addressing and control flow only, the float operations on every
value and their order unchanged.  Regenerate it only with a change that MEANS to change the arithmetic of these kernels, from the
commit before any other change of them.

A line is
    <case> <tensor> <elements> <plain sum> <position-weighted sum>
both sums over the tensor's 32-bit patterns in wrapping 32-bit integer arithmetic, taken on the device (the scheme of
profiles/forward_walk.md, "Identity"); the weight of element i is i + 1.  Tensors per forward case: the model output, the hidden
features (pnvo_forward_features), and — where the case names tap batches — every block output `layer<s>.<i>` and the pooled stem output
`maxpool` (the taps pnvo_tap_shape accepts that a conv_x3 stager writes or reads; a tap runs the plain schedule: stager modes 0 and 1
where the untapped forward runs 2 and 3).

Cases (the smallest at which each code path can go wrong):
    bench224 / bench8 / bench33   the benchmark model (bench.build_model, 341 x 192) at 224 pairs — the smallest batch at which the
                                  eight-wave form, the 16-row one-tile form and the strips all engage — and at 8 and 33 pairs (fine plan,
                                  K split over the waves, in-kernel GroupNorm finalisation)
    odd3 / odd17                  a resnet18 VO model at 200 x 113 with option conv=x3: 50 x 29, 25 x 15, 13 x 8 and 7 x 4 maps — ragged
                                  tiles on the right and at the bottom, patch pixels off all four edges, odd maps under the stride-2 convs
    odd17:<option>=<value>        the same at 17 pairs under pieces=3, ds_fuse=off, tail=separate, pool=separate, x3_w8=off, x3_m16=off,
                                  x3_fine=off
    train                         one training step (forward in train mode, backward) of tests/golden/train_default_45x37_b4_f64.npz with
                                  option conv=x3: the flat gradient and the loss (training forward and backward-data convs)
    persist16 / 64 / 96           the benchmark model with x3_rows=off at 16 and 64 pairs (the batches of
                                  tests/test_gpu_knobs.py::test_persistent_resident_weight_convs_are_bit_identical) and at 96: conv_x3p_kernel
                                  takes layer1's second convs from two tiles per resident workgroup on — 1536 tiles of 18 per pair on 256
                                  CUs, 86 pairs — so 96 is the case that reaches it; the smaller two run the same layers on conv_x3_kernel

Coverage (check_coverage, asserted on what ran, not on what was meant): the cases reach a launch of every stager mode 0-3, a launch
with a riding downsample conv (DSF), an eight-wave launch (W8), a 16-row launch (M16), a K-split launch (KSW) and a persistent launch
— read from the kernel family pnvo_layer_kernel reports for every conv of every case and from the instance the planner names for that
launch (pnvo_conv_x3_describe); a layer that fell back to another kernel family counts for nothing.
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PATH = os.path.join(ROOT, "tests", "golden", "conv_x3_bits.txt")
ODD_W, ODD_H = 200, 113
ODD_OPTIONS = (("pieces", "3", "2"), ("ds_fuse", "off", "on"), ("tail", "separate", "fused"), ("pool", "separate", "fused"),
               ("x3_w8", "off", "on"), ("x3_m16", "off", "on"), ("x3_fine", "off", "on"))
BLOCK_TAPS = ["maxpool"] + [f"layer{s}.{i}" for s in (1, 2, 3, 4) for i in (0, 1)]
NUM_CUS = 256
# field order of pnvo_conv_x3_describe's problem array (include/pnvo.h)
FIELDS = ("B", "H", "W", "CIN", "Ho", "Wo", "COUTP", "ks", "stride", "np", "mode", "tail_scaled", "absmax", "ds",
          "force", "strip", "fine", "w8", "m16", "ksw", "persist_wgs", "rows", "num_cus")
# plan options of a handle with default settings (csrc/pnvo_api.hip: conv_choice) and the model options that set them
PLAN_DEFAULTS = dict(force=0, strip=1, fine=1, w8=1, m16=1, ksw=1, persist=1, rows=1)
PLAN_OPTION = {"conv": ("force", {"x3": 1, "auto": 0}), "x3_w8": ("w8", {"on": 1, "off": 0}), "x3_m16": ("m16", {"on": 1, "off": 0}),
               "x3_fine": ("fine", {"on": 1, "off": 0}), "x3_rows": ("rows", {"on": 1, "off": 0})}


def checksum(t):
    """(elements, plain sum, position-weighted sum) of the tensor's bit patterns, wrapping 32-bit, computed where the tensor lives."""
    bits = t.detach().contiguous().reshape(-1).view(torch.int32).to(torch.int64)
    w = torch.arange(1, bits.numel() + 1, device=bits.device, dtype=torch.int64)
    return bits.numel(), int(bits.sum().item()) & 0xffffffff, int((bits * w).sum().item()) & 0xffffffff


def rup(x, m):
    return (x + m - 1) // m * m


def features(model, obs):
    from pointnav_vo_amd import _lib
    from pointnav_vo_amd.vo_cnn import _obs_ptrs

    dev = next(model.parameters()).device
    ptrs, B, keep = _obs_ptrs(model, obs, dev)
    out = torch.zeros((B, model.cfg.hidden), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.lib.pnvo_forward_features(model._handle, ptrs[0], ptrs[1], ptrs[2], ptrs[3], None, int(B),
                                                  C.c_void_p(out.data_ptr()), C.c_void_p(stream)), model._handle)
    return out


def tap(model, name, obs, B):
    """model.tap with a zero-filled buffer (padding channels, if any, then have defined bits)."""
    from pointnav_vo_amd import _lib

    dev = next(model.parameters()).device
    shape = (C.c_int64 * 4)()
    _lib.check(_lib.lib.pnvo_tap_shape(model._handle, name.encode(), int(B), shape), model._handle)
    buf = torch.zeros(tuple(int(s) for s in shape), device=dev, dtype=torch.float32)
    _lib.check(_lib.lib.pnvo_set_tap(model._handle, name.encode(), C.c_void_p(buf.data_ptr()), buf.numel()), model._handle)
    try:
        model(obs)
    finally:
        _lib.lib.pnvo_set_tap(model._handle, None, None, 0)
    return buf


def launches(model, B, opts):
    """Instance keys ("tile ks3 s1 np2 mode1 ...") of the conv_x3 launches of one untapped forward of `model` at B pairs under option
    settings `opts` ({option: value} on top of the defaults): for every conv that pnvo_layer_kernel puts on the x2 / x3 family, the
    planner's answer for the problem the schedule asks (csrc/pnvo_api.hip: conv_choice — mode 3 behind the pooled stem keys, 2 where the
    conv takes the previous block's tail, 1 behind a GroupNorm, 0 on final activations)."""
    from pointnav_vo_amd import _lib, model_spec as ms

    plan = dict(PLAN_DEFAULTS)
    for k, v in opts.items():
        if k in PLAN_OPTION:
            plan[PLAN_OPTION[k][0]] = PLAN_OPTION[k][1][v]
    tail, pool = opts.get("tail", "fused") == "fused", opts.get("pool", "fused") == "fused"
    convs = ms.conv_plan(model.cfg)[1:]
    fam = {cd.name: model.layer_kernel(cd.name, B)[0] for cd in convs}
    keys, buf = [], C.create_string_buffer(256)
    for k, cd in enumerate(convs):
        if fam[cd.name] not in ("x2", "x3"):              # ("x2-rides": no launch of its own)
            continue
        if ".downsample." in cd.name:                      # a 1x1 stride-2 launch of its own reads the materialised block input
            mode = 0
        elif k == 0:
            mode = 3 if pool else 0
        elif cd.name.endswith(".convs.0") or "compression" in cd.name:
            mode = 2 if tail else 0
        else:
            mode = 1
        ds = int(fam.get(cd.name.replace(".convs.0", ".downsample.0")) == "x2-rides") if cd.name.endswith(".0.convs.0") else 0
        f = dict(B=B, H=cd.hin, W=cd.win, CIN=rup(cd.cin, 8), Ho=cd.hout, Wo=cd.wout, COUTP=rup(cd.cout, 32), ks=cd.k, stride=cd.stride,
                 np=2 if fam[cd.name] == "x2" else 3, mode=mode, tail_scaled=0, absmax=0, ds=ds, force=plan["force"], strip=plan["strip"],
                 fine=plan["fine"], w8=plan["w8"], m16=plan["m16"], ksw=plan["ksw"], persist_wgs=3 * NUM_CUS if plan["persist"] else 0,
                 rows=plan["rows"], num_cus=NUM_CUS)
        q = np.ascontiguousarray([f[n] for n in FIELDS], dtype=np.int32)
        _lib.check(_lib.lib.pnvo_conv_x3_describe(q.ctypes.data_as(C.POINTER(C.c_int)), len(q), buf, len(buf)))
        keys.append(buf.value.decode().split(" | ")[0])
    return keys


def forward_case(out, seen, case, model, obs, B, opts, taps):
    with torch.no_grad():
        for name, t in [("output", model(obs)), ("features", features(model, obs))] + [(n, tap(model, n, obs, B)) for n in taps]:
            out.append("%s %s %d %d %d" % ((case, name) + checksum(t)))
    seen.extend(launches(model, B, opts))


def odd_model(dev):
    import bench
    from pointnav_vo_amd import model_spec as ms, synth
    from pointnav_vo_amd.registry import baseline_registry

    m = baseline_registry.get_vo_model("vo_cnn_rgb_d_dd_top_down")(
        observation_space=bench.SPACE, observation_size=(ODD_W, ODD_H), hidden_size=512, backbone="resnet18", normalize_visual_inputs=True,
        output_dim=3, dropout_p=0.2, discretized_depth_channels=10)
    sd = synth.make_state_dict(ms.state_dict_spec(m.cfg), seed=ODD_W)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    obs = synth.make_obs_pairs(17, ODD_H, ODD_W, observation_space=bench.SPACE, dd_bins=10, seed=ODD_H)
    return m.to(dev).eval(), {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in obs.items()}


def train_case(out, dev):
    from conftest import golden_case, load_golden
    from pointnav_vo_amd.registry import baseline_registry
    from pointnav_vo_amd.train import VOTrainStep

    rec = load_golden("train_default_45x37_b4_f64.npz")
    cfg, sd, obs, _ = golden_case(rec)
    model = baseline_registry.get_vo_model(str(rec["model"]))(
        observation_space=str(rec["obs_space"]).split(","), observation_size=(cfg.width, cfg.height), hidden_size=512, backbone="resnet18",
        normalize_visual_inputs=True, output_dim=3, dropout_p=0.0, discretized_depth_channels=int(rec["dd_bins"]))
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    model = model.to(dev)
    model._ensure_handle(dev)
    model.set_option("conv", "x3")
    ts = VOTrainStep(model, lr=float(rec["lr"]), eps=float(rec["eps"]))
    tobs = {k: torch.from_numpy(v).to(dev) for k, v in obs.items()}
    _, loss = ts.forward_backward(tobs, target=torch.from_numpy(rec["target"]).to(dev))
    torch.cuda.synchronize(dev)
    fams = [model.layer_kernel(cd_name, 4)[0] for cd_name in ("visual_encoder.backbone.layer1.0.convs.0", "visual_encoder.backbone.layer3.1.convs.3")]
    assert all(f in ("x2", "x3") for f in fams), fams
    out.append("train grad %d %d %d" % checksum(ts.grad))
    out.append("train loss %d %d %d" % checksum(loss.detach().reshape(1).to(torch.float32)))
    del ts, model


def table(dev, seen=None):
    """The file's lines; `seen` (a list) receives the instance keys of the conv_x3 launches of the forward cases."""
    import bench

    out, seen = [], [] if seen is None else seen
    model, _ = bench.build_model(dev)
    obs = bench.make_inputs(224, dev, 5)
    first = lambda B: {k: v[:B] for k, v in obs.items()}
    with torch.no_grad():
        model(first(1))                                        # creates the handle and loads the weights
    forward_case(out, seen, "bench224", model, obs, 224, {}, BLOCK_TAPS)
    forward_case(out, seen, "bench8", model, first(8), 8, {}, BLOCK_TAPS)
    forward_case(out, seen, "bench33", model, first(33), 33, {}, ())
    model.set_option("x3_rows", "off")
    for B in (16, 64, 96):
        forward_case(out, seen, f"persist{B}", model, first(B), B, {"x3_rows": "off"}, ())
    model._release()
    del model, obs

    m, oobs = odd_model(dev)
    with torch.no_grad():
        m({k: v[:1] for k, v in oobs.items()})
    m.set_option("conv", "x3")
    forward_case(out, seen, "odd3", m, {k: v[:3] for k, v in oobs.items()}, 3, {"conv": "x3"}, BLOCK_TAPS)
    forward_case(out, seen, "odd17", m, oobs, 17, {"conv": "x3"}, BLOCK_TAPS)
    for key, value, default in ODD_OPTIONS:
        m.set_option(key, value)
        forward_case(out, seen, f"odd17:{key}={value}", m, oobs, 17, {"conv": "x3", key: value}, ())
        m.set_option(key, default)
    m._release()
    del m, oobs

    train_case(out, dev)
    torch.cuda.synchronize(dev)
    return out


def check_coverage(seen):
    """Every stager mode, DSF, W8, M16, KSW and the persistent kernel are reached by a launch of the cases (module docstring)."""
    tile = [k for k in seen if k.startswith("tile ")]
    for mode in range(4):
        assert any(f" mode{mode} " in k for k in tile), (f"no conv_x3_kernel launch with stager mode {mode}", sorted(set(seen)))
    for flag in ("dsf1", "w81", "ksw1", "m161"):
        assert any(f" {flag}" in k + " " for k in tile), (f"no conv_x3_kernel launch with {flag}", sorted(set(seen)))
    assert any(" np3 " in k for k in tile) and any(" ks1 " in k for k in tile), sorted(set(seen))
    assert any(k.startswith("persistent ") for k in seen), ("no conv_x3p_kernel launch", sorted(set(seen)))


if __name__ == "__main__":
    seen = []
    rows = table(torch.device("cuda:0"), seen)
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, "w") as f:
        f.write("\n".join(rows) + "\n")
    print(f"{len(rows)} lines")
    for k in sorted(set(seen)):
        print("launch:", k)
    check_coverage(seen)
    print("coverage ok")
