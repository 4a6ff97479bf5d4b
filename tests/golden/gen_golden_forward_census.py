#!/usr/bin/env python
"""Generate tests/golden/forward_census.txt on the MI355X: the ordered timing table (pnvo_timing_read: entry names in first-launch
order with their launch counts, and the sum of the entries' flops) of ONE inference forward per (model, option set, batch size).

    python tests/golden/gen_golden_forward_census.py

The table pins the forward's WALK — which launches a forward makes, in which order, under which names: tests/test_gpu_forward_census.py
recomputes it (table() below) and compares line for line, so a change of the host code that adds, drops, renames or reorders one launch
of one forward fails there.  It was generated at the commit before the float32 and the bfloat16 forward were split into steps with one
block walk; regenerate it only with a change that means to move a launch, from the commit before a refactor of the walk otherwise.

Models, all at 68 x 52 (rgb + depth, as tests/backbone_reference.py's VO case): a BasicBlock model (resnet18), the resnet50 and the
se_resneXt50 VO model; one dual bfloat16 section on two BasicBlock models.  `pool_init` (the pooled-key form of the max-pool) appears
on the BasicBlock model at 68 x 52 from 64 pairs on at the generating commit: no larger frame was needed.  The persistent
small-batch launch (`smallnet`) cannot appear on it at 68 x 52 at any batch size (SMALL_W below): a fourth, short section runs the
same model at 136 x 104.

Format.  `M <model>` and `O <option>=<value>` open a section; a case line is
    B <batch> <flops sum> S<k>
where S<k> is the k-th distinct launch sequence of the model, written once, on the line before its first use, as
    S<k>= <entry name>*<launches> ...
in the table's order ("conv:" names without the "visual_encoder." / "backbone." prefixes).

Coverage (asserted below on what was written): `pool_init`, `gn_relu_maxpool`, `gn_relu_apply` and `residual` each appear in a line
of the BasicBlock model at 68 x 52 and are absent from another; `smallnet` likewise at 136 x 104; `bf16:residual` likewise in the dual
section.  An `se_gate:` entry cannot be absent from a line of the SE model — the gate runs in every block of every forward of it, and
the persistent small-batch kernel does not take Bottleneck models — so it is required in every line of the se_resneXt50 model and in
no line of the other models.  Every line of the two Bottleneck models holds `residual`: such a block never hands its tail on.
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

PATH = os.path.join(ROOT, "tests", "golden", "forward_census.txt")
VO_W, VO_H = 68, 52
# (model, batch sizes, option sets: (option, value, the default it returns to))
BASIC_BATCHES = (1, 2, 3, 4, 5, 8, 16, 48, 49, 64, 128, 256)
DEEP_BATCHES = (1, 2, 4, 9, 32, 48, 49, 64, 128, 256)
BASIC_OPTIONS = ((None, None, None), ("tail", "separate", "fused"), ("pool", "separate", "fused"), ("ds_fuse", "off", "on"),
                 ("conv", "x3", "auto"), ("conv", "generic", "auto"), ("small_net", "off", "on"), ("head_fuse", "off", "on"))
DEEP_OPTIONS = ((None, None, None), ("conv", "x3", "auto"), ("conv", "generic", "auto"), ("head_fuse", "off", "on"))
# The persistent small-batch kernel does not take the BasicBlock model at 68 x 52 (its compression conv has 352 padded channels there,
# the kernel serves 32, 64 or 128): one short section at 136 x 104 (128 channels), where it takes batches up to 8.
SMALL_W, SMALL_H = 136, 104
SMALL_BATCHES = (1, 3, 8, 9)
SMALL_OPTIONS = ((None, None, None), ("small_net", "off", "on"))
MODELS = (("resnet18", VO_W, VO_H, BASIC_BATCHES, BASIC_OPTIONS), ("resnet50", VO_W, VO_H, DEEP_BATCHES, DEEP_OPTIONS),
          ("se_resneXt50", VO_W, VO_H, DEEP_BATCHES, DEEP_OPTIONS), ("resnet18", SMALL_W, SMALL_H, SMALL_BATCHES, SMALL_OPTIONS))
DUAL_BATCHES = (2, 40, 256)
DUAL_OPTIONS = ((None, None, None), ("bf16_fuse", "off", "on"), ("ds_fuse", "off", "on"), ("gn_fuse", "off", "on"))


def build(backbone, dev, seed=None, W=VO_W, H=VO_H):
    import backbone_reference as BR
    from pointnav_vo_amd import synth
    from pointnav_vo_amd.vo_cnn import VisualOdometryCNNBase

    v = BR.VO
    _, spec = BR.vo_spec(backbone, W, H)
    model = VisualOdometryCNNBase(observation_space=list(v["space"]), observation_size=(W, H), hidden_size=v["hidden"], backbone=backbone,
                                  normalize_visual_inputs=True, output_dim=3, discretized_depth_channels=v["dd_bins"])
    sd = synth.make_state_dict(spec, seed=v["seed"] if seed is None else seed)
    model.load_state_dict({k: torch.from_numpy(np.array(t)) for k, t in sd.items()})
    return model.to(dev).eval()


def inputs(B, dev, W=VO_W, H=VO_H):
    """Contract inputs of the right shapes: the walk depends on shapes and options only."""
    return {"rgb": torch.zeros((B, H, W, 6), device=dev), "depth": torch.zeros((B, H, W, 2), device=dev)}


def census(model):
    """(flops sum, the launch sequence as one string) of what the handle timed since the last read."""
    from pointnav_vo_amd import _lib

    ent = (_lib.pnvo_kernel_time * 256)()
    n = C.c_int(0)
    _lib.check(_lib.lib.pnvo_timing_read(model._handle, ent, 256, C.byref(n)), model._handle)
    assert n.value <= 256
    names = [ent[i].name.decode().replace("visual_encoder.", "").replace("backbone.", "") for i in range(n.value)]
    return sum(ent[i].flops for i in range(n.value)), " ".join(f"{nm}*{ent[i].launches}" for i, nm in enumerate(names))


def section(out, seqs, model, options, batches, run):
    for key, value, default in options:
        out.append("O defaults" if key is None else f"O {key}={value}")
        for m in model if isinstance(model, tuple) else (model,):
            if key is not None:
                m.set_option(key, value)
        for B in batches:
            run(B)
            flops, seq = census(model[0] if isinstance(model, tuple) else model)
            if seq not in seqs:
                seqs[seq] = len(seqs)
                out.append(f"S{seqs[seq]}= {seq}")
            out.append(f"B {B} {flops:.0f} S{seqs[seq]}")
        for m in model if isinstance(model, tuple) else (model,):
            if key is not None:
                m.set_option(key, default)


def table(dev):
    from pointnav_vo_amd import vo_cnn

    out = []
    with torch.no_grad():
        for backbone, W, H, batches, options in MODELS:
            model = build(backbone, dev, W=W, H=H)
            model(inputs(1, dev, W, H))                            # creates the handle and loads the weights
            model.timing(True)
            census(model)
            out.append(f"M {backbone}_{W}x{H}")
            section(out, {}, model, options, batches, lambda B: model(inputs(B, dev, W, H)))
            model.timing(False)
            model._release()
        pair = (build("resnet18", dev).set_precision("bfloat16"), build("resnet18", dev, seed=7).set_precision("bfloat16"))
        vo_cnn.dual_forward(pair[0], pair[1], inputs(1, dev))
        pair[0].timing(True)
        census(pair[0])
        out.append(f"M dual_bf16_resnet18_{VO_W}x{VO_H}")
        section(out, {}, pair, DUAL_OPTIONS, DUAL_BATCHES, lambda B: vo_cnn.dual_forward(pair[0], pair[1], inputs(B, dev)))
        for m in pair:
            m._release()
    torch.cuda.synchronize(dev)
    return out


def check_coverage(rows):
    """Each pinned branch is taken by one case and not taken by another of the same model (module docstring)."""
    lines, seqs, model = {}, {}, None
    for r in rows:
        if r.startswith("M "):
            model, seqs = r[2:], {}
        elif r.startswith("S"):
            k, seq = r.split("= ", 1)
            seqs[k] = [w.rsplit("*", 1)[0] for w in seq.split()]
        elif r.startswith("B "):
            lines.setdefault(model, []).append(seqs[r.split()[3]])
    basic, r50, se, dual, small = (lines[k] for k in (f"resnet18_{VO_W}x{VO_H}", f"resnet50_{VO_W}x{VO_H}", f"se_resneXt50_{VO_W}x{VO_H}",
                                                     f"dual_bf16_resnet18_{VO_W}x{VO_H}", f"resnet18_{SMALL_W}x{SMALL_H}"))
    for name in ("pool_init", "gn_relu_maxpool", "gn_relu_apply", "residual"):
        assert any(name in ln for ln in basic) and any(name not in ln for ln in basic), name
    assert any("smallnet" in ln for ln in small) and any("smallnet" not in ln for ln in small) and not any("smallnet" in ln for ln in basic)
    assert any("bf16:residual" in ln for ln in dual) and any("bf16:residual" not in ln for ln in dual)
    gated = lambda ln: any(w.startswith("se_gate:") for w in ln)
    assert all(gated(ln) for ln in se) and not any(gated(ln) for ln in basic + r50)
    assert all("residual" in ln for ln in r50 + se)              # a Bottleneck block never hands its tail on


if __name__ == "__main__":
    rows = table(torch.device("cuda:0"))
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, "w") as f:
        f.write("\n".join(rows) + "\n")
    print(f"{len(rows)} lines")
    check_coverage(rows)
    print("coverage ok")
