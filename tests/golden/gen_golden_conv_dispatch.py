#!/usr/bin/env python
"""Generate tests/golden/conv_dispatch.txt on the MI355X: which kernel family runs every residual-stage conv, and the matrix-core
FLOPs it executes, at every batch size 1 .. 256 — read through pnvo_layer_kernel only (no forward runs).

    python tests/golden/gen_golden_conv_dispatch.py

The table pins the host's dispatch: tests/test_gpu_conv_dispatch.py recomputes it (table() below) and compares line for line, so a
change of the dispatch code that moves one layer at one batch size under one option fails there.  Regenerate it only with a change
that means to move a threshold, from the commit before a refactor of the dispatch otherwise.

Models: the benchmark's VO model (bench.build_model) and the Bottleneck, ResNeXt and SE-ResNeXt VO models of
tests/test_gpu_backbone_regimes.py at 68 x 52.  Option sets: OPTION_SETS, one option off its default at a time.

Format.  `M <model>` and `O <option>=<value>` open a section; a layer line is
    <conv name without "visual_encoder."> <family>:<executed FLOPs per sample>*<run length> ...
run-length coded over B = 1 .. 256 (executed FLOPs are B times a plan constant in every branch: the per-sample value is an exact
integer).  Sections other than `O defaults` list only the layers whose line differs from the defaults' and close with `same <count>`.
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

PATH = os.path.join(ROOT, "tests", "golden", "conv_dispatch.txt")
BMAX = 256
BACKBONES = ("resnet50", "resneXt50", "se_resneXt50")
VO_W, VO_H = 68, 52
# (option, value, the default it returns to)
OPTION_SETS = [(None, None, None), ("conv", "x3", "auto"), ("conv", "fp32", "auto"), ("conv", "generic", "auto"), ("x3_rows", "off", "on"),
               ("x3_fine", "off", "on"), ("pieces", "3", "2"), ("ds_fuse", "off", "on"), ("small_net", "off", "on")]


def models(dev):
    """(name, model) one at a time; the caller releases it."""
    import backbone_reference as BR
    import bench
    from pointnav_vo_amd import synth
    from pointnav_vo_amd.vo_cnn import VisualOdometryCNNBase

    yield "bench", bench.build_model(dev)[0]
    for bb in BACKBONES:
        cfg, spec = BR.vo_spec(bb, VO_W, VO_H)
        v = BR.VO
        model = VisualOdometryCNNBase(observation_space=list(v["space"]), observation_size=(VO_W, VO_H), hidden_size=v["hidden"], backbone=bb,
                                      normalize_visual_inputs=True, output_dim=3, discretized_depth_channels=v["dd_bins"])
        sd = synth.make_state_dict(spec, seed=v["seed"])
        model.load_state_dict({k: torch.from_numpy(np.array(t)) for k, t in sd.items()})
        yield f"{bb}_{VO_W}x{VO_H}", model.to(dev).eval()


def layer_line(model, name):
    from pointnav_vo_amd import _lib

    buf, fl = C.create_string_buffer(32), C.c_double(0.0)
    runs = []
    for B in range(1, BMAX + 1):
        _lib.check(_lib.lib.pnvo_layer_kernel(model._handle, name.encode(), B, buf, 32, C.byref(fl)), model._handle)
        per = fl.value / B
        assert per == int(per) and int(per) * B == fl.value, (name, B, fl.value)
        key = f"{buf.value.decode()}:{int(per)}"
        if runs and runs[-1][0] == key:
            runs[-1][1] += 1
        else:
            runs.append([key, 1])
    return name[len("visual_encoder."):] + " " + " ".join(f"{k}*{n}" for k, n in runs)


def table(dev):
    from pointnav_vo_amd import model_spec as ms

    out = []
    for mname, model in models(dev):
        assert model._options == {}
        names = [cd.name for cd in ms.conv_plan(model.cfg)[1:]]
        model.layer_kernel(names[0], 1)              # creates the handle and loads the weights; the loop below calls the library directly
        out.append(f"M {mname}")
        base = None
        for key, value, default in OPTION_SETS:
            if key is not None:
                model.set_option(key, value)
            lines = [layer_line(model, n) for n in names]
            if key is not None:
                model.set_option(key, default)
            if base is None:
                base = lines
                out += ["O defaults"] + lines
            else:
                diff = [ln for ln, b in zip(lines, base) if ln != b]
                out += [f"O {key}={value}"] + diff + [f"same {len(lines) - len(diff)}"]
        model._release()
    return out


if __name__ == "__main__":
    rows = table(torch.device("cuda:0"))
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, "w") as f:
        f.write("\n".join(rows) + "\n")
    print(f"{len(rows)} lines")
