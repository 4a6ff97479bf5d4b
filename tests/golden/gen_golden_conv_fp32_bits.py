#!/usr/bin/env python
"""Generate tests/golden/conv_fp32_bits.txt on the MI355X: checksums of the BITS of what the float32-MFMA kernels (csrc/conv_mfma.hip:
conv_mfma_kernel in all its flavours with the split-K reductions; csrc/conv3_lds.hip: conv3_lds_kernel, conv3_wave_kernel) compute,
case by case.

    python tests/golden/gen_golden_conv_fp32_bits.py

tests/test_gpu_conv_fp32_bits.py recomputes the table (table() below) and compares it line by line, so a change of those kernels or of
what is launched for a layer that moves one bit of one output, hidden feature, block output or training gradient fails there.  The file
was written by a build of commit 2152deb ("Test the VO training step of every model variant against fp64"), the parent of the change
that gave this kernel family one problem, one plan and one instance table: host code only, the kernels and what is launched unchanged.
That build read the family's five knobs from the environment into function-local statics, once per process, so this script — run as a
program — computes the lines of each option set in a child process of its own with that set's PNVO_* variables in the environment; the
test sets the same values as options of the handle (fp32_tile, fp32_wsplit, fp32_form, wave_wgs, wave_nt) in ONE process, which is what
moving them onto the handle made possible.  Regenerate the file only with a change that MEANS to change the arithmetic of these kernels
or their selection, from the commit before any other change of them.

A line is
    <case> <tensor> <elements> <plain sum> <position-weighted sum>
(the scheme and helpers of gen_golden_conv_x3_bits.py: both sums over the tensor's 32-bit patterns in wrapping 32-bit integer
arithmetic, taken on the device; the weight of element i is i + 1).

Cases (the smallest that reach each path), `k` = index of the option set (test_conv_fp32_plan.option_sets: the defaults, then the
float32-MFMA settings of test_gpu_knobs.KNOBS):
    <g>:<base>:o<k>        the three golden models of test_gpu_knobs.CHECK — g = d341 (341 x 192, 2 pairs), d45 (45 x 37, 3), w64 (wider,
                           64 x 48, 2) — under base = fp32 (conv=fp32), gen (conv=generic) and dense (stem=dense), with every option set:
                           output and hidden features; under fp32 with the default set also every block output and the pooled stem output
    odd:o<k>               a resnet18 model at 200 x 113, 3 pairs, conv=fp32: 50 x 29, 25 x 15, 13 x 8 and 7 x 4 maps — ragged LDS tiles —
                           with every option set (the default set also with the block taps)
    r50:auto:o<k>, r50:fp32  the resnet50 model of tests/golden/gen_golden_forward_census.py at 68 x 52, 9 pairs (the size of a policy's
                           encoder input) with every option set, and under conv=fp32 with the default set: the 1x1 convs of the Bottleneck
                           blocks on the generic kernel, plain and behind a GroupNorm
    fc:head / fc:plain     d45 with conv=fp32 and fc_rows=0 (the Linear layers on the MFMA kernel at 3 pairs): the hidden layer's split-K
                           reduction with the output head riding on it, and (head_fuse=off) the plain reduction + the head's own split-K launch
    train / train:masked   one training step (forward in train mode, backward) of tests/golden/train_default_45x37_b4_f64.npz with
                           conv=fp32, and again with dgrad=masked: flat gradient and loss — the parity-phase and the full backward-data
                           convs (strided output, upsampled input, accumulate) and the transposed Linears

Coverage (check_coverage, asserted on what ran, not on what was meant): from the kernel family pnvo_layer_kernel reports for every conv
of every forward case and the plan pnvo_conv_fp32_describe names for the problem that launch states (and for the Linear layers,
backward-data convs and transposed Linears of the fc and train cases), the cases reach operand modes 0 / 1, FEAT 0 / 1 / 2, a split-K
launch with the plain reduction and one with the riding head, both LDS-staged kernels and each of their instantiated tile shapes, and the
resnet50 case runs 1x1 convs on the generic kernel in both modes; what they do not reach is named in UNREACHED with the reason.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gen_golden_conv_x3_bits import BLOCK_TAPS, checksum, features, rup, tap  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "conv_fp32_bits.txt")
GOLDENS = (("d341", "model_default_341x192_b2.npz"), ("d45", "model_default_45x37_b3.npz"), ("w64", "model_wider_64x48_b2.npz"))
BASES = (("fp32", {"conv": "fp32"}), ("gen", {"conv": "generic"}), ("dense", {"stem": "dense"}))
SPACE = ["rgb", "depth", "discretized_depth", "top_down_view"]
OPTION_OF = {"tile": "fp32_tile", "wsplit": "fp32_wsplit", "form": "fp32_form", "wave_wgs": "wave_wgs", "wave_nt": "wave_nt"}
WORDS = {"form": {0: "auto", 1: "tile", 2: "wave"}, "wsplit": {-1: "auto", 0: "off", 1: "on"}}


def option_sets():
    import test_conv_fp32_plan as t

    return t.option_sets()


def apply_options(model, o, how):
    """Option set o on the model's handle (how = "option"); how = "env": the process was started with o's PNVO_* variables (a build that
    reads them into statics), nothing to set."""
    if how == "option":
        for field, name in OPTION_OF.items():
            model.set_option(name, WORDS.get(field, {}).get(o[field], str(o[field])))


def golden_model(fname, dev):
    from conftest import golden_case, load_golden
    from pointnav_vo_amd import vo_cnn  # noqa: F401  (registers the models)
    from pointnav_vo_amd.registry import baseline_registry

    rec = load_golden(fname)
    cfg, sd, obs, _ = golden_case(rec)
    kw = dict(observation_space=str(rec["obs_space"]).split(","), observation_size=(cfg.width, cfg.height), hidden_size=512,
              backbone="resnet18", normalize_visual_inputs=True, output_dim=3, dropout_p=0.2)
    if int(rec["dd_bins"]):
        kw["discretized_depth_channels"] = int(rec["dd_bins"])
    m = baseline_registry.get_vo_model(str(rec["model"]))(**kw)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return m.to(dev).eval(), {k: torch.from_numpy(v).to(dev) for k, v in obs.items()}, rec["out64"]


def synth_model(dev, size, B):
    from pointnav_vo_amd import model_spec as ms, synth
    from pointnav_vo_amd import vo_cnn  # noqa: F401  (registers the models)
    from pointnav_vo_amd.registry import baseline_registry

    m = baseline_registry.get_vo_model("vo_cnn_rgb_d_dd_top_down")(
        observation_space=SPACE, observation_size=size, hidden_size=512, backbone="resnet18", normalize_visual_inputs=True, output_dim=3,
        dropout_p=0.2, discretized_depth_channels=10)
    sd = synth.make_state_dict(ms.state_dict_spec(m.cfg), seed=size[0])
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    obs = synth.make_obs_pairs(B, size[1], size[0], observation_space=SPACE, dd_bins=10, seed=size[1])
    return m.to(dev).eval(), {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in obs.items()}


def r50_model(dev, B=9):
    """The forward census's resnet50 VO model (rgb + depth, 68 x 52) with drawn inputs."""
    import backbone_reference as BR
    import gen_golden_forward_census as census
    from pointnav_vo_amd import synth

    obs = synth.make_obs_pairs(B, census.VO_H, census.VO_W, observation_space=list(BR.VO["space"]), dd_bins=1, seed=census.VO_H)
    return census.build("resnet50", dev), {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in obs.items()}


def describe(**f):
    import test_conv_fp32_plan as t
    from pointnav_vo_amd import _lib

    q = np.ascontiguousarray(t.problem_of(**f), dtype=np.int32)
    buf = C.create_string_buffer(512)
    _lib.check(_lib.lib.pnvo_conv_fp32_describe(q.ctypes.data_as(C.POINTER(C.c_int)), len(q), buf, len(buf)))
    return buf.value.decode()


def forward_launches(model, B, o, generic, linear=None, ks=None):
    """Plan lines of the float32-MFMA launches of one untapped forward at B pairs under option set o: for every conv that
    pnvo_layer_kernel puts on that family, the planner's answer for the problem the schedule states (csrc/pnvo_api.hip run_conv_fp32 —
    no block tail reaches these kernels: a block's first conv, a downsample conv and the compression conv read final activations, mode
    0; the others read a raw tensor through its GroupNorm, mode 1).  linear = "head" / "plain": also the hidden layer and, without the
    riding head, the output head (option fc_rows=0).  ks: only the convs of that kernel size."""
    from pointnav_vo_amd import model_spec as ms

    cfg, out = model.cfg, []
    for cd in ms.conv_plan(cfg)[1:]:
        if model.layer_kernel(cd.name, B)[0] not in ("fp32-lds", "fp32-generic") or (ks is not None and cd.k != ks):
            continue
        first = cd.name.endswith(".convs.0") or ".downsample." in cd.name or "compression" in cd.name
        out.append(describe(B=B, H=cd.hin, W=cd.win, CIN=rup(cd.cin, 8), Ho=cd.hout, Wo=cd.wout, COUT=cd.cout, KH=cd.k, KW=cd.k, stride=cd.stride,
                            pad=cd.pad, mode=0 if first else 1, lds_ok=0 if generic else 1, **o))
    if linear is not None:
        fh, fw = cfg.final_hw
        out.append(describe(B=B, H=fh, W=fw, CIN=rup(cfg.comp_channels, 32), Ho=1, Wo=1, COUT=cfg.hidden, KH=fh, KW=fw, pad=0, stats=0, mode=1,
                            y_cstride=cfg.hidden, linear=1, ksplit_ok=1, head=cfg.out_dim if linear == "head" else 0, lds_ok=0, **o))
        if linear == "plain":
            out.append(describe(B=B, H=1, W=1, CIN=cfg.hidden, Ho=1, Wo=1, COUT=cfg.out_dim, KH=1, KW=1, pad=0, stats=0, y_cstride=cfg.out_dim,
                                linear=1, ksplit_ok=1, lds_ok=0, **o))
    return out


def backward_launches(cfg, B, o, phases):
    """Plan lines of one backward under conv=fp32 (csrc/pnvo_train_api.hip dgrad_problem / linear_t_problem): every conv's backward-data
    conv — the first block's first conv accumulates into the pooled gradient's buffer only where a skip joins, which the plan does not
    look at beyond the flag: both are listed — and the two transposed Linears."""
    from pointnav_vo_amd import model_spec as ms

    out = []
    for cd in ms.conv_plan(cfg)[1:]:
        for accum in (0, 1):
            base = dict(B=B, H=cd.hout, W=cd.wout, CIN=rup(cd.cout, 32), COUT=cd.cin, stats=0, y_cstride=cd.cin, accum=accum, **o)
            if phases and cd.k == 3 and cd.stride == 2:
                for ph, pw in ((0, 0), (0, 1), (1, 0), (1, 1)):
                    ho, wo = (cd.hin - ph + 1) // 2, (cd.win - pw + 1) // 2
                    if ho > 0 and wo > 0:
                        out.append(describe(Ho=ho, Wo=wo, KH=2 if ph else 1, KW=2 if pw else 1, pad=0, y_sh=2, y_sw=2, y_oh=ph, y_ow=pw, y_H=cd.hin,
                                            y_W=cd.win, lds_ok=0, **base))
            else:
                out.append(describe(Ho=cd.hin, Wo=cd.win, KH=cd.k, KW=cd.k, pad=cd.k - 1 - cd.pad, up=cd.stride, lds_ok=1, **base))
    fh, fw = cfg.final_hw
    n = fh * fw * rup(cfg.comp_channels, 32)
    for cin, cout in ((8, cfg.hidden), (cfg.hidden, n)):
        out.append(describe(B=B, H=1, W=1, CIN=cin, Ho=1, Wo=1, COUT=cout, KH=1, KW=1, pad=0, stats=0, y_cstride=cout, lds_ok=0, **o))
    return out


def forward_case(out, case, model, obs, taps):
    B = next(iter(obs.values())).shape[0]
    with torch.no_grad():
        for name, t in [("output", model(obs)), ("features", features(model, obs))] + [(n, tap(model, n, obs, B)) for n in taps]:
            out.append("%s %s %d %d %d" % ((case, name) + checksum(t)))
    return B


def train_case(out, seen, dev, o, how):
    from conftest import golden_case, load_golden
    from pointnav_vo_amd import vo_cnn  # noqa: F401  (registers the models)
    from pointnav_vo_amd.registry import baseline_registry
    from pointnav_vo_amd.train import VOTrainStep

    rec = load_golden("train_default_45x37_b4_f64.npz")
    cfg, sd, obs, _ = golden_case(rec)
    for case, dgrad in (("train", "phase"), ("train:masked", "masked")):
        model = baseline_registry.get_vo_model(str(rec["model"]))(
            observation_space=str(rec["obs_space"]).split(","), observation_size=(cfg.width, cfg.height), hidden_size=512, backbone="resnet18",
            normalize_visual_inputs=True, output_dim=3, dropout_p=0.0, discretized_depth_channels=int(rec["dd_bins"]))
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        model = model.to(dev)
        model._ensure_handle(dev)
        model.set_option("conv", "fp32")
        model.set_option("dgrad", dgrad)
        apply_options(model, o, how)
        ts = VOTrainStep(model, lr=float(rec["lr"]), eps=float(rec["eps"]))
        tobs = {k: torch.from_numpy(v).to(dev) for k, v in obs.items()}
        _, loss = ts.forward_backward(tobs, target=torch.from_numpy(rec["target"]).to(dev))
        torch.cuda.synchronize(dev)
        out.append("%s grad %d %d %d" % ((case,) + checksum(ts.grad)))
        out.append("%s loss %d %d %d" % ((case,) + checksum(loss.detach().reshape(1).to(torch.float32))))
        if seen is not None:
            seen.extend(backward_launches(model.cfg, 4, o, dgrad == "phase"))
        del ts, model


def table(dev, seen=None, how="option", only=None):
    """The file's lines.  `seen` (a list) receives the plan lines of the float32-MFMA launches of the cases (needs this build's
    pnvo_conv_fp32_describe); how: see apply_options; only = k: the lines of option set k alone (the recorder's child processes)."""
    out, sets = [], option_sets()
    models = {}

    def model_of(name, make):
        if name not in models:
            models[name] = make()
        return models[name]

    for k, o in enumerate(sets):
        if only is not None and k != only:
            continue
        for g, fname in GOLDENS:
            model, obs, _ = model_of(g, lambda: golden_model(fname, dev))
            apply_options(model, o, how)
            for base, opts in BASES:
                for key, value in opts.items():
                    model.set_option(key, value)
                B = forward_case(out, f"{g}:{base}:o{k}", model, obs, BLOCK_TAPS if (base == "fp32" and k == 0) else ())
                if seen is not None:
                    seen.extend(forward_launches(model, B, o, base == "gen"))
                for key in opts:
                    model.set_option(key, "auto")
        m, oobs = model_of("odd", lambda: synth_model(dev, (200, 113), 3))
        apply_options(m, o, how)
        m.set_option("conv", "fp32")
        B = forward_case(out, f"odd:o{k}", m, oobs, BLOCK_TAPS if k == 0 else ())
        if seen is not None:
            seen.extend(forward_launches(m, B, o, False))
        m, robs = model_of("r50", lambda: r50_model(dev))
        apply_options(m, o, how)
        for conv in ("auto", "fp32") if k == 0 else ("auto",):
            m.set_option("conv", conv)
            B = forward_case(out, f"r50:auto:o{k}" if conv == "auto" else "r50:fp32", m, robs, ())
            if seen is not None:
                ones = forward_launches(m, B, o, False, ks=1)      # the Bottleneck blocks' 1x1 convs: generic kernel, both operand modes
                assert ones and all(l.startswith("generic ") for l in ones), ones
                assert any(" mode0 " in l for l in ones) and any(" mode1 " in l for l in ones), ones
                seen.extend(forward_launches(m, B, o, False))
        m.set_option("conv", "auto")
        if k != 0:
            continue
        # the cases that run under the default option set alone
        m, fobs, _ = golden_model(GOLDENS[1][1], dev)
        apply_options(m, o, how)
        m.set_option("conv", "fp32")
        m.set_option("fc_rows", "0")
        for case, fuse in (("head", "on"), ("plain", "off")):
            m.set_option("head_fuse", fuse)
            B = forward_case(out, f"fc:{case}", m, fobs, ())
            if seen is not None:
                seen.extend(forward_launches(m, B, o, False, linear=case))
        m._release()
        train_case(out, seen, dev, o, how)
    for m in models.values():
        m[0]._release()
    torch.cuda.synchronize(dev)
    return out


# What no case reaches, with the reason (checked on the commit the golden was recorded from).
UNREACHED = {
    "mode2": "the generic kernel's observation-tensor fetch runs only for a stem stem_lds.hip does not serve (more than 32 input channels, "
             "or a stem that is not 32 / 64 channels wide); no model the suite builds has one",
}


def check_coverage(seen):
    """Operand modes, FEATs, both reductions, both LDS-staged kernels and each of their tile shapes are reached by a launch of the cases
    (module docstring)."""
    keys = sorted({l.split(" | ")[0] for l in seen if l != "none"})
    assert "none" not in seen, "a case states a problem the planner refuses"
    generic = [k for k in keys if k.startswith("generic ")]
    for mode in (0, 1, 2):
        assert any(f" mode{mode} " in k for k in generic) != (f"mode{mode}" in UNREACHED), (f"conv_mfma_kernel launches with operand mode {mode}", keys)
    for feat in (0, 1, 2):
        assert any(k.endswith(f" feat{feat}") for k in generic), (f"no conv_mfma_kernel launch with FEAT {feat}", keys)
    for red in ("plain", "head"):
        assert any(f" reduce {red} " in l for l in seen), (f"no split-K launch with the {red} reduction", keys)
    want = [f"lds_tile blk{b} wy{wy} wx{wx} " for b, wy, wx in ((0, 4, 1), (1, 3, 1), (0, 3, 1))]
    want += [f"lds_wave blk{b} nt{nt} mode{mode} mt{mt}" for b, nt, mt in ((0, 1, 1), (0, 1, 2), (0, 2, 1), (1, 1, 1), (1, 2, 1)) for mode in (0, 1)]
    for w in want:
        if w.strip() in UNREACHED:
            assert not any(k.startswith(w) for k in keys), (w, "is reached: take it out of UNREACHED")
        else:
            assert any(k.startswith(w) for k in keys), (f"no launch of {w.strip()}", keys)


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        print("\n".join("ROW " + r for r in table(dev, None, "env", only=int(sys.argv[2]))))
        sys.exit(0)
    import gen_golden_conv_fp32_plans as plans

    rows = []
    for k, o in enumerate(option_sets()):
        env = {n: v for n, v in os.environ.items() if not n.startswith("PNVO_")}
        env.update(plans.option_env(o))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(k)], env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:                # a failed step ends the run: nothing more is started on the GPU
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(r.returncode if r.returncode > 0 else 1)
        got = [l[4:] for l in r.stdout.splitlines() if l.startswith("ROW ")]
        rows += got
        print(f"option set {k} {o}: {len(got)} lines", flush=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, "w") as f:
        f.write("\n".join(rows) + "\n")
    print(f"{len(rows)} lines")
