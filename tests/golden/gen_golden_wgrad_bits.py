#!/usr/bin/env python
"""Generate tests/golden/wgrad_bits.txt on the MI355X: checksums of the BITS of the flat gradient and the loss of one training step,
case by case, so that a change of the weight-gradient dispatch (csrc/train_kernels.hip, wgrad_x3.hip, pnvo_train_api.hip) that moves
one bit of one gradient fails tests/test_gpu_wgrad_bits.py.

    python tests/golden/gen_golden_wgrad_bits.py

The file was written by a build of commit fc7ffff ("VO training step: sensor-frame entry from the dataset to the stem wgrad") plus
only a recorder's pnvo_wgrad_describe (tests/golden/gen_golden_wgrad_plans.py), the parent of the change that gave the weight
gradients one planner, one instance table and the option `wgrad`; the table was computed twice there and had to come out identical
(the training step has no float atomics).  That build knew PNVO_WGRAD only as a per-process environment variable, so there the two
`wgrad=` cases ran in child processes with the variable set (run_case_in_child); a build with the option sets it on the handle.
Regenerate the file only with a change that MEANS to change the arithmetic of the training step, from the commit before it.

A line is `<case> <tensor> <elements> <plain sum> <position-weighted sum>` — the checksum scheme of gen_golden_conv_x3_bits.py.

Cases (the smallest at which each path can go wrong):
    fix[:<options>]   one step (train-mode forward, loss, backward) of tests/golden/train_default_45x37_b4_f64.npz under the defaults,
                      conv=x3, conv=x3 train_pieces=3, conv=x3 wgrad3=fp32, wgrad=lds9, wgrad=generic, wgrad_stem=fp32 — and under
                      wgrad3=fp32 wgrad=lds9, the one setting at which the nine-wave kernel takes the stride-1 convs of this model (with
                      the matrix-core family allowed it takes them first, with the twelve-wave family allowed that one does)
    odd[:wgrad3=fp32] a seeded resnet18 VO model at 200 x 113 (50 x 29, 25 x 15, 13 x 8 and 7 x 4 maps: ragged tiles right and bottom,
                      odd maps under the stride-2 convs), 3 pairs, dropout 0.2, a seeded grad_out instead of a loss

Coverage (check_coverage, asserted on what the planner says ran): every weight-gradient request of every case is described
(pnvo_wgrad_describe on the problem csrc/pnvo_train_api.hip's wgrad_request builds for it, with the handle's options) and the union
must hit the matrix-core family at np 2 and 3, the twelve-wave and the nine-wave family at stride 1 and 2, the float32 stem kernel, the
generic kernel with tap groups of 9, 7, 1 and 6 or 3, and mode 1 on each of the three 3x3 kernel families (stride 1: a block's strided
conv is its first and reads a plain tensor).  Tap groups of 7 come from the hidden layer on the odd model's 4 x 7 feature map; the stem
itself reaches the generic kernel only with wgrad_stem=fp32 and wgrad=generic together, which no case sets.  The twelve-wave kernel runs
double-buffered (nbuf 2) in every case: no problem of tests/test_wgrad_plan.py's whole grid plans a single buffer.  The float16 form counts as permitted for the
second conv of a block when train_pieces is 2: the third condition, the forward's bound on the conv's input below 6.0e4, holds for these
seeded models by orders of magnitude and is not visible from here.  The stem's request is described only where it runs (wgrad_stem=fp32;
a 64-output stem, which no case here has: stem_is_a_request, used by tests/test_gpu_train_models.py, which runs `generic tg7 mode2`).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gen_golden_conv_x3_bits import checksum, rup  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "wgrad_bits.txt")
ODD_W, ODD_H, ODD_B = 200, 113, 3
SPACE = ["rgb", "depth", "discretized_depth", "top_down_view"]
FIX_CASES = ({}, {"conv": "x3"}, {"conv": "x3", "train_pieces": "3"}, {"conv": "x3", "wgrad3": "fp32"}, {"wgrad": "lds9"},
             {"wgrad": "generic"}, {"wgrad_stem": "fp32"}, {"wgrad3": "fp32", "wgrad": "lds9"})
ODD_CASES = ({}, {"wgrad3": "fp32"})
# field order of pnvo_wgrad_describe's problem array (include/pnvo.h)
FIELDS = ("B", "H", "W", "CIN", "Ho", "Wo", "COUT", "DYC", "KH", "KW", "stride", "pad", "mode", "np", "wgrad3", "wgrad")


def case_name(kind, opts):
    return kind + "".join(f":{k}={v}" for k, v in opts.items())


def stem_is_a_request(cfg, opts):
    """Does the stem's weight gradient go through the planner?  Not where the matrix-core stem kernel serves it: 32 stem outputs
    (backward_stem's l.coutp == 32; every modality layout of the registered models fits that kernel) and no wgrad_stem=fp32."""
    return opts.get("wgrad_stem", "mx") == "fp32" or cfg.baseplanes != 32


def request_names(cfg, opts):
    """The parameter each row of requests() is the weight gradient of, in the same order."""
    from pointnav_vo_amd import model_spec as ms

    names = [cd.name + ".weight" for k, cd in enumerate(ms.conv_plan(cfg)) if k or stem_is_a_request(cfg, opts)]
    return names + [("hidden_generator.1" if cfg.act_embed else "visual_fc.2") + ".weight", "output_head.1.weight"]


def requests(cfg, B, opts, dropout):
    """The problems of one backward's weight-gradient requests, as FIELDS rows (csrc/pnvo_train_api.hip: wgrad_request and its callers)."""
    from pointnav_vo_amd import model_spec as ms

    w3 = {"x3": 1, "fp32": 0}[opts.get("wgrad3", "x3")]
    wg = {"auto": 0, "lds9": 1, "generic": 2}[opts.get("wgrad", "auto")]
    f16 = opts.get("train_pieces", "2") == "2"
    rows = []
    for k, cd in enumerate(ms.conv_plan(cfg)):
        if k == 0 and not stem_is_a_request(cfg, opts):
            continue                                       # the matrix-core stem kernel is not a request of this planner
        block_conv = ".convs." in cd.name
        mode = 2 if k == 0 else 1 if block_conv and not cd.name.endswith(".convs.0") else 0
        rows.append((B, cd.hin, cd.win, 32 if k == 0 else cd.cin, cd.hout, cd.wout, cd.cout, rup(cd.cout, 32), cd.k, cd.k, cd.stride, cd.pad,
                     mode, 2 if block_conv and f16 else 3, w3, wg))
    fh, fw = cfg.final_hw
    rows.append((B, fh, fw, rup(cfg.comp_channels, 32), 1, 1, cfg.hidden, cfg.hidden, fh, fw, 1, 0, 0 if dropout else 1, 3, w3, wg))
    rows.append((B, 1, 1, cfg.hidden, 1, 1, cfg.out_dim, 8, 1, 1, 1, 0, 0, 3, w3, wg))
    return rows


def describe_requests(seen, cfg, B, opts, dropout):
    from pointnav_vo_amd import _lib

    buf = C.create_string_buffer(512)
    for row in requests(cfg, B, opts, dropout):
        q = np.ascontiguousarray(row, dtype=np.int32)
        _lib.check(_lib.lib.pnvo_wgrad_describe(q.ctypes.data_as(C.POINTER(C.c_int)), len(q), buf, len(buf)))
        seen.append((buf.value.decode(), row))


def fix_model(dev):
    from conftest import golden_case, load_golden
    from pointnav_vo_amd import vo_cnn  # noqa: F401  (registers the models)
    from pointnav_vo_amd.registry import baseline_registry

    rec = load_golden("train_default_45x37_b4_f64.npz")
    cfg, sd, obs, _ = golden_case(rec)
    model = baseline_registry.get_vo_model(str(rec["model"]))(
        observation_space=str(rec["obs_space"]).split(","), observation_size=(cfg.width, cfg.height), hidden_size=512, backbone="resnet18",
        normalize_visual_inputs=True, output_dim=3, dropout_p=0.0, discretized_depth_channels=int(rec["dd_bins"]))
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    tobs = {k: torch.from_numpy(v).to(dev) for k, v in obs.items()}
    return model.to(dev), tobs, dict(lr=float(rec["lr"]), eps=float(rec["eps"])), dict(target=torch.from_numpy(rec["target"]).to(dev))


def odd_model(dev):
    from pointnav_vo_amd import model_spec as ms, synth
    from pointnav_vo_amd import vo_cnn  # noqa: F401  (registers the models)
    from pointnav_vo_amd.registry import baseline_registry

    m = baseline_registry.get_vo_model("vo_cnn_rgb_d_dd_top_down")(
        observation_space=SPACE, observation_size=(ODD_W, ODD_H), hidden_size=512, backbone="resnet18", normalize_visual_inputs=True,
        output_dim=3, dropout_p=0.2, discretized_depth_channels=10)
    sd = synth.make_state_dict(ms.state_dict_spec(m.cfg), seed=ODD_W)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    obs = synth.make_obs_pairs(ODD_B, ODD_H, ODD_W, observation_space=SPACE, dd_bins=10, seed=ODD_H)
    grad_out = torch.from_numpy(np.random.default_rng(ODD_B).standard_normal((ODD_B, 3)).astype(np.float32)).to(dev)
    return m.to(dev), {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in obs.items()}, {}, dict(grad_out=grad_out)


def run_case(out, seen, kind, opts, dev):
    """One training step of a fresh model under `opts`; False: this build has no option `wgrad` (the caller runs the case in a child)."""
    from pointnav_vo_amd.train import VOTrainStep

    model, tobs, ts_kw, fb_kw = (fix_model if kind == "fix" else odd_model)(dev)
    model._ensure_handle(dev)
    try:
        for k, v in opts.items():
            if k == "wgrad" and os.environ.get("PNVO_WGRAD") == v and not has_wgrad_option(model):
                continue                                   # the recorder's child process: the environment already says it
            model.set_option(k, v)
        ts = VOTrainStep(model, **ts_kw)
        _, loss = ts.forward_backward(tobs, **fb_kw)
        torch.cuda.synchronize(dev)
        name = case_name(kind, opts)
        out.append("%s grad %d %d %d" % ((name,) + checksum(ts.grad)))
        if loss is not None:
            out.append("%s loss %d %d %d" % ((name,) + checksum(loss.detach().reshape(1).to(torch.float32))))
        B = next(iter(tobs.values())).shape[0]
        describe_requests(seen, model.cfg, B, opts, dropout=kind == "odd")
        del ts
    finally:
        model._release()


def has_wgrad_option(model):
    try:
        model.get_option("wgrad")
        return True
    except Exception:
        return False


def run_case_in_child(out, seen, kind, opts):
    env = dict(os.environ, PNVO_WGRAD=opts["wgrad"])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, ",".join(f"{k}={v}" for k, v in opts.items())], env=env, check=True, capture_output=True,
                       text=True, timeout=300)
    for l in r.stdout.splitlines():
        if l.startswith("LINE "):
            out.append(l[5:])
        elif l.startswith("SEEN "):
            text, _, row = l[5:].rpartition(" @ ")
            seen.append((text, tuple(map(int, row.split(",")))))


def table(dev, seen=None):
    """The file's lines; `seen` (a list) receives (describe line, problem) of every weight-gradient request of every case."""
    out, seen = [], [] if seen is None else seen
    probe, _, _, _ = fix_model(dev)
    probe._ensure_handle(dev)
    in_process = has_wgrad_option(probe)
    probe._release()
    for kind, cases in (("fix", FIX_CASES), ("odd", ODD_CASES)):
        for opts in cases:
            if "wgrad" in opts and not in_process:
                run_case_in_child(out, seen, kind, opts)
            else:
                run_case(out, seen, kind, opts, dev)
    return out


def check_coverage(seen):
    inst = {text.split(" | ")[0] for text, _ in seen}
    need = ["x3 mode0 np2", "x3 mode1 np2", "x3 mode0 np3", "x3 mode1 np3", "mw12 mode0 s1", "mw12 mode1 s1", "mw12 mode0 s2", "lds9 mode0 s1",
            "lds9 mode1 s1", "lds9 mode0 s2", "stem_lds", "generic tg9 mode0", "generic tg1 mode0"]
    missing = [n for n in need if n not in inst]
    assert not missing, (missing, sorted(inst))
    assert any(i.startswith("generic tg7 ") for i in inst), sorted(inst)
    assert any(i.startswith("generic tg6 ") or i.startswith("generic tg3 ") for i in inst), sorted(inst)   # the hidden layer


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    if len(sys.argv) > 3 and sys.argv[1] == "--child":
        out, seen = [], []
        run_case(out, seen, sys.argv[2], dict(kv.split("=") for kv in sys.argv[3].split(",")), dev)
        for l in out:
            print("LINE " + l)
        for text, row in seen:
            print("SEEN " + text + " @ " + ",".join(map(str, row)))
        sys.exit(0)
    seen = []
    rows = table(dev, seen)
    again = table(dev)
    assert rows == again, [(a, b) for a, b in zip(rows, again) if a != b]
    print("two runs identical")
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, "w") as f:
        f.write("\n".join(rows) + "\n")
    print(f"{len(rows)} lines")
    for k in sorted({text for text, _ in seen}):
        print("request:", k)
    check_coverage(seen)
    print("coverage ok")
