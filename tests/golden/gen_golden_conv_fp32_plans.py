#!/usr/bin/env python
"""Generate tests/golden/conv_fp32_plans.txt.xz (CPU only): one line of pnvo_conv_fp32_describe for every problem of
tests/test_conv_fp32_plan.py's grid, in that module's compact run-length format, xz-compressed.

    python tests/golden/gen_golden_conv_fp32_plans.py

The file was written from commit 2152deb ("Test the VO training step of every model variant against fp64"), the parent of the change
that gave the float32-MFMA convs one problem, one plan and one instance table.  That commit had no describe entry; the recorder linked
one on top of its UNCHANGED choose_tile / conv_slots / conv_wsplit / conv_ksplit / conv3_lds_supported / conv3_lds_slots / pick_cfg /
wave_blk / wave_mt / use_wave_kernel: the callers' rules (conv_choice, run_conv_fp32, run_dgrad: the LDS-staged kernel where it is
allowed and supported, n-tiles per wave from the layer's n-tile count, the split-K query of the Linear layers, the head riding on the
reduction) and a literal transcription of the launch_conv / launch_t / launch_conv3_lds / launch_cfg / launch_wave ladders for the
template instance, grid, block size, LDS bytes, the LDS table floats and the reduce launch ("none" where a ladder returned
hipErrorInvalidValue).  Those functions read PNVO_CONV_TILE, PNVO_CONV_WSPLIT, PNVO_CONV3, PNVO_WAVE_WGS and PNVO_WAVE_NT from the
environment into function-local statics, once per process, so the grid points of each option set are described by a child process of
their own with the variables of that set in its environment (the recorder ignored the option fields of the problem array); today the
fields alone decide and the planner reads no environment, but the recorder still runs that way.
Regenerate the file only with a change that MEANS to change what the planner chooses.
"""
import lzma
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FORM_WORDS = {1: "tile", 2: "wave"}


def option_env(o):
    """The environment of option set o: a variable only where o leaves the default."""
    import test_conv_fp32_plan as t

    env = {}
    for name, (field, _) in t.ENV.items():
        if o[field] != t.OPT_DEFAULTS[field]:
            env[name] = FORM_WORDS[o[field]] if field == "form" else str(o[field])
    return env


def rows_of(t, g, o):
    at = [t.FIELDS.index(k) for k in t.OPT_DEFAULTS]
    want = [o[k] for k in t.OPT_DEFAULTS]
    return [i for i in range(len(g)) if g[i, at].tolist() == want]


def child(k):
    import test_conv_fp32_plan as t

    g = t.grid()
    for line in t.describe_all(g[rows_of(t, g, t.option_sets()[k])]):
        print(line.decode())


def main(path):
    import test_conv_fp32_plan as t

    g = t.grid()
    out = [None] * len(g)
    for k, o in enumerate(t.option_sets()):
        env = {n: v for n, v in os.environ.items() if n not in t.ENV}
        env.update(option_env(o))
        got = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(k)], env=env, check=True, capture_output=True,
                             text=True).stdout.splitlines()
        at = rows_of(t, g, o)
        assert len(got) == len(at), (o, len(got), len(at))
        for i, l in zip(at, got):
            out[i] = l
    assert None not in out
    parts, lines, runs = {}, {}, []
    for l in out:
        ids = tuple(parts.setdefault(p, len(parts)) for p in l.split(" | "))
        n = lines.setdefault(ids, len(lines))
        if runs and runs[-1][0] == n:
            runs[-1][1] += 1
        else:
            runs.append([n, 1])
    with lzma.open(path, "wt", preset=9) as f:
        for text, n in parts.items():
            f.write(f"P {n} {text}\n")
        for ids, n in lines.items():
            f.write(f"= {n} " + " ".join(map(str, ids)) + "\n")
        for k in range(0, len(runs), 64):
            f.write("@ " + " ".join(f"{n}:{c}" for n, c in runs[k:k + 64]) + "\n")
    print(f"{len(out)} grid points, {len(lines)} distinct lines, {len(parts)} parts, {os.path.getsize(path)} bytes")
    for inst in sorted({l.split(" | ")[0] for l in out}):
        print("reached:", inst)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "conv_fp32_plans.txt.xz"))
