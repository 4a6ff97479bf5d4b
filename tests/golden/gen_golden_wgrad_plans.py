#!/usr/bin/env python
"""Generate tests/golden/wgrad_plans.txt.xz (CPU only): one line of pnvo_wgrad_describe for every problem of tests/test_wgrad_plan.py's
grid, in that module's compact run-length format, xz-compressed.

    python tests/golden/gen_golden_wgrad_plans.py

The file was written from commit fc7ffff ("VO training step: sensor-frame entry from the dataset to the stem wgrad"), the parent of
the change that gave the weight gradients one planner and one instance table.  That commit had no describe entry; the recorder linked
one on top of its UNCHANGED wgrad_plan / wgrad_plan_mw / wgrad_x3_plan: the planned WgradArgs printed field by field, a literal
transcription of the launch_wgrad / launch_wgrad_x3 ladders for the template instance, grid, block size, LDS bytes and the reduce
launch, and backward_block's rule for the float16 form (np = 2 exactly when the plan is the matrix-core one and the caller permits it).
That planner read PNVO_WGRAD from the environment once per process, so the grid points of each `wgrad` value are described by a child
process of their own with the variable set to that value (the entry of that build refused a problem whose `wgrad` field disagreed with
the environment); today the field alone decides and the variable is not read by the planner, but the recorder still runs that way.
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


def child(wg):
    import test_wgrad_plan as t

    g = t.grid()
    for row in g[g[:, t.FIELDS.index("wgrad")] == wg]:
        print(t.describe(row))


def main(path):
    import test_wgrad_plan as t

    g = t.grid()
    col = g[:, t.FIELDS.index("wgrad")]
    out = [None] * len(g)
    for word, wg in t.WGRAD.items():
        env = dict(os.environ)
        env.pop("PNVO_WGRAD", None)
        if wg:
            env["PNVO_WGRAD"] = word
        got = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(wg)], env=env, check=True, capture_output=True,
                             text=True).stdout.splitlines()
        at = [i for i in range(len(g)) if col[i] == wg]
        assert len(got) == len(at), (word, len(got), len(at))
        for i, l in zip(at, got):
            out[i] = l
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
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "wgrad_plans.txt.xz"))
