"""CPU: the conv_x3 planner (problem -> plan -> instance table, pointnav-vo_amd/csrc/conv_x3.hip) over a grid of problems, through the
host-only entry pnvo_conv_x3_describe, against tests/golden/conv_x3_plans.txt.

The golden was recorded from the planner of the commit BEFORE the refactor (conv_x3_plan + conv_x3_persistent + conv_rows32_plan and a
transcription of launch_ks's (mode, mw, nw, flags) -> template-instance mapping, linked against that commit's objects), so it pins
kernel selection, geometry, grid, block size and LDS bytes of every grid point to what the project launched before.

Grid (in this order, the last axis fastest):
    shape   every 3x3 (stride 1 / 2, pad 1) and 1x1 stride-2 conv behind the stem of the default model and of the baseplanes-16 and
            baseplanes-64 configs at 341 x 192, forward, and the backward-data problem of every 3x3 stride-1 conv with a 32-multiple of
            input channels (input and output channels and sizes swapped), duplicates dropped
    np      2, 3
    mode    stager modes 0-3
    ds      without / with a riding downsample conv
    B       BATCHES
    opts    the defaults, then each of the seven plan options flipped alone (the first flip is `force` on)
    tail    without / with a tail skip that carries its own scale
Forward defaults: every option on (force off), the rows form allowed, 256 CUs.  Backward-data defaults are what the training step
passes: fine, W8, M16 and K-split off, no rows form, and the gradient's absolute-maximum record with two-piece operands.

File format: `P n <text>` defines part n; `= n a b c` defines distinct line n as parts a, b, c joined by " | " (family and instance
key | grid, block, LDS bytes | geometry and slots); `@ n:c n:c ...` appends runs (c consecutive grid points map to line n).
"""
import ctypes as C
import itertools
import os

import numpy as np

from conftest import ROOT
from pointnav_vo_amd import _lib, model_spec as ms

GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_x3_plans.txt")
BATCHES = [1, 2, 7, 8, 12, 16, 17, 32, 33, 47, 48, 63, 64, 65, 111, 112, 128, 199, 200, 223, 224, 256]
SPACE = ["rgb", "depth", "discretized_depth", "top_down_view"]
NUM_CUS = 256
OPTS = ("force", "strip", "fine", "w8", "m16", "ksw", "persist_wgs")
FWD_DEFAULTS = dict(force=0, strip=1, fine=1, w8=1, m16=1, ksw=1, persist_wgs=3 * NUM_CUS, rows=1)
BWD_DEFAULTS = dict(force=0, strip=1, fine=0, w8=0, m16=0, ksw=0, persist_wgs=3 * NUM_CUS, rows=0)
# field order of pnvo_conv_x3_describe's problem array (include/pnvo.h)
FIELDS = ("B", "H", "W", "CIN", "Ho", "Wo", "COUTP", "ks", "stride", "np", "mode", "tail_scaled", "absmax", "ds",
          "force", "strip", "fine", "w8", "m16", "ksw", "persist_wgs", "rows", "num_cus")


def rup(x, m):
    return (x + m - 1) // m * m


def config(baseplanes):
    return ms.config_from_kwargs(observation_space=SPACE, observation_size=(341, 192), hidden_size=512, backbone="resnet18",
                                 resnet_baseplanes=baseplanes, normalize_visual_inputs=True, output_dim=3,
                                 discretized_depth_channels=10)


def eligible(cd):
    return (cd.k == 3 and cd.pad == 1 and cd.stride in (1, 2)) or (cd.k == 1 and cd.pad == 0 and cd.stride == 2)


def fwd_shape(cd):
    return (cd.hin, cd.win, rup(cd.cin, 8), cd.hout, cd.wout, rup(cd.cout, 32), cd.k, cd.stride, 0)


def shapes():
    """(H, W, CIN, Ho, Wo, COUTP, ks, stride, bwd) of every grid shape, forward shapes first."""
    out = []
    for bwd in (0, 1):
        for bp in (32, 16, 64):
            for cd in ms.conv_plan(config(bp))[1:]:
                if not eligible(cd):
                    continue
                s = fwd_shape(cd)
                if bwd:
                    if not (cd.k == 3 and cd.stride == 1 and cd.cin % 32 == 0):
                        continue
                    s = (cd.hout, cd.wout, rup(cd.cout, 32), cd.hin, cd.win, cd.cin, 3, 1, 1)
                if s not in out:
                    out.append(s)
    return out


def option_sets(bwd):
    base = dict(BWD_DEFAULTS if bwd else FWD_DEFAULTS)
    sets = [base]
    for name in OPTS:
        o = dict(base)
        o[name] = (0 if o[name] else 3 * NUM_CUS) if name == "persist_wgs" else 1 - o[name]
        sets.append(o)
    return sets


def grid():
    """Every problem of the grid as a row of FIELDS, in the golden's order."""
    rows = []
    for (H, W, CIN, Ho, Wo, COUTP, ks, stride, bwd) in shapes():
        for np_, mode, ds, B, o, tail in itertools.product((2, 3), range(4), (0, 1), BATCHES, option_sets(bwd), (0, 1)):
            rows.append((B, H, W, CIN, Ho, Wo, COUTP, ks, stride, np_, mode, tail, int(bwd and np_ == 2), ds,
                         o["force"], o["strip"], o["fine"], o["w8"], o["m16"], o["ksw"], o["persist_wgs"], o["rows"], NUM_CUS))
    return np.asarray(rows, dtype=np.int32)


def describe(problem):
    q = np.ascontiguousarray(problem, dtype=np.int32)
    buf = C.create_string_buffer(256)
    _lib.check(_lib.lib.pnvo_conv_x3_describe(q.ctypes.data_as(C.POINTER(C.c_int)), len(q), buf, len(buf)))
    return buf.value.decode()


def problem_of(**kw):
    """A problem row from named fields (forward defaults for the rest)."""
    f = dict(FWD_DEFAULTS, num_cus=NUM_CUS, np=2, mode=0, tail_scaled=0, absmax=0, ds=0)
    f.update(kw)
    return [f[k] for k in FIELDS]


def read_golden():
    parts, lines, index = {}, {}, []
    for raw in open(GOLDEN):
        head, _, rest = raw.rstrip("\n").partition(" ")
        if head == "P":
            n, _, text = rest.partition(" ")
            parts[int(n)] = text
        elif head == "=":
            n, *ids = map(int, rest.split())
            lines[n] = " | ".join(parts[i] for i in ids)
        elif head == "@":
            for run in rest.split():
                n, c = run.split(":")
                index += [int(n)] * int(c)
    return lines, index


def golden_line(lines, index, g, problem):
    """The golden's line for a problem of the grid (first match)."""
    hit = np.flatnonzero((g == np.asarray(problem, dtype=np.int32)).all(axis=1))
    assert hit.size, problem
    return lines[index[int(hit[0])]]


def test_every_grid_point_plans_as_before_the_refactor():
    lines, index = read_golden()
    g = grid()
    assert len(index) == len(g), (len(index), len(g))
    bad = []
    buf, fn, row = C.create_string_buffer(256), _lib.lib.pnvo_conv_x3_describe, g.strides[0]
    want = {n: l.encode() for n, l in lines.items()}
    for i in range(len(g)):
        rc = fn(C.cast(g.ctypes.data + i * row, C.POINTER(C.c_int)), g.shape[1], buf, 256)
        if rc != 0 or buf.value != want[index[i]]:
            bad.append((g[i].tolist(), rc, buf.value.decode(), lines[index[i]]))
    assert not bad, (len(bad), bad[:5])
    fams = {l.split()[0] for l in lines.values()}
    assert fams == {"none", "tile", "persistent", "rows"}, fams          # the grid reaches every family


def test_every_taken_plan_names_an_instance_of_the_table():
    """The planner looks its instance up in the table; the table's own listing (problem = nullptr, row index) names every instance."""
    table = set()
    buf = C.create_string_buffer(256)
    i = 0
    while _lib.lib.pnvo_conv_x3_describe(None, i, buf, len(buf)) == 0:
        table.add(buf.value.decode())
        i += 1
    assert len(table) == i == 160, (i, len(table))                       # 156 conv_x3_kernel + 4 conv_x3p_kernel instances, no duplicates
    lines, _ = read_golden()
    taken = {l.split(" | ")[0] for l in lines.values() if l.split()[0] in ("tile", "persistent")}
    assert taken and taken <= table, sorted(taken - table)
    for l in lines.values():                                             # block size of the line = the instance's thread count
        if l.split()[0] in ("tile", "persistent"):
            assert f"block {512 if ' w81 ' in l else 256} " in l, l


def test_describe_rejects_bad_arguments():
    buf = C.create_string_buffer(256)
    q = (C.c_int * len(FIELDS))(*problem_of(B=8, H=48, W=86, CIN=32, Ho=48, Wo=86, COUTP=32, ks=3, stride=1))
    assert _lib.lib.pnvo_conv_x3_describe(q, len(FIELDS) - 1, buf, len(buf)) == -1
    assert _lib.lib.pnvo_conv_x3_describe(q, len(FIELDS), None, 0) == -1
    assert _lib.lib.pnvo_conv_x3_describe(q, len(FIELDS), buf, len(buf)) == 0 and buf.value
