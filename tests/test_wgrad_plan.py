"""CPU: the weight-gradient planner (problem -> plan -> instance table, pointnav-vo_amd/csrc/train_kernels.hip and wgrad_x3.hip) over a
grid of problems, through the host-only entry pnvo_wgrad_describe, against tests/golden/wgrad_plans.txt.xz.

The golden was recorded from the planner of the commit BEFORE the refactor (tests/golden/gen_golden_wgrad_plans.py names it and says
how), so it pins kernel family, template instance, grid, block size, LDS bytes, scratch size, the reduce launch and every geometry
field of every grid point to what the project launched before.

Grid (in this order, the last axis fastest):
    shape   every conv of the resnet18 model with baseplanes 32, 16 and 64 at 341 x 192, 200 x 113 and 45 x 37 — the stem as the
            training step asks it (observation tensors, 32 input channels), the hidden layer (a valid conv whose taps are the feature
            map, over the channel-padded compression map) and the output head (1x1, 8 gradient channels) — duplicates dropped
    mode    0 (plain input) and 1 (producer GroupNorm + ReLU recomputed); the stem: 2 only
    B       BATCHES (those of test_conv_x3_plan.py)
    wgrad3  x3, fp32
    wgrad   auto, lds9, generic
    np      3 (bf16 pieces only), 2 (the caller permits the float16 form)

File format (that of conv_x3_plans.txt, xz-compressed: the batch axis moves the geometry of nearly every line, 8 124 distinct ones, and
the plain text would be close to a megabyte): `P n <text>` defines part n; `= n a b c` defines distinct line n as parts a, b, c joined by
" | " (family and instance | grid, block, LDS bytes, scratch floats, reduce grid | geometry); `@ n:c n:c ...` appends runs (c
consecutive grid points map to line n).
"""
import ctypes as C
import itertools
import lzma
import os

import numpy as np

from conftest import ROOT
from pointnav_vo_amd import _lib, model_spec as ms
from test_conv_x3_plan import BATCHES, SPACE, rup

GOLDEN = os.path.join(ROOT, "tests", "golden", "wgrad_plans.txt.xz")
SIZES = [(341, 192), (200, 113), (45, 37)]
WGRAD3 = {"x3": 1, "fp32": 0}
WGRAD = {"auto": 0, "lds9": 1, "generic": 2}
# field order of pnvo_wgrad_describe's problem array (include/pnvo.h)
FIELDS = ("B", "H", "W", "CIN", "Ho", "Wo", "COUT", "DYC", "KH", "KW", "stride", "pad", "mode", "np", "wgrad3", "wgrad")
# Rows of the instance table that no problem of the grid reaches, by name, with the reason (checked on the commit the golden was
# recorded from): the generic kernel's observation-tensor fetch (mode 2) is instantiated for every tap group, but the only layer that
# reads observation tensors is the 7x7 stem, whose 49 taps go in groups of 7.
UNREACHED = {"generic tg9 mode2", "generic tg6 mode2", "generic tg3 mode2", "generic tg1 mode2"}
TABLE_ROWS = 28


def config(baseplanes, size):
    return ms.config_from_kwargs(observation_space=SPACE, observation_size=size, hidden_size=512, backbone="resnet18",
                                 resnet_baseplanes=baseplanes, normalize_visual_inputs=True, output_dim=3,
                                 discretized_depth_channels=10)


def layer_shapes(cfg):
    """(H, W, CIN, Ho, Wo, COUT, DYC, KH, KW, stride, pad, stem) of every weight-gradient request of one backward, in backward order
    reversed: stem, residual convs, compression conv, hidden layer, head (csrc/pnvo_train_api.hip: wgrad_request)."""
    plan = ms.conv_plan(cfg)
    out = []
    for k, cd in enumerate(plan):
        out.append((cd.hin, cd.win, 32 if k == 0 else cd.cin, cd.hout, cd.wout, cd.cout, rup(cd.cout, 32), cd.k, cd.k, cd.stride, cd.pad, k == 0))
    fh, fw = cfg.final_hw
    out.append((fh, fw, rup(cfg.comp_channels, 32), 1, 1, cfg.hidden, cfg.hidden, fh, fw, 1, 0, False))
    out.append((1, 1, cfg.hidden, 1, 1, cfg.out_dim, 8, 1, 1, 1, 0, False))
    return out


def shapes():
    out = []
    for bp in (32, 16, 64):
        for size in SIZES:
            for s in layer_shapes(config(bp, size)):
                if s not in out:
                    out.append(s)
    return out


def grid():
    """Every problem of the grid as a row of FIELDS, in the golden's order."""
    rows = []
    for s in shapes():
        for mode, B, w3, wg, np_ in itertools.product((2,) if s[-1] else (0, 1), BATCHES, (1, 0), (0, 1, 2), (3, 2)):
            rows.append((B,) + s[:-1] + (mode, np_, w3, wg))
    return np.asarray(rows, dtype=np.int32)


def describe(problem):
    q = np.ascontiguousarray(problem, dtype=np.int32)
    buf = C.create_string_buffer(512)
    _lib.check(_lib.lib.pnvo_wgrad_describe(q.ctypes.data_as(C.POINTER(C.c_int)), len(q), buf, len(buf)))
    return buf.value.decode()


def problem_of(**kw):
    """A problem row from named fields (a 3x3 stride-1 conv's defaults for the rest)."""
    f = dict(KH=3, KW=3, stride=1, pad=1, mode=0, np=3, wgrad3=1, wgrad=0)
    f.update(kw)
    f.setdefault("DYC", rup(f["COUT"], 32))
    return [f[k] for k in FIELDS]


def read_golden():
    parts, lines, index = {}, {}, []
    for raw in lzma.open(GOLDEN, "rt"):
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


def table():
    rows, buf = [], C.create_string_buffer(512)
    while _lib.lib.pnvo_wgrad_describe(None, len(rows), buf, len(buf)) == 0:
        rows.append(buf.value.decode())
    return rows


def test_every_grid_point_plans_as_before_the_refactor():
    lines, index = read_golden()
    g = grid()
    assert len(index) == len(g), (len(index), len(g))
    bad = []
    buf, fn, row = C.create_string_buffer(512), _lib.lib.pnvo_wgrad_describe, g.strides[0]
    want = {n: l.encode() for n, l in lines.items()}
    for i in range(len(g)):
        rc = fn(C.cast(g.ctypes.data + i * row, C.POINTER(C.c_int)), g.shape[1], buf, 512)
        if rc != 0 or buf.value != want[index[i]]:
            bad.append((g[i].tolist(), rc, buf.value.decode(), lines[index[i]]))
    assert not bad, (len(bad), bad[:5])
    fams = {l.split()[0] for l in lines.values()}
    assert fams == {"generic", "lds9", "mw12", "stem_lds", "x3"}, fams    # the grid reaches every family


def test_the_grid_reaches_every_row_of_the_instance_table():
    """The table's own listing (problem = nullptr, row index) names every instance; a row that no grid point reaches is named in
    UNREACHED with the reason, not silently absent."""
    rows = table()
    assert len(rows) == len(set(rows)) == TABLE_ROWS, rows
    lines, _ = read_golden()
    taken = {l.split(" | ")[0] for l in lines.values()}
    assert taken <= set(rows), sorted(taken - set(rows))
    assert set(rows) - taken == UNREACHED, (sorted(set(rows) - taken), sorted(UNREACHED))
    blocks = {"generic": 256, "lds9": 576, "mw12": 768, "stem_lds": 448, "x3": 256}   # the launch bounds of the five kernels
    for l in lines.values():
        assert f" block {blocks[l.split()[0]]} " in l, l


def test_options_steer_the_choice():
    """wgrad=lds9 matters only where wgrad3 already keeps the matrix-core family out; wgrad=generic skips every LDS family, the float32
    stem kernel included; the float16 form is granted to the matrix-core family alone."""
    conv = dict(B=8, H=48, W=86, CIN=64, Ho=48, Wo=86, COUT=64)
    fam = lambda **kw: describe(problem_of(**dict(conv, **kw))).split()[0]
    assert fam() == "x3" and fam(wgrad=1) == "x3" and fam(wgrad=2) == "x3"
    assert fam(wgrad3=0) == "mw12" and fam(wgrad3=0, wgrad=1) == "lds9" and fam(wgrad3=0, wgrad=2) == "generic"
    assert describe(problem_of(**dict(conv, np=2))).startswith("x3 mode0 np2 ") and describe(problem_of(**conv)).startswith("x3 mode0 np3 ")
    assert describe(problem_of(**dict(conv, np=2, wgrad3=0))).endswith(" np 0")
    stem = dict(B=8, H=192, W=341, CIN=32, Ho=96, Wo=171, COUT=32, KH=7, KW=7, stride=2, pad=3, mode=2)
    assert describe(problem_of(**stem)).startswith("stem_lds ")
    assert describe(problem_of(**dict(stem, wgrad=1))).startswith("stem_lds ")
    assert describe(problem_of(**dict(stem, wgrad=2))).startswith("generic tg7 mode2 ")


def test_describe_rejects_bad_arguments():
    buf = C.create_string_buffer(512)
    q = (C.c_int * len(FIELDS))(*problem_of(B=8, H=48, W=86, CIN=32, Ho=48, Wo=86, COUT=32))
    assert _lib.lib.pnvo_wgrad_describe(q, len(FIELDS) - 1, buf, len(buf)) == -1
    assert _lib.lib.pnvo_wgrad_describe(q, len(FIELDS), None, 0) == -1
    assert _lib.lib.pnvo_wgrad_describe(None, TABLE_ROWS, buf, len(buf)) == -1
    assert _lib.lib.pnvo_wgrad_describe(None, -1, buf, len(buf)) == -1
    assert _lib.lib.pnvo_wgrad_describe(q, len(FIELDS), buf, len(buf)) == 0 and buf.value
    for field, value in (("mode", 3), ("np", 4), ("wgrad", 3), ("wgrad3", 2), ("B", 0), ("KH", 0)):
        bad = (C.c_int * len(FIELDS))(*problem_of(**dict(dict(B=8, H=48, W=86, CIN=32, Ho=48, Wo=86, COUT=32), **{field: value})))
        assert _lib.lib.pnvo_wgrad_describe(bad, len(FIELDS), buf, len(buf)) == -1, field
