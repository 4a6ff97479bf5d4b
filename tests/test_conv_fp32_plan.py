"""CPU: the planner of the float32-MFMA convs and Linear layers (problem -> plan -> instance table, pointnav-vo_amd/csrc/conv_mfma.hip with
conv3_lds.hip's kernels) over a grid of problems, through the host-only entry pnvo_conv_fp32_describe, against
tests/golden/conv_fp32_plans.txt.xz.

The golden was recorded from the launch code of the commit BEFORE the refactor (tests/golden/gen_golden_conv_fp32_plans.py names it and
says how), so it pins kernel family, template instance, grid, block size, LDS bytes, both splits, the scratch size, the reduce launch,
the statistics slots and the rows per wave tile of every grid point to what the project launched before.

Grid (in this order, the last axis fastest):
    shape    forward convs — every conv behind the stem of the resnet18 model with baseplanes 32, 16 and 64 and the 1x1 convs of resnet50,
             at 341 x 192, 200 x 113 and 45 x 37 (statistics wanted, padded output); the stems as the generic kernel takes them (observation
             tensors); the hidden layer (a valid conv whose taps are the feature map: Linear epilogue, split-K scratch available, a
             three-unit head offered) and the output head; the backward-data problems of the resnet18 convs — the full form (the
             forward's stride as upsampling) and, for the 3x3 stride-2 convs, the four parity phases (1- and 2-tap kernels, strided
             output) —, each overwriting and accumulating; the two transposed Linears.  Duplicates dropped.
    mode     0 (plain operand) and 1 (producer GroupNorm + ReLU) for forward convs and the Linear layers; the stems 2 only; backward 0 only
    B        BATCHES (those of test_conv_x3_plan.py)
    lds_ok   0, 1
    options  the defaults, then each float32-MFMA setting of test_gpu_knobs.KNOBS

File format (that of wgrad_plans.txt.xz): `P n <text>` defines part n; `= n a b c` defines distinct line n as parts a, b, c joined by
" | " (family and instance | grid, block, LDS bytes, wave split, K split, scratch floats, reduce launch | tiles, groups, items, LDS table
floats, slots, rows per wave tile); `@ n:c n:c ...` appends runs (c consecutive grid points map to line n).
"""
import ctypes as C
import itertools
import lzma
import os
import re

import numpy as np

from conftest import ROOT
from pointnav_vo_amd import _lib, model_spec as ms
from test_conv_x3_plan import BATCHES, SPACE, rup
from test_gpu_knobs import KNOBS

GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_fp32_plans.txt.xz")
SIZES = [(341, 192), (200, 113), (45, 37)]
NUM_CUS = 256
# field order of pnvo_conv_fp32_describe's problem array (include/pnvo.h)
FIELDS = ("B", "H", "W", "CIN", "Ho", "Wo", "COUT", "COUTP", "KH", "KW", "stride", "pad", "up", "y_cstride", "mode", "accum",
          "y_sh", "y_sw", "y_oh", "y_ow", "y_H", "y_W", "linear", "stats", "ksplit_ok", "head", "lds_ok",
          "tile", "wsplit", "form", "wave_wgs", "wave_nt", "num_cus")
OPT_DEFAULTS = dict(tile=0, wsplit=-1, form=0, wave_wgs=3, wave_nt=1)
# the environment seeds of the five options (csrc/pnvo_api.hip kOptions) and how their words read
ENV = {"PNVO_CONV_TILE": ("tile", int), "PNVO_CONV_WSPLIT": ("wsplit", int), "PNVO_CONV3": ("form", {"tile": 1, "wave": 2}.__getitem__),
       "PNVO_WAVE_WGS": ("wave_wgs", int), "PNVO_WAVE_NT": ("wave_nt", int)}
# Rows of the instance table that no problem of the grid reaches, by name, with the reason (checked on the commit the golden was
# recorded from).
_G = "generic mt{} nt{} mode{} jc{} feat{}".format
UNREACHED = {
    # wave tiles of four and of two pixel tiles by one N-tile: only option fp32_tile selects them, and the knob tests set 12 and 22 alone
    **{_G(mt, 1, mode, jc, 0): "fp32_tile is only ever 12 or 22" for mt, jcs in ((4, (1,)), (2, (4, 1))) for mode in (0, 1) for jc in jcs},
    _G(4, 1, 2, 1, 0): "fp32_tile is only ever 12 or 22", _G(2, 1, 2, 1, 0): "fp32_tile is only ever 12 or 22",
    # 8-channel stages (an input that is no 32-channel multiple) under a wave of several tiles: the grid's narrow inputs are the 16-channel
    # tensors of the 16-base-plane models, whose convs have one N-tile, and the 8 gradient channels of the transposed head, 16 N-tiles over
    # few rows, which choose_tile spreads one per wave
    **{_G(mt, nt, mode, 1, 0): "narrow inputs only feed one-N-tile waves" for mt, nt in ((2, 2), (1, 2), (1, 4)) for mode in (0, 1)},
    **{_G(1, 2, mode, 1, 1): "narrow inputs only feed one-N-tile waves" for mode in (0, 1)},
    # a parity phase reads an output gradient, channel-padded to 32: always 32-channel stages
    **{_G(1, nt, 0, 1, 2): "backward-data inputs are 32-channel multiples" for nt in (1, 2, 4)},
    _G(1, 4, 2, 1, 0): "a stem has 32 or 64 output channels: at most two N-tiles",
    # the 12 x 8 workgroup tile with one N-tile per wave: the one-N-tile layers of the grid (32 output channels) have 48 x 86, 24 x 43,
    # 29 x 50, 15 x 25, 10 x 12 and 5 x 6 maps, none of which pads least on it
    "lds_tile blk0 wy3 wx1 nt1 mode0": "no 32-channel map of the grid pads least on 12 x 8 tiles",
    "lds_tile blk0 wy3 wx1 nt1 mode1": "no 32-channel map of the grid pads least on 12 x 8 tiles",
}
TABLE_ROWS = 64


def option_sets():
    """The defaults, then the float32-MFMA settings of every knob-test environment that has one (in KNOBS' order, duplicates dropped)."""
    sets = [dict(OPT_DEFAULTS)]
    for env in KNOBS:
        o = dict(OPT_DEFAULTS)
        for name, word in env.items():
            if name in ENV:
                o[ENV[name][0]] = ENV[name][1](word)
        if o not in sets:
            sets.append(o)
    return sets


def config(backbone, baseplanes, size):
    return ms.config_from_kwargs(observation_space=SPACE, observation_size=size, hidden_size=512, backbone=backbone,
                                 resnet_baseplanes=baseplanes, normalize_visual_inputs=True, output_dim=3,
                                 discretized_depth_channels=10)


def shape_of(**kw):
    """One grid shape: the problem fields a launch site states, the rest off; `modes` = the operand modes it is asked with."""
    f = dict(pad=0, stride=1, up=1, accum=0, y_sh=0, y_sw=0, y_oh=0, y_ow=0, y_H=0, y_W=0, linear=0, stats=0, ksplit_ok=0, head=0, modes=(0,))
    f.update(kw)
    f.setdefault("COUTP", rup(f["COUT"], 32))
    f.setdefault("y_cstride", f["COUTP"])
    return f


def shapes():
    out = []

    def add(**kw):
        s = shape_of(**kw)
        if s["Ho"] > 0 and s["Wo"] > 0 and s not in out:        # (a parity phase of a one-row map is empty: nothing is launched)
            out.append(s)

    cfgs18 = [config("resnet18", bp, size) for bp in (32, 16, 64) for size in SIZES]
    cfgs50 = [config("resnet50", 32, size) for size in SIZES]
    # forward convs (csrc/pnvo_api.hip conv_choice / run_conv_fp32): statistics wanted, channel-padded output
    for cfg in cfgs18 + cfgs50:
        for cd in ms.conv_plan(cfg)[1:]:
            if cfg in cfgs50 and cd.k != 1:
                continue
            add(H=cd.hin, W=cd.win, CIN=rup(cd.cin, 8), Ho=cd.hout, Wo=cd.wout, COUT=cd.cout, KH=cd.k, KW=cd.k, stride=cd.stride, pad=cd.pad,
                stats=1, modes=(0, 1))
    # the stem on the generic kernel: operand gathered from the observation tensors
    for cfg in cfgs18:
        cd = ms.conv_plan(cfg)[0]
        add(H=cd.hin, W=cd.win, CIN=rup(cd.cin, 8), Ho=cd.hout, Wo=cd.wout, COUT=cd.cout, KH=cd.k, KW=cd.k, stride=cd.stride, pad=cd.pad,
            stats=1, modes=(2,))
    # hidden layer and output head (pnvo_api.hip: the Linear layers): bias / ReLU, exact output stride, split-K scratch
    for cfg in cfgs18:
        fh, fw = cfg.final_hw
        add(H=fh, W=fw, CIN=rup(cfg.comp_channels, 32), Ho=1, Wo=1, COUT=cfg.hidden, KH=fh, KW=fw, y_cstride=cfg.hidden, linear=1, ksplit_ok=1,
            head=cfg.out_dim, modes=(0, 1))
        add(H=1, W=1, CIN=cfg.hidden, Ho=1, Wo=1, COUT=cfg.out_dim, KH=1, KW=1, y_cstride=cfg.out_dim, linear=1, ksplit_ok=1, modes=(0, 1))
    # backward-data (csrc/pnvo_train_api.hip dgrad_problem): input and output swapped, exact output stride
    for cfg in cfgs18:
        for cd in ms.conv_plan(cfg)[1:]:
            for accum in (0, 1):
                add(H=cd.hout, W=cd.wout, CIN=rup(cd.cout, 32), Ho=cd.hin, Wo=cd.win, COUT=cd.cin, KH=cd.k, KW=cd.k, pad=cd.k - 1 - cd.pad,
                    up=cd.stride, y_cstride=cd.cin, accum=accum)
                if cd.k == 3 and cd.stride == 2:
                    for ph, pw in itertools.product((0, 1), (0, 1)):
                        add(H=cd.hout, W=cd.wout, CIN=rup(cd.cout, 32), Ho=(cd.hin - ph + 1) // 2, Wo=(cd.win - pw + 1) // 2, COUT=cd.cin,
                            KH=2 if ph else 1, KW=2 if pw else 1, y_cstride=cd.cin, accum=accum, y_sh=2, y_sw=2, y_oh=ph, y_ow=pw, y_H=cd.hin,
                            y_W=cd.win)
    # the transposed Linears of the backward (linear_t_problem): head (8 gradient channels -> hidden), hidden layer (hidden -> feature map)
    for cfg in cfgs18:
        fh, fw = cfg.final_hw
        add(H=1, W=1, CIN=8, Ho=1, Wo=1, COUT=cfg.hidden, KH=1, KW=1, y_cstride=cfg.hidden)
        n = fh * fw * rup(cfg.comp_channels, 32)
        add(H=1, W=1, CIN=cfg.hidden, Ho=1, Wo=1, COUT=n, KH=1, KW=1, y_cstride=n)
    return out


def grid():
    """Every problem of the grid as a row of FIELDS, in the golden's order."""
    rows, opts = [], option_sets()
    for s in shapes():
        for mode, B, lds_ok, o in itertools.product(s["modes"], BATCHES, (0, 1), opts):
            f = dict(s, mode=mode, B=B, lds_ok=lds_ok, num_cus=NUM_CUS, **o)
            rows.append([f[k] for k in FIELDS])
    return np.asarray(rows, dtype=np.int32)


def describe(problem):
    q = np.ascontiguousarray(problem, dtype=np.int32)
    buf = C.create_string_buffer(512)
    _lib.check(_lib.lib.pnvo_conv_fp32_describe(q.ctypes.data_as(C.POINTER(C.c_int)), len(q), buf, len(buf)))
    return buf.value.decode()


def problem_of(**kw):
    """A problem row from named fields (a 3x3 stride-1 forward conv's defaults for the rest)."""
    f = dict(dict(mode=0, lds_ok=1, num_cus=NUM_CUS, **OPT_DEFAULTS), **shape_of(**dict(dict(KH=3, KW=3, pad=1, stats=1), **kw)))
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
    while _lib.lib.pnvo_conv_fp32_describe(None, len(rows), buf, len(buf)) == 0:
        rows.append(buf.value.decode())
    return rows


def describe_all(g):
    buf, fn, row = C.create_string_buffer(512), _lib.lib.pnvo_conv_fp32_describe, g.strides[0]
    out = []
    for i in range(len(g)):
        rc = fn(C.cast(g.ctypes.data + i * row, C.POINTER(C.c_int)), g.shape[1], buf, 512)
        out.append(buf.value if rc == 0 else b"error %d" % rc)
    return out


def test_every_grid_point_plans_as_before_the_refactor():
    lines, index = read_golden()
    g = grid()
    assert len(index) == len(g), (len(index), len(g))
    want = {n: l.encode() for n, l in lines.items()}
    got = describe_all(g)
    bad = [(g[i].tolist(), got[i].decode(), lines[index[i]]) for i in range(len(g)) if got[i] != want[index[i]]]
    assert not bad, (len(bad), bad[:5])
    fams = {l.split()[0] for l in lines.values()}
    assert fams == {"generic", "lds_tile", "lds_wave", "none"}, fams    # the grid reaches every family, and requests no kernel serves


def test_the_grid_reaches_every_row_of_the_instance_table():
    """The table's own listing (problem = nullptr, row index) names every instance; a row that no grid point reaches is named in
    UNREACHED with the reason, not silently absent."""
    rows = table()
    assert len(rows) == len(set(rows)) == TABLE_ROWS, rows
    lines, _ = read_golden()
    taken = {l.split(" | ")[0] for l in lines.values()} - {"none"}
    assert taken <= set(rows), sorted(taken - set(rows))
    assert set(rows) - taken == set(UNREACHED), (sorted(set(rows) - taken - set(UNREACHED)), sorted(set(UNREACHED) - (set(rows) - taken)))
    blocks = {"generic": {256}, "lds_tile": {192, 256}, "lds_wave": {256}}   # the launch bounds of the three kernels
    for l in lines.values():
        if l != "none":
            assert int(l.split(" block ")[1].split()[0]) in blocks[l.split()[0]], l


def test_family_tile_and_slots_do_not_depend_on_the_operand_mode():
    """The schedule asks per layer with the plain operand and launches with the real one: kernel family, the instance's wave tile and the
    statistics slots (with the rows per wave tile the GroupNorm finalisation is given) must be the same for both."""
    g = grid()
    got = describe_all(g)
    mode_at = FIELDS.index("mode")

    def tile_of(line):
        if line == "none":
            return None
        head, geo = line.split(" | ")[0], line.rsplit(" | ", 1)[1]
        w = dict(re.match(r"([a-z]+)(\d+)$", t).groups() for t in head.split()[1:])
        return (head.split()[0], w.get("mt"), w.get("nt"), w.get("blk"), w.get("wy"), w.get("wx"), geo.split(" slots ")[1])

    by_rest, n_pairs = {}, 0
    for i in range(len(g)):
        row = g[i].tolist()
        mode = row[mode_at]
        row[mode_at] = -1
        by_rest.setdefault(tuple(row), {})[mode] = got[i].decode()
    for rest, per_mode in by_rest.items():
        if len(per_mode) > 1:
            n_pairs += 1
            assert len({tile_of(l) for l in per_mode.values()}) == 1, (rest, per_mode)
    assert n_pairs > 1000, n_pairs


def test_options_steer_what_they_name():
    conv = dict(B=8, H=48, W=86, CIN=64, Ho=48, Wo=86, COUT=64)
    fam = lambda **kw: describe(problem_of(**dict(conv, **kw))).split(" | ")[0]
    # fp32_form: which LDS-staged kernel; auto = the wave kernel from 64 input channels on
    assert fam().startswith("lds_wave ") and fam(form=2) == fam() and fam(form=1).startswith("lds_tile ")
    assert fam(CIN=32, COUT=32).startswith("lds_tile ") and fam(CIN=32, COUT=32, form=2).startswith("lds_wave ")
    assert fam(lds_ok=0).startswith("generic ") and fam(lds_ok=0, form=2) == fam(lds_ok=0)
    # wave_nt / wave_wgs: N-tiles per wave item, workgroups per CU of the persistent grid
    assert " nt1 " in fam() and " nt2 " in fam(wave_nt=2)
    big = dict(conv, B=256)
    grid_x = lambda **kw: int(describe(problem_of(**dict(big, **kw))).split(" grid ")[1].split("x")[0])
    assert grid_x() == 3 * NUM_CUS and grid_x(wave_wgs=4) == 4 * NUM_CUS and grid_x(wave_wgs=1) == NUM_CUS
    assert grid_x(form=1) == grid_x(form=1, wave_wgs=1)                         # (the tile kernel sizes its own grid)
    # fp32_wsplit: forced on / off wherever the split is possible (a long enough reduction, one pixel tile, <= 2 N-tiles) ...
    deep = dict(B=8, H=6, W=11, CIN=256, Ho=6, Wo=11, COUT=256, lds_ok=0)
    ws = lambda **kw: describe(problem_of(**dict(deep, **kw))).split(" wsplit ")[1].split()[0]
    assert ws(wsplit=1) == "1" and ws(wsplit=0) == "0" and ws() in ("0", "1")
    assert " feat1 " in describe(problem_of(**dict(deep, wsplit=1))) + " "
    # ... and nowhere else: a 1x1 conv over 32 channels has 4 stages
    assert describe(problem_of(**dict(deep, CIN=32, KH=1, KW=1, pad=0, wsplit=1))).split(" wsplit ")[1].split()[0] == "0"
    # fp32_tile: the forced wave tile from 8192 output pixels on, ignored below
    small, large = dict(conv, lds_ok=0, B=1), dict(conv, lds_ok=0, B=2)        # 4128 and 8256 output pixels
    for tile, key in ((12, "generic mt1 nt2 "), (22, "generic mt2 nt2 "), (21, "generic mt2 nt1 "), (41, "generic mt4 nt1 ")):
        assert describe(problem_of(**dict(large, tile=tile))).startswith(key), tile
        assert describe(problem_of(**dict(small, tile=tile))) == describe(problem_of(**small)), tile
    assert describe(problem_of(**dict(large, tile=14))) == describe(problem_of(**large))       # 4 does not divide the layer's 2 N-tiles
    assert describe(problem_of(**dict(large, COUT=96, tile=33))) == "none"                       # no such instance: refused when planning


def test_unserved_requests_plan_as_none():
    """What the kernels have no instance for is refused by the planner, on the host, not met as a launch error."""
    phase = dict(B=64, H=24, W=43, CIN=64, Ho=24, Wo=43, COUT=32, KH=2, KW=2, pad=0, stats=0, y_cstride=32, y_sh=2, y_sw=2, y_oh=1, y_ow=1,
                 y_H=48, y_W=86, lds_ok=0)
    assert describe(problem_of(**phase)).startswith("generic mt1 nt1 mode0 jc4 feat2 ")
    assert describe(problem_of(**dict(phase, mode=1))) == "none"                 # strided output with a producer affine
    assert describe(problem_of(**dict(phase, COUT=64, y_cstride=64, tile=22))) == "none"   # ... or on a two-pixel-tile wave
    assert describe(problem_of(B=8, H=48, W=86, CIN=64, Ho=48, Wo=86, COUT=64, mode=2)) == "none"   # LDS stagers read no observation tensors


def test_describe_rejects_bad_arguments():
    buf = C.create_string_buffer(512)
    ok = dict(B=8, H=48, W=86, CIN=32, Ho=48, Wo=86, COUT=32)
    q = (C.c_int * len(FIELDS))(*problem_of(**ok))
    fn = _lib.lib.pnvo_conv_fp32_describe
    assert fn(q, len(FIELDS) - 1, buf, len(buf)) == -1
    assert fn(q, len(FIELDS), None, 0) == -1
    assert fn(None, TABLE_ROWS, buf, len(buf)) == -1
    assert fn(None, -1, buf, len(buf)) == -1
    assert fn(q, len(FIELDS), buf, len(buf)) == 0 and buf.value
    for field, value in (("mode", 3), ("mode", -1), ("B", 0), ("KH", 0), ("up", 3), ("wsplit", 2), ("form", 3), ("num_cus", 0), ("y_cstride", 0), ("pad", -1)):
        bad = (C.c_int * len(FIELDS))(*problem_of(**dict(ok, **{field: value})))
        assert fn(bad, len(FIELDS), buf, len(buf)) == -1, field
