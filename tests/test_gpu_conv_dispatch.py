"""GPU (-m gpu): the host's conv dispatch against the pinned table tests/golden/conv_dispatch.txt — kernel family and executed FLOPs of
every residual-stage conv at every batch size 1 .. 256, for the benchmark model and a Bottleneck, a ResNeXt and an SE-ResNeXt model,
on the default options and with one option off its default at a time (tests/golden/gen_golden_conv_dispatch.py: models, option sets
and the file's format).  Read through pnvo_layer_kernel only: no forward runs.  The table was generated at the commit before the
dispatch was gathered into pnvo_conv_choice, so a refactor of it that moves one layer at one batch size under one option fails here.
"""
import os
import sys

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import gen_golden_conv_dispatch as gen  # noqa: E402

pytestmark = pytest.mark.gpu


def test_dispatch_table_is_unchanged():
    with open(gen.PATH) as f:
        want = f.read().splitlines()
    assert os.path.getsize(gen.PATH) < os.path.getsize(os.path.join(GOLDEN, "conv_x3_plans.txt"))
    got = gen.table(torch.device("cuda:0"))
    assert len(got) == len(want), (len(got), len(want))
    section = {}
    for k, (g, w) in enumerate(zip(got, want)):
        if w[:2] in ("M ", "O "):
            section[w[0]] = w
        assert g == w, f"line {k + 1} ({section.get('M')}, {section.get('O')}): the dispatch computes\n  {g}\nthe table pins\n  {w}"
