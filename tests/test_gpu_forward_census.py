"""GPU (-m gpu): the walk of the inference forwards against the pinned table tests/golden/forward_census.txt — the ordered timing table
(entry names with their launch counts, and the flops sum) of one forward per model, option set and batch size, for a BasicBlock, a
Bottleneck and an SE-ResNeXt VO model on float32 and a dual bfloat16 forward (tests/golden/gen_golden_forward_census.py: models, option
sets, batch sizes, the file's format and what it must cover).  The table was generated at the commit before the two forwards were split
into steps with one block walk, so a change of the host code that adds, drops, renames or reorders one launch of one forward fails here.
"""
import os
import sys

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import gen_golden_forward_census as gen  # noqa: E402

pytestmark = pytest.mark.gpu


def test_forward_census_is_unchanged():
    with open(gen.PATH) as f:
        want = f.read().splitlines()
    assert os.path.getsize(gen.PATH) < os.path.getsize(os.path.join(GOLDEN, "conv_x3_plans.txt")) // 2
    gen.check_coverage(want)
    got = gen.table(torch.device("cuda:0"))
    assert len(got) == len(want), (len(got), len(want))
    section = {}
    for k, (g, w) in enumerate(zip(got, want)):
        if w[:2] in ("M ", "O "):
            section[w[0]] = w
        assert g == w, f"line {k + 1} ({section.get('M')}, {section.get('O')}): the forward runs\n  {g}\nthe table pins\n  {w}"
