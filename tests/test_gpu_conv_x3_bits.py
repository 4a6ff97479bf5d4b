"""GPU (-m gpu): the conv_x3 kernels compute what they computed before their global-memory accesses moved onto buffer descriptors, bit
for bit — checksums of the bits of outputs, hidden features, block outputs, pooled activations and one training step's gradient against
the pinned table tests/golden/conv_x3_bits.txt (tests/golden/gen_golden_conv_x3_bits.py: cases, tensors, the file's format, the commit
whose build wrote it, and what the cases must cover).  The table is recomputed once and compared line by line; the coverage check
runs on the launches of THIS build's forwards, so a case that falls back to another kernel family fails it instead of passing for less.
"""
import os
import sys

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import gen_golden_conv_x3_bits as gen  # noqa: E402

pytestmark = pytest.mark.gpu


def test_conv_x3_bits_are_unchanged():
    with open(gen.PATH) as f:
        want = f.read().splitlines()
    assert os.path.getsize(gen.PATH) < 16 * 1024
    seen = []
    got = gen.table(torch.device("cuda:0"), seen)
    for k in sorted(set(seen)):
        print("launch:", k)
    gen.check_coverage(seen)
    assert len(got) == len(want), (len(got), len(want))
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    for g, w in bad:
        print(f"computed  {g}\npinned    {w}")
    assert not bad, f"{len(bad)} of {len(want)} tensors changed bits; first: {bad[0][0]} (pinned: {bad[0][1]})"
