"""GPU (-m gpu): one training step's flat gradient and loss, bit for bit what they were before the weight gradients got one planner and
one instance table — checksums against the pinned table tests/golden/wgrad_bits.txt (tests/golden/gen_golden_wgrad_bits.py: cases,
the file's format, the commit whose build wrote it, and what the cases must cover).  The table is recomputed once and compared line by
line; the coverage check runs on what THIS build's planner says each request of each case ran on.
"""
import os
import sys

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import gen_golden_wgrad_bits as gen  # noqa: E402

pytestmark = pytest.mark.gpu


def test_wgrad_bits_are_unchanged():
    with open(gen.PATH) as f:
        want = f.read().splitlines()
    assert os.path.getsize(gen.PATH) < 16 * 1024
    seen = []
    got = gen.table(torch.device("cuda:0"), seen)
    for k in sorted({text.split(" | ")[0] for text, _ in seen}):
        print("request:", k)
    gen.check_coverage(seen)
    assert len(got) == len(want), (len(got), len(want))
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    for g, w in bad:
        print(f"computed  {g}\npinned    {w}")
    assert not bad, f"{len(bad)} of {len(want)} tensors changed bits; first: {bad[0][0]} (pinned: {bad[0][1]})"
