"""GPU (-m gpu): the float32-MFMA kernels compute what they computed before their launch was planned in one place, bit for bit — checksums
of the bits of outputs, hidden features, block outputs and two training steps' gradients against the pinned table
tests/golden/conv_fp32_bits.txt (tests/golden/gen_golden_conv_fp32_bits.py: cases, tensors, the file's format, the commit whose build
wrote it, and what the cases must cover).  The table is recomputed once, with the kernels' five knobs set as options of the handles in
this one process, and compared line by line; the coverage check runs on the plans of THIS build's launches, so a case that falls back to
another kernel family fails it instead of passing for less.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import gen_golden_conv_fp32_bits as gen  # noqa: E402

pytestmark = pytest.mark.gpu


def test_conv_fp32_bits_are_unchanged():
    with open(gen.PATH) as f:
        want = f.read().splitlines()
    assert os.path.getsize(gen.PATH) < 16 * 1024
    seen = []
    got = gen.table(torch.device("cuda:0"), seen)
    for k in sorted({l.split(" | ")[0] for l in seen}):
        print("launch:", k)
    gen.check_coverage(seen)
    assert len(got) == len(want), (len(got), len(want))
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    for g, w in bad:
        print(f"computed  {g}\npinned    {w}")
    assert not bad, f"{len(bad)} of {len(want)} tensors changed bits; first: {bad[0][0]} (pinned: {bad[0][1]})"


def test_two_handles_in_one_process_differ_in_fp32_form():
    """Nothing of the kernel selection is cached per process any more: two handles of one model, one on the workgroup-tile form of the
    LDS-staged convs and one on the wave-private form, run interleaved.  Each computes, to the bit, what a process of its own with that
    form in the environment computed on the commit the table was recorded from (the table's lines of the two form option sets), the
    planner names the two kernels for their launches, and both match the fp64 golden within the suite's 1e-4."""
    dev = torch.device("cuda:0")
    with open(gen.PATH) as f:
        pinned = dict(l.rsplit(" ", 3)[0:1] + [tuple(map(int, l.split()[2:]))] for l in f.read().splitlines())
    sets = gen.option_sets()
    models = {form: gen.golden_model(gen.GOLDENS[0][1], dev) for form in ("tile", "wave")}
    for form, (m, obs, ref) in models.items():
        m.set_option("conv", "fp32")
        m.set_option("fp32_form", form)
    for _ in range(2):                       # interleaved: a value cached by one handle's launch would show in the other's
        for form, (m, obs, ref) in models.items():
            o = dict(sets[0], form={"tile": 1, "wave": 2}[form])
            with torch.no_grad():
                out = m(obs)
            assert m.get_option("fp32_form") == form
            assert gen.checksum(out) == pinned[f"{gen.GOLDENS[0][0]}:fp32:o{sets.index(o)} output"], form
            fams = {l.split()[0] for l in gen.forward_launches(m, out.shape[0], o, False)}
            assert ("lds_tile" in fams and "lds_wave" not in fams) if form == "tile" else "lds_wave" in fams, (form, fams)
            got = out.double().cpu().numpy()
            err = np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-2)
            assert np.isfinite(got).all() and err.max() < 1e-4, (form, err)
    assert pinned[f"{gen.GOLDENS[0][0]}:fp32:o{sets.index(dict(sets[0], form=1))} output"] != \
        pinned[f"{gen.GOLDENS[0][0]}:fp32:o{sets.index(dict(sets[0], form=2))} output"]       # (the two forms do differ in bits)
