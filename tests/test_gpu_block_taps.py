"""GPU (-m gpu): block-output taps of a Bottleneck model.  The library answers `layer<stage>.<index>` from its block table
(csrc/pnvo_model.h: Block), so a Bottleneck block's tap has that block's real output geometry (four times the stage's planes)
and resnet101's two-digit block indices can be named.  Shapes against the fp64 oracle's taps; values within the activation
tolerance of test_every_intermediate_activation_matches_reference (2e-5 of the reference's largest magnitude)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import oracle
from pointnav_vo_amd import _lib
from test_gpu_parity import build

pytestmark = pytest.mark.gpu

# resnet101: [3, 4, 23, 3] Bottleneck blocks — the first and the last block of every stage, and a two-digit name inside stage 3
BLOCK_TAPS = ["layer1.0", "layer1.2", "layer2.0", "layer2.3", "layer3.0", "layer3.10", "layer3.22", "layer4.0", "layer4.2"]


def test_bottleneck_block_taps_match_the_oracle():
    rec = load_golden("model_deeper_64x48_b2.npz")
    assert str(rec["backbone"]) == "resnet101"
    model, cfg, sd, obs, tobs, _, _ = build(rec)
    taps = {}
    oracle.forward(sd, obs, ngroups=cfg.ngroups, dtype=np.float64, taps=taps)
    for name in BLOCK_TAPS:
        want = taps[name]
        with torch.no_grad():
            out, got = model.tap(name, tobs)
        got = got.cpu().numpy()
        assert got.shape == want.shape, (name, got.shape, want.shape)
        scale = np.abs(want).max() + 1e-6
        err = np.abs(got - want).max()
        print(f"{name}: shape {got.shape} max|got - ref| / max|ref| = {err / scale:.3e}")
        assert err / scale < 2e-5, (name, err, scale)
        assert np.isfinite(out.cpu().numpy()).all()


@pytest.mark.parametrize("name", ["layer5.0", "layer1.9"])
def test_unknown_block_tap_is_refused_by_name(name):
    rec = load_golden("model_deeper_64x48_b2.npz")
    model, cfg, sd, obs, tobs, _, _ = build(rec)
    with torch.no_grad(), pytest.raises(_lib.PnvoError, match=name.replace(".", r"\.")):
        model.tap(name, tobs)
