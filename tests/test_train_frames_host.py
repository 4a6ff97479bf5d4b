"""CPU: the host side of the training step's sensor-frame entry — the C ABI declares it, and the Python methods refuse a CPU model /
a CPU batcher and name the tensor whose shape is wrong, without touching a device."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from pointnav_vo_amd import _lib, synth
from pointnav_vo_amd import vo_cnn  # noqa: F401
from pointnav_vo_amd.dataset import StatePairBatcher
from pointnav_vo_amd.registry import baseline_registry
from pointnav_vo_amd.train import GeoInvarianceTrainStep, VOTrainStep

SPACE = ["rgb", "depth", "discretized_depth", "top_down_view"]
W, H = 45, 37


def cpu_step(name="vo_cnn_rgb_d_dd_top_down", space=SPACE, bins=10):
    """A VOTrainStep around a CPU model, as far as it gets without a device (the constructor itself refuses a CPU model)."""
    kw = dict(observation_space=space, observation_size=(W, H), hidden_size=512, backbone="resnet18", normalize_visual_inputs=True,
              output_dim=3, dropout_p=0.0)
    if bins:
        kw["discretized_depth_channels"] = bins
    st = object.__new__(VOTrainStep)
    st.model = baseline_registry.get_vo_model(name)(**kw)
    st.dev = torch.device("cpu")
    return st


def frame_tensors(B=2):
    return (torch.zeros((B, 2, H, W, 3), dtype=torch.uint8), torch.zeros((B, 2, H, W), dtype=torch.float32),
            torch.zeros((B, H, W, 2), dtype=torch.float32))


def test_header_declares_the_frame_entry_points():
    src = open(os.path.join(ROOT, "include", "pnvo.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for sym, nargs in (("pnvo_input_moments_raw", 11), ("pnvo_train_forward_raw", 11), ("pnvo_dataset_frames", 14)):
        m = re.search(r"\bint\s+" + sym + r"\s*\(([^)]*)\)\s*;", src)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, (sym, m.group(1))
        assert sym in _lib._SIGNATURES and len(_lib._SIGNATURES[sym][1]) == nargs
        assert getattr(_lib.lib, sym) is not None                     # ... and the library exports them


def test_forward_train_raw_refuses_a_cpu_model():
    st = cpu_step()
    rgb, dep, tdv = frame_tensors()
    for call in (lambda: st.forward_train_raw(rgb, dep, tdv), lambda: st.forward_backward_raw(rgb, dep, tdv, target=torch.zeros(2, 3)),
                 lambda: st.step_raw(rgb, dep, tdv, target=torch.zeros(2, 3))):
        with pytest.raises(RuntimeError, match="MI355X"):
            call()


def test_process_chunk_frames_refuses_a_cpu_batcher():
    with pytest.raises(RuntimeError, match="MI355X"):
        StatePairBatcher(W, H, device="cpu")
    b = object.__new__(StatePairBatcher)                               # (what the constructor would not build)
    b.W, b.H, b.dev, b.bins, b.edges, b.tdv, b.act_type, b.geo = W, H, torch.device("cpu"), 0, None, None, -1, ()
    ch = synth.make_dataset_chunk(2, H, W, seed=1)
    for kw in ({}, {"frames": True}):
        with pytest.raises(RuntimeError, match="MI355X"):
            b.process_chunk(ch, **kw)


@pytest.mark.parametrize("what,edit", [
    ("rgb_frames", lambda a: a.__setitem__(0, torch.zeros((2, 2, H, W, 4), dtype=torch.uint8))),          # a channel too many
    ("rgb_frames", lambda a: a.__setitem__(0, torch.zeros((2, 2, H, W, 3), dtype=torch.float32))),        # pair-style floats
    ("rgb_frames", lambda a: a.__setitem__(0, None)),                                                      # the model has rgb
    ("depth_frames", lambda a: a.__setitem__(1, torch.zeros((2, H, W, 2), dtype=torch.float32))),         # the pair layout
    ("depth_frames", lambda a: a.__setitem__(1, torch.zeros((2, 2, H, W, 1), dtype=torch.float32))),
    ("top_down_view", lambda a: a.__setitem__(2, torch.zeros((3, H, W, 2), dtype=torch.float32))),        # another batch size
    ("top_down_view", lambda a: a.__setitem__(2, None)),
    ("edges", lambda a: a.__setitem__(3, [0.0, 0.5, 1.0])),                                                # not bins + 1 of them
])
def test_frame_argument_errors_name_the_offending_tensor(what, edit):
    st = cpu_step()
    args = list(frame_tensors()) + [None]
    edit(args)
    with pytest.raises(ValueError, match=what):
        st._frame_ptrs(*args)


def test_frame_arguments_of_a_model_without_rgb_and_top_down_view():
    st = cpu_step("vo_cnn_d_dd_top_down", ["depth", "discretized_depth", "top_down_view"])
    rgb, dep, tdv = frame_tensors()
    edges = [float(np.float16(i / 10)) for i in range(10)] + [1.0]
    ptrs, keep, B = st._frame_ptrs(rgb, dep, tdv, edges)               # rgb frames handed to a model without rgb are not passed on
    assert B == 2 and ptrs[0] is None and ptrs[1] is not None and ptrs[2] is not None and len(keep) == 2
    assert list(ptrs[3]) == [float(np.float32(e)) for e in edges]


def test_geo_step_keeps_the_edges_for_frame_batches():
    js = GeoInvarianceTrainStep({2: cpu_step()}, edges=[0.0, 1.0])
    assert js.edges == [0.0, 1.0] and GeoInvarianceTrainStep({2: cpu_step()}).edges is None
