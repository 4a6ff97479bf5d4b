"""CPU: VO.OBS_TRANSFORM / RL.OBS_TRANSFORM host logic against tests/golden/obs_transform.npz (captured from the reference's
misc_utils transforms and its _compute_local_delta_states_from_vo with a transformer set): the size and crop arithmetic, a torch
restatement of the reference's call sequence (the one test_gpu_obs_transform.py checks the kernel against) pinned to the fixture
digests, the observation-space overwrite quirk, and the errors raised before any launch."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from pointnav_vo_amd import _lib, synth
from pointnav_vo_amd.obs_transforms import MODES, ResizeCenterCropper, Resizer, as_transform, transformed_size
from pointnav_vo_amd.trainer import AttrDict, BaseRLTrainerWithVO

REC = load_golden("obs_transform.npz")
W, H, BINS = int(REC["width"]), int(REC["height"]), int(REC["bins"])


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.numpy(), dtype=np.float32).tobytes()).hexdigest()


def reference_obs_pairs(prev, cur, mode, channels_last=False):
    """The reference's sequence (base_trainer_with_vo.py:172-207 + misc_utils.py:241-318), restated with torch CPU ops and this
    package's transformed_size: float rgb / depth pairs concatenated to 8 NHWC channels, resampled by F.interpolate(mode='area')
    in the memory format the reference hands torch, center-cropped, split.  Returns (rgb [H,W,6], depth [H,W,2])."""
    rgb = torch.cat([torch.FloatTensor(prev["rgb"]), torch.FloatTensor(cur["rgb"])], dim=2)[None]
    dep = torch.cat([torch.FloatTensor(prev["depth"]), torch.FloatTensor(cur["depth"])], dim=2)[None]
    x = torch.cat((rgb, dep), dim=3)
    h, w = x.shape[1:3]
    rs_h, rs_w, cy, cx, oh, ow = transformed_size(h, w, mode, (W, H))
    x = x.permute(0, 3, 1, 2)
    if channels_last:
        x = x.contiguous()
    y = F.interpolate(x, size=(rs_h, rs_w), mode="area")[..., cy:cy + oh, cx:cx + ow].permute(0, 2, 3, 1)
    return y[0, :, :, :6], y[0, :, :, 6:]


def onehot(depth):
    """_discretize_depth_func (base_trainer_with_vo.py:135-167) restated: bins [i/B, (i+1)/B), the last one closed."""
    ends = [i * 1.0 / BINS for i in np.arange(BINS)] + [1.0]
    out = torch.zeros(depth.shape + (BINS,))
    for i in range(BINS):
        hi = depth <= ends[i + 1] if i == BINS - 1 else depth < ends[i + 1]
        out[..., i][(depth >= ends[i]) & hi] = 1.0
    return out


@pytest.mark.parametrize("k", range(len(REC["size_cases"])))
def test_sizes_and_crop_match_the_reference(k):
    h, w, m = (int(v) for v in REC["size_cases"][k])
    rs_h, rs_w, cy, cx, oh, ow = transformed_size(h, w, MODES[m], (W, H))
    assert (oh, ow) == tuple(int(v) for v in REC["size_out"][k])
    tr = (Resizer if MODES[m] == "resize" else ResizeCenterCropper)((W, H))
    assert tr.output_size(h, w) == (oh, ow)


def test_documented_examples():
    assert transformed_size(360, 640, "resize", (W, H)) == (192, 341, 0, 0, 192, 341)
    assert transformed_size(360, 640, "resize_crop", (W, H)) == (341, 606, 74, 133, 192, 341)
    assert transformed_size(192, 341, "resize_crop", (W, H))[:2] == (341, 605)        # upsampling
    assert transformed_size(480, 640, "resize", (W, H))[4:] == (192, 256)             # does not fit the model


@pytest.mark.parametrize("c", range(len(REC["boundary_cases"])))
def test_restatement_matches_the_reference_digests(c):
    h, w, m, fp16 = (int(v) for v in REC["boundary_cases"][c])
    seed = int(REC["obs_seed"])
    for s, (pi, ci, _act, zb) in enumerate(REC["steps"]):
        prev = synth.make_raw_obs(h, w, seed=seed, index=int(pi), zero_border=int(zb), depth_fp16=bool(fp16))
        cur = synth.make_raw_obs(h, w, seed=seed, index=int(ci), zero_border=int(zb), depth_fp16=bool(fp16))
        rgb, dep = reference_obs_pairs(prev, cur, MODES[m])
        assert sha(rgb) == str(REC[f"c{c}/s{s}/rgb/sha"]), (c, s)
        assert sha(dep) == str(REC[f"c{c}/s{s}/depth/sha"]), (c, s)
        dd = torch.cat((onehot(dep[..., 0]), onehot(dep[..., 1])), dim=2)
        assert sha(dd) == str(REC[f"c{c}/s{s}/discretized_depth/sha"]), (c, s)
        if h > H:                                        # downsampling: the two division rules differ, so the digest pins the rule
            rgb_c, dep_c = reference_obs_pairs(prev, cur, MODES[m], channels_last=True)
            assert not (torch.equal(rgb_c, rgb) and torch.equal(dep_c, dep))


def test_observation_space_overwrite_quirk():
    class Box:
        def __init__(self, shape):
            self.shape = shape

    class Space:
        def __init__(self, d):
            self.spaces = d

    sp = Space({"depth": Box((360, 640, 1)), "rgb": Box((360, 640, 3)), "pointgoal_with_gps_compass": Box((2,))})
    out = ResizeCenterCropper((W, H)).transform_observation_space(sp)
    assert tuple(out.spaces["depth"].shape) == tuple(REC["space_depth"]) == (W, H, 1)     # (W, H), not (H, W)
    assert tuple(out.spaces["rgb"].shape) == tuple(REC["space_rgb"])
    assert tuple(out.spaces["pointgoal_with_gps_compass"].shape) == tuple(REC["space_goal"])
    assert tuple(sp.spaces["depth"].shape) == (360, 640, 1)                               # a deep copy


def test_reference_instances_are_accepted_by_duck_type():
    ResizeCenterCropper_ = type("ResizeCenterCropper", (), {"_size": (W, H), "channels_last": False})
    t = as_transform(ResizeCenterCropper_())
    assert isinstance(t, ResizeCenterCropper) and t._size == (W, H) and not t.channels_last
    with pytest.raises(NotImplementedError):
        as_transform(type("Other", (), {"_size": (W, H), "channels_last": False})())


def test_size_mismatch_raises_before_any_launch():
    cfg = AttrDict(VO=dict(VO_TYPE="REGRESS", OBS_TRANSFORM="resize", VIS_SIZE_W=W, VIS_SIZE_H=H,
                           REGRESS_MODEL=dict(name="vo_cnn_rgb_d_dd_top_down", visual_type=["rgb", "depth"], regress_type="sep_act",
                                              mode="det", discretized_depth_channels=BINS)))
    t = BaseRLTrainerWithVO(cfg, torch.device("cpu"))
    t._set_up_vo_obs_transformer()
    assert isinstance(t._vo_obs_transformer, Resizer)
    obs = synth.make_raw_obs(480, 640, seed=0)
    with pytest.raises(ValueError, match=r"480x640.*192x256.*192x341"):
        t.compute_local_delta_states_batch([obs], [obs], [1])
    cfg.VO.OBS_TRANSFORM = "resize_crop"
    t._set_up_vo_obs_transformer()
    assert isinstance(t._vo_obs_transformer, ResizeCenterCropper)
    cfg.VO.OBS_TRANSFORM = "none"
    t._set_up_vo_obs_transformer()
    assert t._vo_obs_transformer is None


def test_resize_kernel_rejects_bad_arguments():
    fake = C.c_void_p(16)                                # never dereferenced: the checks come first
    ok = dict(n=1, h=360, w=640, c=3, rs=(192, 341), crop=(0, 0), out=(192, 341))

    def call(**kw):
        a = dict(ok, **kw)
        return _lib.lib.pnvo_resize_area(fake, 0, a["n"], a["h"], a["w"], a["c"], a["h"] * a["w"] * 3, a["w"] * 3, 3, a["rs"][0], a["rs"][1],
                                         a["crop"][0], a["crop"][1], a["out"][0], a["out"][1], fake, 1, 192 * 341 * 3, 0, 341 * 3, 3,
                                         1, None)
    assert call(c=5) == -1                               # up to 4 channels
    assert call(crop=(1, 0)) == -1                       # the window leaves the resized grid
    assert b"outside the resized" in _lib.lib.pnvo_last_error(None)
    assert call(n=-1) == -1
    assert call(n=0) == 0                                # nothing to do, nothing launched
