"""Observation transforms on the device: mirrors of the reference's ResizeCenterCropper and Resizer.

  ResizeCenterCropper          /root/reference/pointnav_vo/utils/misc_utils.py:81-121
  Resizer                      misc_utils.py:330-366
  image_resize_shortest_edge   misc_utils.py:241-288  (F.interpolate(mode="area") == adaptive_avg_pool2d)
  center_crop                  misc_utils.py:291-318

The sizes are computed on the host with Python floats exactly as the reference does (``transformed_size``); the resampling and
the crop run in ONE launch of libpnvo.so's pnvo_resize_area (csrc/obs_resize.hip), which computes only the crop window.

torch's CPU area kernel divides by the window in two ways, chosen by the memory format it receives, and the results differ in the
last bit for ~15-20 % of the outputs.  Both are reproduced bit-exactly:
  contiguous NCHW input                      (sum / kh) / kw                          DIV_CONTIGUOUS
  channels-last input (NCHW view of NHWC)    sum / (kh * kw) for the channels in whole 8-float vectors of torch's kernel,
                                             (sum / kh) / kw for the remaining C % 8 channels                 DIV_CHANNELS_LAST
The VO boundary hands torch an 8-channel NHWC tensor permuted without .contiguous() (base_trainer_with_vo.py:195-207): every
channel takes sum / (kh * kw).  The policy hands it depth permuted and made contiguous (resnet_policy.py:157-168): (sum / kh) / kw.
"""
import copy
import ctypes as C
import numbers

import torch
import torch.nn as nn

from . import _lib

DIV_CONTIGUOUS = 0
DIV_CHANNELS_LAST = 1
_TORCH_CL_VEC = 8          # channels torch's channels-last kernel divides with one vector op: c < C - C % 8 take sum / (kh * kw)

MODES = ("resize", "resize_crop")


def transformed_size(h, w, mode, size):
    """Sizes of one transform of an h x w frame: (rs_h, rs_w, crop_y, crop_x, out_h, out_w) — the resized grid and the output
    window inside it.  mode 'resize' (Resizer) or 'resize_crop' (ResizeCenterCropper); size = (W, H) as the reference's `size`."""
    if mode not in MODES:
        raise ValueError(f"unknown observation transform {mode!r} (expected one of {MODES})")
    if isinstance(size, numbers.Number):
        size = (int(size), int(size))
    cw, ch = int(size[0]), int(size[1])
    edge = min(cw, ch) if mode == "resize" else max(cw, ch)
    scale = edge / min(h, w)                               # misc_utils.py:274-277: Python floats, int() truncation
    rs_h, rs_w = int(h * scale), int(w * scale)
    if mode == "resize":
        return rs_h, rs_w, 0, 0, rs_h, rs_w
    startx = rs_w // 2 - (cw // 2)                         # center_crop, misc_utils.py:310-311
    starty = rs_h // 2 - (ch // 2)
    if startx < 0 or starty < 0 or starty + ch > rs_h or startx + cw > rs_w:
        raise ValueError(f"center crop {ch}x{cw} does not fit the resized {rs_h}x{rs_w} grid of a {h}x{w} frame")
    return rs_h, rs_w, starty, startx, ch, cw


def launch_resize(src, dtype, n, in_h, in_w, channels, src_strides, geom, dst, group, dst_strides, div_rule, dev):
    """One pnvo_resize_area launch on the current stream of `dev`.  src / dst: integer device addresses; src_strides = (frame, row,
    pixel) and dst_strides = (group, member, row, pixel) in elements; geom = transformed_size(...)."""
    rs_h, rs_w, cy, cx, oh, ow = geom
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.pnvo_resize_area(
            C.c_void_p(src), 0 if dtype == torch.uint8 else 1, int(n), int(in_h), int(in_w), int(channels), *[int(s) for s in src_strides],
            int(rs_h), int(rs_w), int(cy), int(cx), int(oh), int(ow), C.c_void_p(dst), int(group), *[int(s) for s in dst_strides],
            int(div_rule), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))


def _overwrite_box_shape(box, shape):
    """overwrite_gym_box_shape (misc_utils.py:321-327) without requiring gym: a gym Box is rebuilt as the reference does, any other
    space object is copied with its `shape` replaced."""
    if tuple(box.shape) == tuple(shape):
        return box
    shape = list(shape) + list(box.shape[len(shape):])
    try:
        from gym.spaces import Box
    except ImportError:
        Box = None
    if Box is not None and isinstance(box, Box):
        import numpy as np
        low = box.low if np.isscalar(box.low) else np.min(box.low)
        high = box.high if np.isscalar(box.high) else np.max(box.high)
        return Box(low=low, high=high, shape=shape, dtype=box.dtype)
    new = copy.copy(box)
    new.shape = tuple(shape)
    return new


class _AreaTransform(nn.Module):
    mode = None

    def __init__(self, size, channels_last: bool = False):
        super().__init__()
        if isinstance(size, numbers.Number):
            size = (int(size), int(size))
        assert len(size) == 2, "forced input size must be len of 2 (w, h)"
        self._size = size
        self.channels_last = channels_last

    def transform_observation_space(self, observation_space, trans_keys=("rgb", "depth", "semantic")):
        """As the reference: every listed space's shape becomes `size` = (W, H) + its trailing dims — note (W, H, C), not (H, W, C);
        the reference's encoders only use the product of the two (resnet_policy.py:85-95)."""
        size = self._size
        observation_space = copy.deepcopy(observation_space)
        if size:
            for key in observation_space.spaces:
                if key in trans_keys and observation_space.spaces[key].shape != size:
                    observation_space.spaces[key] = _overwrite_box_shape(observation_space.spaces[key], size)
        self.observation_space = observation_space
        return observation_space

    def output_size(self, h, w):
        """(out_h, out_w) of an h x w input."""
        return transformed_size(h, w, self.mode, self._size)[4:]

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        """input: CUDA uint8 / float32, [N,C,H,W] (channels_last False) or [N,H,W,C] (channels_last True), or without N.  Returns float32
        (the reference's .to(img.dtype) of a float32 input) in the same layout, the divisions as torch's for that memory format."""
        if self._size is None:
            return input
        x = input
        if not x.is_cuda or x.dtype not in (torch.uint8, torch.float32):
            raise TypeError("the observation transform takes CUDA uint8 / float32 tensors (there is no CPU fallback)")
        no_batch = x.dim() == 3
        if no_batch:
            x = x.unsqueeze(0)
        if x.dim() != 4:
            raise NotImplementedError("4-D (or 3-D) image tensors only")
        if self.channels_last:
            N, H, W, Cc = x.shape
            nhwc = x.contiguous()                          # the reference permutes to NCHW and calls .contiguous()
            full = 0
        else:
            N, Cc, H, W = x.shape
            cl = x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()
            nhwc = x.permute(0, 2, 3, 1) if cl else None
            full = (Cc - Cc % _TORCH_CL_VEC) if cl else 0    # channels that take torch's vector division
        geom = transformed_size(H, W, self.mode, self._size)
        oh, ow = geom[4:]
        dev = x.device
        out = torch.empty((N, oh, ow, Cc), dtype=torch.float32, device=dev)
        if nhwc is not None:
            s = nhwc.stride()
            es = nhwc.element_size()
            for c0 in range(0, Cc, 4):                     # up to 4 adjacent channels per launch
                cnt = min(4, Cc - c0)
                for lo, hi, rule in ((c0, min(c0 + cnt, full), DIV_CHANNELS_LAST), (max(c0, full), c0 + cnt, DIV_CONTIGUOUS)):
                    if hi > lo:
                        launch_resize(nhwc.data_ptr() + lo * s[3] * es, x.dtype, N, H, W, hi - lo, (s[0], s[1], s[2]), geom,
                                      out.data_ptr() + lo * 4, 1, (oh * ow * Cc, 0, ow * Cc, Cc), rule, dev)
        else:                                              # contiguous NCHW: every (n, c) plane is a 1-channel frame
            planes = x.contiguous()
            launch_resize(planes.data_ptr(), x.dtype, N * Cc, H, W, 1, (H * W, W, 1), geom, out.data_ptr(), Cc,
                          (oh * ow * Cc, 1, ow * Cc, Cc), DIV_CONTIGUOUS, dev)
        if not self.channels_last:
            out = out.permute(0, 3, 1, 2)                  # (channels-last memory, as torch's output for either input format here)
            if nhwc is None:
                out = out.contiguous()
        if no_batch:
            out = out.squeeze(0)
        return out


class ResizeCenterCropper(_AreaTransform):
    """Resize the shortest edge to max(size), then center-crop to size = (W, H)  (misc_utils.py:81-121)."""
    mode = "resize_crop"


class Resizer(_AreaTransform):
    """Resize the shortest edge to min(size)  (misc_utils.py:330-366)."""
    mode = "resize"


def as_transform(obj):
    """This package's transform for `obj`: one of ours, or a duck-typed reference instance (ResizeCenterCropper / Resizer from
    pointnav_vo.utils.misc_utils — what the reference trainers construct from RL.OBS_TRANSFORM, ddppo_trainer.py:92-103).  None
    stays None."""
    if obj is None or isinstance(obj, _AreaTransform):
        return obj
    name = type(obj).__name__
    cls = {"ResizeCenterCropper": ResizeCenterCropper, "Resizer": Resizer}.get(name)
    if cls is None or not hasattr(obj, "_size") or not hasattr(obj, "channels_last"):
        raise NotImplementedError(f"observation transform {name} is not built (ResizeCenterCropper and Resizer are)")
    return cls(obj._size, channels_last=bool(obj.channels_last))
