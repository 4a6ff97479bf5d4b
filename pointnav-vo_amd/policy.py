"""HIP-backed navigation policy registered under the reference's name ``resnet_rnn_policy``.

Drop-in for PointNavResNetPolicy (/root/reference/pointnav_vo/rl/policies/resnet_policy.py:25-58) in the configurations
the reference's nav loop uses (configs/rl/ddppo_pointnav.yaml:48-54: resnet18 encoder, 2-layer LSTM — or GRU, the other
value RL.Policy.rnn_backbone takes (rnn_state_encoder.py:28) — RL.OBS_TRANSFORM 'none', 'resize' or 'resize_crop';
RL.Policy.visual_types 'depth', 'rgb' or both, normalize_visual_inputs False or True with RunningMeanAndVar's three buffers updated on
the device whenever the policy runs in training mode, single process): same constructor keywords (ddppo_trainer.py:122-133), same
``state_dict`` keys/shapes, same ``act`` / ``get_value`` signatures and return values (policy.py:29-50).  The module tree
only HOLDS parameters; ``act`` is one call into libpnvo.so (pnvo_policy_act) on the caller's current HIP stream plus the
categorical sampling / arg-max over the 4 logits, which stays in torch as in the reference (policy.py:38-43).
``evaluate_actions`` (PPO training of the policy) exists once a ``ppo.PolicyTrainStep`` has been attached to the policy (ppo.py: the
rollout forward, back-propagation through time and Adam on one flat buffer); a plain policy raises NotImplementedError.
``policy.net.visual_encoder`` is callable (pnvo_policy_encode) and has ``output_shape``, and ``act`` / ``get_value`` / ``evaluate_actions``
take ``observations["visual_features"]`` in place of ``depth`` (resnet_policy.py:249-252): the reference trainers' frozen-encoder
branch (RL.DDPPO.train_encoder False, ddppo_trainer.py:158-161,257-271).  No CPU fallback.
"""
import ctypes as C
import math
import weakref

import torch
import torch.nn as nn

from . import _lib
from . import model_spec as ms
from .obs_transforms import DIV_CONTIGUOUS, as_transform, launch_resize, transformed_size
from .registry import baseline_registry

GOAL_SENSOR = "pointgoal_with_gps_compass"
FEATURES_KEY = "visual_features"                         # ddppo_trainer.py:257-271, resnet_policy.py:249-252


class _Holder(nn.Module):
    pass


class pnvo_policy_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "baseplanes", "hidden", "n_actions", "rnn_layers", "flat_size", "rnn_type",
                                         "rgb_channels", "no_depth", "normalize", "backbone_depth", "resnext", "se")]


# rnn_type -> (pnvo_policy_config.rnn_type, gate blocks per weight, state tensors per layer): torch.nn.LSTM (i, f, g, o; h and c),
# torch.nn.GRU (r, z, n; h only)
RNN_TYPES = {"LSTM": (0, 4, 2), "GRU": (1, 3, 1)}


def _rnn(rnn_type):
    if rnn_type not in RNN_TYPES:
        raise NotImplementedError(f"rnn_type {rnn_type!r}: the HIP policy implements 'LSTM' and 'GRU'")
    return RNN_TYPES[rnn_type]


def encoder_output_shape(*, width, height, flat_size=2048):
    """ResNetEncoder.output_shape (resnet_policy.py:106-133) for a [height, width] depth frame: (C, fh, fw) with
    fh, fw = ceil((H // 2) / 32), ceil((W // 2) / 32) — avg_pool2d(2), then the backbone's final_spatial_compress of 1 / 32 — and
    C = round(flat_size / (fh * fw)): the shape of the tensor the encoder returns, rows before columns."""
    fh, fw = int(math.ceil((height // 2) / 32)), int(math.ceil((width // 2) / 32))
    return int(round(flat_size / (fh * fw))), fh, fw


RMV_PREFIX = "net.visual_encoder.running_mean_and_var."


def visual_channels(vis_types):
    """(rgb channels, depth channels) the encoder takes for RL.Policy.visual_types: membership, as the reference tests it
    (resnet_policy.py:82-94); torch.cat order is rgb, then depth (:150-167)."""
    n_rgb, n_depth = (3 if "rgb" in vis_types else 0), (1 if "depth" in vis_types else 0)
    if n_rgb + n_depth == 0:
        raise NotImplementedError(f"vis_types {list(vis_types)!r}: the HIP policy is not blind (it takes 'depth', 'rgb' or both)")
    return n_rgb, n_depth


def policy_state_dict_spec(*, width, height, baseplanes=32, hidden=512, n_actions=4, rnn_layers=2, flat_size=2048, rnn_type="LSTM",
                           vis_types=("depth",), normalize_visual_inputs=False, backbone="resnet18"):
    """(name, shape) of every tensor of PointNavResNetPolicy.state_dict(), in its order, for each of the seven backbones of
    resnet.py:226-286 (model_spec.BACKBONES); with normalize_visual_inputs the three RunningMeanAndVar buffers come first among the
    encoder's entries."""
    gates = _rnn(rnn_type)[1]
    n_in = sum(visual_channels(vis_types))
    spec = []
    pre = "net.visual_encoder."
    bb = pre + "backbone."
    if normalize_visual_inputs:                          # running_mean_and_var.py:16-18
        spec += [(RMV_PREFIX + "_mean", (1, n_in, 1, 1)), (RMV_PREFIX + "_var", (1, n_in, 1, 1)), (RMV_PREFIX + "_count", ())]
    spec += [(bb + "conv1.0.weight", (baseplanes, n_in, 7, 7)), (bb + "conv1.1.weight", (baseplanes,)),
             (bb + "conv1.1.bias", (baseplanes,))]
    # the residual stages on the pooled frame (F.avg_pool2d(x, 2), then stem stride 2 + maxpool): the VO models' block table
    # (model_spec.block_plan: BasicBlock, Bottleneck, ResNeXt and SE blocks)
    cfg = ms.config_from_kwargs(observation_space={"depth": None}, observation_size=(width // 2, height // 2),
                                resnet_baseplanes=baseplanes, backbone=backbone)
    blocks, (cin, h, w) = ms.block_plan(cfg, bb)
    for prefix, convs, se in blocks:
        spec += ms.block_spec(prefix, convs, se)
    comp = int(round(flat_size / (h * w)))               # resnet_policy.py:113-117 (python round)
    spec += [(pre + "compression.0.weight", (comp, cin, 3, 3)), (pre + "compression.1.weight", (comp,)),
             (pre + "compression.1.bias", (comp,))]
    spec = [("net.prev_action_embedding.weight", (n_actions + 1, 32)), ("net.tgt_embeding.weight", (32, 3)),
            ("net.tgt_embeding.bias", (32,))] + spec
    assert (comp, h, w) == encoder_output_shape(width=width, height=height, flat_size=flat_size)
    spec += [("net.visual_fc.1.weight", (hidden, comp * h * w)), ("net.visual_fc.1.bias", (hidden,))]
    for layer in range(rnn_layers):
        k = hidden + 64 if layer == 0 else hidden
        r = "net.state_encoder.rnn."
        spec += [(f"{r}weight_ih_l{layer}", (gates * hidden, k)), (f"{r}weight_hh_l{layer}", (gates * hidden, hidden)),
                 (f"{r}bias_ih_l{layer}", (gates * hidden,)), (f"{r}bias_hh_l{layer}", (gates * hidden,))]
    spec += [("action_distribution.linear.weight", (n_actions, hidden)), ("action_distribution.linear.bias", (n_actions,)),
             ("critic.fc.weight", (1, hidden)), ("critic.fc.bias", (1,))]
    return spec


def _init(name, shape):
    t = torch.empty(shape)
    leaf = name.rsplit(".", 1)[1]
    if "state_encoder.rnn" in name:                      # rnn_state_encoder.py:36-41
        nn.init.orthogonal_(t) if "weight" in leaf else t.zero_()
    elif name.startswith("action_distribution"):         # misc_utils.py:73-74
        nn.init.orthogonal_(t, gain=0.01) if leaf == "weight" else t.zero_()
    elif name.startswith("critic"):                      # policy.py:70-71
        nn.init.orthogonal_(t) if leaf == "weight" else t.zero_()
    elif name == "net.prev_action_embedding.weight":
        nn.init.normal_(t)
    elif ".se.excite." in name:                          # ResNetEncoder.layer_init covers the SE branch's Linear layers too
        nn.init.kaiming_normal_(t, nn.init.calculate_gain("relu")) if leaf == "weight" else t.zero_()
    elif len(shape) in (2, 4):                           # ResNetEncoder.layer_init / torch defaults
        nn.init.kaiming_normal_(t, nn.init.calculate_gain("relu")) if len(shape) == 4 else \
            nn.init.kaiming_uniform_(t, a=math.sqrt(5))
    elif leaf == "weight":
        t.fill_(1.0)                                     # GroupNorm gamma
    else:
        t.zero_()
    return t


class _Frames:
    """The visual input of one call of an rgb / rgb-d / normalised policy: the transformed frames on the device and the statistics
    buffers, as the *_rgbd entry points take them.  `shape[0]` is the number of frames."""

    def __init__(self, rgb, depth, stats):
        self.rgb, self.depth, self.stats = rgb, depth, stats
        self.shape = (rgb if rgb is not None else depth).shape[:1]

    def args(self):
        """(rgb, rgb_is_u8, depth, run_mean, run_var, run_count, training) of pnvo_policy_act_rgbd / _encode_rgbd / _evaluate_rgbd."""
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        mean, var, count, training = self.stats if self.stats is not None else (None, None, None, 0)
        return (p(self.rgb), int(self.rgb is not None and self.rgb.dtype == torch.uint8), p(self.depth), p(mean), p(var), p(count),
                int(training))


class _NetHolder(_Holder):
    """`policy.net` of the reference (PointNavResNetNet, resnet_policy.py:177-282) as far as its callers read it."""

    @property
    def num_recurrent_layers(self):
        return self._layers * self._states                 # LSTM: h and c, GRU: h (rnn_state_encoder.py:41-43)

    @property
    def output_size(self):
        return self._hidden

    @property
    def is_blind(self):
        return False                                       # a visual encoder is always present here


class _EncoderHolder(_Holder):
    """`policy.net.visual_encoder` of the reference (ResNetEncoder, resnet_policy.py:61-175) as the trainers' frozen-encoder branch uses
    it (ddppo_trainer.py:158-161,257-271; ppo_trainer.py:270-272): the holder of the encoder's parameters, callable on an observation
    dict, with output_shape.  The policy it belongs to is reached through a weak reference: the policy is neither a submodule nor a
    strong attribute of its own encoder."""

    @property
    def is_blind(self):
        return False

    @property
    def output_shape(self):
        return self._output_shape

    def _policy(self):
        pol = self._policy_ref()
        if pol is None or pol.net.visual_encoder is not self:       # (a copied module tree keeps the original's reference)
            raise RuntimeError("this visual encoder is not part of a live policy: call it through policy.net.visual_encoder")
        return pol

    def forward(self, observations):
        """observations['depth'] [B,Hs,Ws,1] and / or ['rgb'] [B,Hs,Ws,3] -> [B, C, fh, fw] float32 on the device: RL.OBS_TRANSFORM,
        avg_pool2d(2), RunningMeanAndVar (updated first when the policy is in training mode), the backbone, compression conv +
        GroupNorm(1) + ReLU (one call into libpnvo.so: pnvo_policy_encode / pnvo_policy_encode_rgbd).  No gradient, no CPU fallback."""
        return self._policy()._encode(observations)


@baseline_registry.register_policy(name="resnet_rnn_policy")
class PointNavResNetPolicy(nn.Module):
    def __init__(self, *, observation_space, action_space, goal_sensor_uuid=GOAL_SENSOR, hidden_size=512,
                 num_recurrent_layers=2, rnn_type="LSTM", resnet_baseplanes=32, backbone="resnet18",
                 normalize_visual_inputs=False, obs_transform=None, vis_types=("depth",), **kwargs):
        super().__init__()
        # resnet.py:226-286: resnet18 | resnet50 | resnet101 | resneXt50 | se_resnet50 | se_resneXt50 | se_resneXt101 (the reference
        # resolves the name with getattr(resnet, backbone)); every backbone but resnet18 runs frozen (ppo.PolicyTrainStep)
        self._backbone = backbone
        self._backbone_fields = ms.backbone_fields(backbone)
        self._rnn_type = rnn_type
        self._rnn_code, _, self._states = _rnn(rnn_type)
        self._n_rgb, self._n_depth = visual_channels(vis_types)
        self._normalize = bool(normalize_visual_inputs)
        # today's depth-only, un-normalised policy keeps its own path (pnvo_policy_act: the persistent small-batch encoder, the VO
        # frame-ring hand-off); every other configuration runs the *_rgbd entry points on the per-layer kernels
        self._plain = self._n_rgb == 0 and not self._normalize
        self._vis_keys = [k for k, n in (("rgb", self._n_rgb), ("depth", self._n_depth)) if n]
        for k in self._vis_keys:
            if k not in observation_space.spaces:
                raise ValueError(f"vis_types names {k!r}, which the observation space does not hold")
        if goal_sensor_uuid != GOAL_SENSOR:
            raise NotImplementedError(goal_sensor_uuid)
        # RL.OBS_TRANSFORM (ddppo_trainer.py:92-103,131): this package's ResizeCenterCropper / Resizer or the reference's own instances
        self._obs_transform = as_transform(obs_transform)
        if self._obs_transform is not None:
            if self._obs_transform.channels_last:
                raise NotImplementedError("the policy hands the transform NCHW frames (resnet_policy.py:150-167): channels_last=False")
            # the encoder runs on the transformed [VIS_H, VIS_W] frame; transform_observation_space writes (W, H, 1) into the depth
            # space (resnet_policy.py:75-80), which the reference's sizes only use through the product W * H
            self._obs_transform.transform_observation_space(observation_space)
            self._W, self._H = (int(v) for v in self._obs_transform._size)
        else:
            shapes = {k: tuple(int(v) for v in observation_space.spaces[k].shape) for k in self._vis_keys}     # (H, W, 3) / (H, W, 1)
            self._H, self._W = shapes[self._vis_keys[-1]][:2]
            for k, n in (("rgb", self._n_rgb), ("depth", self._n_depth)):
                if n and shapes[k] != (self._H, self._W, n):
                    raise ValueError(f"observation space {k!r} has shape {shapes[k]}, expected {(self._H, self._W, n)}: the visual "
                                     "types are concatenated on the channel axis (resnet_policy.py:167)")
        self._tgeom = {}
        self.dim_actions = int(action_space.n)
        self._hidden, self._layers, self._baseplanes = int(hidden_size), int(num_recurrent_layers), int(resnet_baseplanes)
        self._spec = policy_state_dict_spec(width=self._W, height=self._H, baseplanes=self._baseplanes,
                                            hidden=self._hidden, n_actions=self.dim_actions, rnn_layers=self._layers,
                                            rnn_type=rnn_type, vis_types=tuple(vis_types),
                                            normalize_visual_inputs=self._normalize, backbone=backbone)
        for name, shape in self._spec:
            parts = name.split(".")
            mod = self
            for p in parts[:-1]:
                if not hasattr(mod, p):
                    mod.add_module(p, _Holder())
                mod = getattr(mod, p)
            if name.startswith(RMV_PREFIX):                     # RunningMeanAndVar's statistics: buffers, zero (running_mean_and_var.py:16-18)
                mod.register_buffer(parts[-1], torch.zeros(tuple(shape)))
            else:
                mod.register_parameter(parts[-1], nn.Parameter(_init(name, tuple(shape))))
        self._param_spec = [(n, sh) for n, sh in self._spec if not n.startswith(RMV_PREFIX)]
        # the reference trainers read these through policy.net (ppo_trainer.py:618, ddppo_trainer.py:279)
        net = self.net
        net.__class__ = _NetHolder
        net._layers, net._hidden, net._states = self._layers, self._hidden, self._states
        # ... and call net.visual_encoder when RL.DDPPO.train_encoder is False (ddppo_trainer.py:257-271)
        enc = net.visual_encoder
        enc.__class__ = _EncoderHolder
        enc._output_shape = encoder_output_shape(width=self._W, height=self._H)
        enc._policy_ref = weakref.ref(self)
        self._feat_shape = enc._output_shape
        self._handle = None
        self._handle_dev = None
        self._loaded_sig = None
        self._train_step = None                            # ppo.PolicyTrainStep once attached: the weights then live in its flat buffer
        self._dist_stats = False                           # distributed_statistics(): RunningMeanAndVar's moments are all-reduced
        self._stats_hook = self._stats_sums = None         # (the callback object and the device buffer the library borrows)

    @property
    def num_recurrent_layers(self):
        return self._layers * self._states                 # LSTM: h and c, GRU: h (rnn_state_encoder.py:41-43)

    @property
    def output_size(self):
        return self._hidden

    # ------------------------------------------------------------------ libpnvo plumbing
    def distributed_statistics(self, on=True):
        """Opt in to (or out of) the cross-process reduction of RunningMeanAndVar's batch moments (running_mean_and_var.py:24-42 under
        torch.distributed): in training mode every act / get_value / net.visual_encoder / evaluate_actions call then all-reduces 2C + 1
        float64 sums over the default process group inside the input stage (one round, on the launch stream), so EVERY rank must make
        the same calls in the same order, and the three buffers must start out equal on all ranks (DDPPO.init_distributed broadcasts
        them).  A policy without normalize_visual_inputs has nothing to reduce."""
        self._dist_stats = bool(on) and self._normalize
        if self._handle is not None:
            self._install_stats_hook()
        return self

    def _on_stats(self, user, sums, n, stream):
        """pnvo_stats_reduce_fn: called by the input stage on the host; the sums are final on the launch stream (the current one)."""
        if torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            torch.distributed.all_reduce(self._stats_sums)

    def _install_stats_hook(self):
        on = self._stats_hook is not None
        if on == self._dist_stats:
            return
        if self._dist_stats:
            dev = torch.device("cuda", self._handle_dev or 0)
            self._stats_sums = torch.zeros(2 * (self._n_rgb + self._n_depth) + 1, device=dev, dtype=torch.float64)
            self._stats_hook = _lib.STATS_REDUCE_FN(self._on_stats)
            _lib.check(_lib.lib.pnvo_policy_set_stats_hook(self._handle, C.cast(self._stats_hook, C.c_void_p), None,
                                                           C.c_void_p(self._stats_sums.data_ptr())))
        else:
            _lib.check(_lib.lib.pnvo_policy_set_stats_hook(self._handle, None, None, None))
            self._stats_hook = self._stats_sums = None

    def _ensure(self, device):
        if self._train_step is not None:                    # the library reads the train step's flat buffer: nothing to upload
            if self._handle_dev != device.index:
                raise RuntimeError("the policy moved to another device after a PolicyTrainStep was attached")
            self._install_stats_hook()
            self._train_step._sync_params()
            return
        if self._handle is None or self._handle_dev != device.index:
            self._release()
            cc = pnvo_policy_config(width=self._W, height=self._H, baseplanes=self._baseplanes, hidden=self._hidden,
                                    n_actions=self.dim_actions, rnn_layers=self._layers, flat_size=2048,
                                    rnn_type=self._rnn_code, rgb_channels=self._n_rgb, no_depth=int(self._n_depth == 0),
                                    normalize=int(self._normalize), backbone_depth=self._backbone_fields[0],
                                    resnext=self._backbone_fields[1], se=self._backbone_fields[2])
            h = C.c_void_p()
            _lib.check(_lib.lib.pnvo_policy_create(C.byref(cc), int(device.index or 0), C.byref(h)))
            self._handle, self._handle_dev, self._loaded_sig = h, device.index, None
            self._stats_hook = self._stats_sums = None          # (a new handle has no hook yet)
        self._install_stats_hook()
        tensors = getattr(self, "_spec_tensors", None)      # (the walk over the module tree costs ~50 us per step: kept until _apply)
        if tensors is None:
            sd = dict(self.named_parameters())
            tensors = self._spec_tensors = [(n, sd[n]) for n, _ in self._param_spec]
        sig = tuple([(t.data_ptr(), t._version) for _, t in tensors])
        if sig != self._loaded_sig:
            blob, toc = _lib.pack_tensors(tensors)
            _lib.check(_lib.lib.pnvo_policy_load_weights(self._handle, blob.ctypes.data_as(C.c_void_p), blob.size, toc,
                                                         len(tensors)))
            self._loaded_sig = sig

    def _apply(self, fn, *a, **k):                          # .to() / .cuda() / .float(): parameters may be replaced
        self._spec_tensors = None
        return super()._apply(fn, *a, **k)

    def _release(self):
        if getattr(self, "_handle", None) is not None:
            _lib.lib.pnvo_policy_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    # ------------------------------------------------------------------ forward
    def _net(self, observations, rnn_hidden_states, prev_actions, masks, want_features=True):
        ref = next(self.parameters())
        if ref.device.type != "cuda":
            raise RuntimeError("pointnav_vo_amd policies run on an MI355X only: move the policy with .to('cuda') "
                               "(there is no CPU fallback)")
        dev = ref.device
        vis, from_features = self._visual_input(observations, dev)
        self._ensure(dev)
        B = vis.shape[0]
        goal = observations[GOAL_SENSOR].to(device=dev, dtype=torch.float32).contiguous().reshape(B, 2)
        pa = prev_actions.to(device=dev, dtype=torch.int64).contiguous().reshape(B)
        mk = masks.to(device=dev, dtype=torch.float32).contiguous().reshape(B)
        hin = rnn_hidden_states.to(device=dev, dtype=torch.float32).contiguous()
        assert tuple(hin.shape) == (self.num_recurrent_layers, B, self._hidden), tuple(hin.shape)
        hout = torch.empty_like(hin)
        feats = torch.empty((B, self._hidden), device=dev, dtype=torch.float32) if want_features else None
        logits = torch.empty((B, self.dim_actions), device=dev, dtype=torch.float32)
        value = torch.empty((B, 1), device=dev, dtype=torch.float32)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            if isinstance(vis, _Frames):
                _lib.check(_lib.lib.pnvo_policy_act_rgbd(self._handle, *vis.args(), p(goal), p(pa), p(mk), p(hin), int(B), p(hout), p(feats),
                                                         p(logits), p(value), stream))
            else:
                fn = _lib.lib.pnvo_policy_act_features if from_features else _lib.lib.pnvo_policy_act
                _lib.check(fn(self._handle, p(vis), p(goal), p(pa), p(mk), p(hin), int(B), p(hout), p(feats), p(logits), p(value), stream))
        return feats, hout, logits, value

    def _visual_input(self, observations, dev):
        """-> (input, from_features): observations['visual_features'] [B,C,fh,fw] when the key is present (resnet_policy.py:249-252: the
        encoder does not run, the frames need not be there and the statistics are not touched), else the transformed
        observations['depth'] [B,H,W,1] of the depth-only, un-normalised policy, else the _Frames of the other configurations.  Every
        check is made here, before anything is launched."""
        if FEATURES_KEY in observations:
            feats = observations[FEATURES_KEY].to(device=dev, dtype=torch.float32).contiguous()
            if feats.dim() < 1 or tuple(feats.shape[1:]) != tuple(self._feat_shape):
                raise ValueError(f"observations['{FEATURES_KEY}'] has shape {tuple(feats.shape)}, expected "
                                 f"{('B',) + tuple(self._feat_shape)} (net.visual_encoder.output_shape)")
            return feats, True
        return self._frames(observations, dev, f"observations hold neither '{FEATURES_KEY}' nor {{}} (keys: {{}}): the policy needs one "
                                               "of them"), False

    def _frames(self, observations, dev, missing):
        """The encoder's input from the sensor entries, checked (keys, dtype, shape, the statistics' process model) and transformed."""
        for k in self._vis_keys:
            if k not in observations:
                raise ValueError(missing.format(repr(k), sorted(observations.keys())))
        rgb = depth = None
        if self._n_rgb:
            rgb = observations["rgb"]
            # uint8 as the simulator hands it, float32 in 0..255 as batch_obs and RolloutStorage do: the same bits either way
            if rgb.dtype not in (torch.uint8, torch.float32):
                raise ValueError(f"observations['rgb'] has dtype {rgb.dtype}, expected torch.uint8 or torch.float32 (values 0..255)")
            if rgb.dim() != 4 or rgb.shape[3] != 3:
                raise ValueError(f"observations['rgb'] has shape {tuple(rgb.shape)}, expected [B,H,W,3]")
            if self._obs_transform is None and tuple(rgb.shape[1:]) != (self._H, self._W, 3):
                raise ValueError(f"observations['rgb'] has shape {tuple(rgb.shape)}, expected [B,{self._H},{self._W},3]")
        if self._n_depth:
            depth = observations["depth"]
            if depth.dim() != 4 or depth.shape[3] != 1:
                raise ValueError(f"observations['depth'] has shape {tuple(depth.shape)}, expected [B,H,W,1]")
            if self._obs_transform is None and tuple(depth.shape[1:]) != (self._H, self._W, 1):
                raise ValueError(f"observations['depth'] has shape {tuple(depth.shape)}, expected [B,{self._H},{self._W},1]")
            if rgb is not None and depth.shape[0] != rgb.shape[0]:
                raise ValueError(f"observations['rgb'] holds {rgb.shape[0]} frames, observations['depth'] {depth.shape[0]}")
        stats = self._statistics(dev) if not self._plain else None
        if self._obs_transform is not None:                     # (the geometry is checked before the first launch)
            for t in (rgb, depth):
                if t is not None:
                    self._transform_geometry(t.shape[1], t.shape[2])
        if depth is not None:
            depth = depth.to(device=dev, dtype=torch.float32).contiguous()
            if self._obs_transform is not None:
                depth = self._transform(depth, dev)
        if self._plain:
            return depth
        if rgb is not None:
            rgb = rgb.to(device=dev).contiguous()
            if self._obs_transform is not None:
                rgb = self._transform(rgb, dev)
        return _Frames(rgb, depth, stats)

    def _statistics(self, dev):
        """(_mean, _var, _count, training) of net.visual_encoder.running_mean_and_var as the library borrows them, or None without
        normalisation.  In training mode the reference all-reduces the batch moments over the processes (running_mean_and_var.py:
        27-38); here that reduction is an opt-in (distributed_statistics), because it makes every call a collective: without it a
        process group and training mode together are refused."""
        if not self._normalize:
            return None
        if self.training and not self._dist_stats and torch.distributed.is_available() and torch.distributed.is_initialized():
            raise NotImplementedError("normalize_visual_inputs in training mode under torch.distributed: the cross-process reduction "
                                      "(all_reduce) of RunningMeanAndVar's batch moments is off; call policy.distributed_statistics(True) "
                                      "(DDPPO.init_distributed does) so that every rank's calls reduce them, run one process, or call "
                                      ".eval() on the policy")
        rmv = self.net.visual_encoder.running_mean_and_var
        bufs = (rmv._mean, rmv._var, rmv._count)
        for name, b in zip(("_mean", "_var", "_count"), bufs):
            if b.device != dev or b.dtype != torch.float32 or not b.is_contiguous():
                raise RuntimeError(f"{RMV_PREFIX}{name} must be a contiguous float32 buffer on {dev} (it is {b.dtype} on {b.device})")
        return bufs + (int(self.training),)

    def _encode(self, observations):
        ref = next(self.parameters())
        if ref.device.type != "cuda":
            raise RuntimeError("pointnav_vo_amd policies run on an MI355X only: move the policy with .to('cuda') "
                               "(there is no CPU fallback)")
        dev = ref.device
        vis = self._frames(observations, dev, "net.visual_encoder needs observations[{}] (keys: {})")
        self._ensure(dev)
        B = vis.shape[0]
        out = torch.empty((B,) + tuple(self._feat_shape), device=dev, dtype=torch.float32)
        if B:
            with torch.cuda.device(dev):
                stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                if isinstance(vis, _Frames):
                    _lib.check(_lib.lib.pnvo_policy_encode_rgbd(self._handle, *vis.args(), int(B), C.c_void_p(out.data_ptr()), stream))
                else:
                    _lib.check(_lib.lib.pnvo_policy_encode(self._handle, C.c_void_p(vis.data_ptr()), int(B), C.c_void_p(out.data_ptr()),
                                                           stream))
        return out

    def _transform_geometry(self, Hs, Ws):
        geom = self._tgeom.get((Hs, Ws))
        if geom is None:
            geom = transformed_size(Hs, Ws, self._obs_transform.mode, self._obs_transform._size)
            if tuple(geom[4:]) != (self._H, self._W):
                raise ValueError(f"RL.OBS_TRANSFORM {self._obs_transform.mode!r} maps the {Hs}x{Ws} frame to {geom[4]}x{geom[5]}, but the "
                                 f"policy's encoder takes {self._H}x{self._W}")
            self._tgeom[(Hs, Ws)] = geom
        return geom

    def _transform(self, frames, dev):
        """[B,Hs,Ws,c] sensor frames (c = 1 depth, 3 rgb, uint8 or float32) -> [B,VIS_H,VIS_W,c] float32 by the observation transform,
        before avg_pool2d(2) (resnet_policy.py:150-168).  The reference permutes each sensor to [B,c,H,W] and calls .contiguous():
        torch's contiguous area kernel, (sum / kh) / kw per channel.  It divides rgb by 255 in front of the transform; here the raw
        0..255 values are resized and the input stage divides behind it (both steps are linear)."""
        B, Hs, Ws, c = (int(v) for v in frames.shape)
        geom = self._transform_geometry(Hs, Ws)
        out = torch.empty((B, self._H, self._W, c), device=dev, dtype=torch.float32)
        if B:
            launch_resize(frames.data_ptr(), frames.dtype, B, Hs, Ws, c, (Hs * Ws * c, Ws * c, c), geom, out.data_ptr(), 1,
                          (self._H * self._W * c, 0, self._W * c, c), DIV_CONTIGUOUS, dev)
        return out

    def forward(self, *x):
        raise NotImplementedError                          # as the reference (policy.py:26-27)

    def act(self, observations, rnn_hidden_states, prev_actions, masks, deterministic=False):
        """-> (value [B,1], action [B,1] int64, action_log_probs [B,1], rnn_hidden_states)  (policy.py:29-46)."""
        with torch.no_grad():
            _, hout, logits, value = self._net(observations, rnn_hidden_states, prev_actions, masks, want_features=False)
            # CategoricalNet's distribution (policy.py:29-46 -> utils.CategoricalNet): log-probabilities = logits - logsumexp, probabilities
            # = their softmax, sample = multinomial(probabilities, 1), log_prob = gather.  Written out (log_softmax, exp, multinomial,
            # gather: four launches instead of the distribution object's ten; the sampling call and its generator use are unchanged)
            logp_all = torch.log_softmax(logits, dim=-1)
            probs = logp_all.exp()
            action = probs.argmax(dim=-1, keepdim=True) if deterministic else torch.multinomial(probs, 1, True)
            logp = logp_all.gather(-1, action)
        return value, action, logp, hout

    def get_value(self, observations, rnn_hidden_states, prev_actions, masks):
        with torch.no_grad():
            return self._net(observations, rnn_hidden_states, prev_actions, masks)[3]

    def features_and_logits(self, observations, rnn_hidden_states, prev_actions, masks):
        """(features [B,hidden], rnn_hidden_states, logits [B,n], value [B,1]) — for checkers."""
        with torch.no_grad():
            return self._net(observations, rnn_hidden_states, prev_actions, masks)

    def evaluate_actions(self, observations, rnn_hidden_states, prev_actions, masks, action):
        """-> (value [M,1], action_log_probs [M,1], distribution_entropy, rnn_hidden_states)  (policy.py:52-63), for a policy with a
        ppo.PolicyTrainStep attached; gradients come from that step's backward(), not from autograd."""
        if self._train_step is None:
            raise NotImplementedError("PPO training of the policy (policy.py:52-63) is outside the built path "
                                      "(attach a train step first: pointnav_vo_amd.ppo.PolicyTrainStep(policy) or ppo.PPO(policy, ...))")
        return self._train_step.evaluate_actions(observations, rnn_hidden_states, prev_actions, masks, action)
