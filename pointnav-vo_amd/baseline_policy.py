"""HIP-backed PointNavBaselinePolicy: the policy the reference's plain PPOTrainer builds (rl/ppo/ppo_trainer.py:79-85; class at
rl/ppo/policy.py:82-163).

SimpleCNN (model_utils/visual_encoders/simple_cnn.py: three bias convs without normalisation and one large Linear) on
cat([rgb / 255, depth]), the raw goal vector behind its embedding, a one-layer GRU (RNNStateEncoder's defaults) and the two heads of
PointNavResNetPolicy.  Same positional constructor, same ``state_dict`` names / shapes / order, same ``act`` / ``get_value`` signatures
and return values.  The module tree only HOLDS parameters; a step is one call into libpnvo.so (pnvo_baseline_act: seven launches on the
caller's current HIP stream) plus the categorical sampling / arg-max over the logits, which stays in torch as in policy.py of this
package.  ``policy.net`` and ``policy.net.visual_encoder`` are callable as the reference's are.  ``evaluate_actions`` (the PPO update of
this policy) delegates to an attached ``ppo.BaselineTrainStep`` (``ppo.PPO(policy, ...)`` attaches one); the weights then live in that
step's flat buffer and the library reads them there.  No CPU fallback.
"""
import ctypes as C
import weakref

import torch
import torch.nn as nn

from . import _lib
from .policy import _Holder

MIN_FRAME = 36                                              # 36 -> 8 -> 3 -> 1: the smallest frame that leaves conv3 an output pixel
_CNN = "net.visual_encoder.cnn."
_RNN = "net.state_encoder.rnn."
_CONVS = ((8, 4), (4, 2), (3, 1))                           # (kernel, stride) of cnn.0 / cnn.2 / cnn.4, pad 0


class pnvo_baseline_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "rgb_channels", "depth_channels", "hidden", "n_actions", "goal_dim")]


def simple_cnn_dims(height, width):
    """[(h, w)] of the three conv maps: floor((d - k) / s) + 1 each (simple_cnn.py:102-127)."""
    dims, h, w = [], int(height), int(width)
    for k, s in _CONVS:
        h, w = (h - k) // s + 1, (w - k) // s + 1
        dims.append((h, w))
    return dims


def baseline_state_dict_spec(*, width, height, rgb_channels=3, depth_channels=1, hidden=512, n_actions=4, goal_dim=2):
    """(name, shape) of every tensor of PointNavBaselinePolicy.state_dict(), in its order; a blind policy (no rgb, no depth) has no
    cnn.* entries and a GRU that takes the goal alone."""
    c_in = rgb_channels + depth_channels
    spec = []
    if c_in:
        h, w = simple_cnn_dims(height, width)[-1]
        for i, (cout, cin, k) in zip((0, 2, 4), ((32, c_in, 8), (64, 32, 4), (32, 64, 3))):
            spec += [(f"{_CNN}{i}.weight", (cout, cin, k, k)), (f"{_CNN}{i}.bias", (cout,))]
        spec += [(_CNN + "6.weight", (hidden, 32 * h * w)), (_CNN + "6.bias", (hidden,))]
    k_in = (hidden if c_in else 0) + goal_dim
    spec += [(_RNN + "weight_ih_l0", (3 * hidden, k_in)), (_RNN + "weight_hh_l0", (3 * hidden, hidden)),
             (_RNN + "bias_ih_l0", (3 * hidden,)), (_RNN + "bias_hh_l0", (3 * hidden,))]
    spec += [("action_distribution.linear.weight", (n_actions, hidden)), ("action_distribution.linear.bias", (n_actions,)),
             ("critic.fc.weight", (1, hidden)), ("critic.fc.bias", (1,))]
    return spec


def _init(name, shape):
    t = torch.empty(shape)
    if not name.endswith("weight") and "weight_" not in name:           # every bias starts at zero
        return t.zero_()
    if name.startswith(_CNN):                                # SimpleCNN.layer_init (simple_cnn.py:129-134)
        nn.init.kaiming_normal_(t, nn.init.calculate_gain("relu"))
    elif name.startswith("action_distribution"):             # CategoricalNet (misc_utils.py:73-74)
        nn.init.orthogonal_(t, gain=0.01)
    else:                                                    # RNNStateEncoder.layer_init, CriticHead (policy.py:75)
        nn.init.orthogonal_(t)
    return t


class _Part(_Holder):
    """A callable piece of the policy that reaches it through a weak reference (the policy is no submodule of its own net)."""

    def _policy(self):
        pol = self._policy_ref()
        if pol is None:
            raise RuntimeError("this module is not part of a live policy: call it through policy.net")
        return pol

    @property
    def is_blind(self):
        return self._blind


class _Encoder(_Part):
    def forward(self, observations):
        """observations['rgb'] [B,H,W,3] (uint8 or float32, 0..255) and / or ['depth'] [B,H,W,1] -> [B, hidden] float32 on the device
        (pnvo_baseline_encode).  No gradient, no CPU fallback."""
        return self._policy()._encode(observations)


class _Net(_Part):
    @property
    def output_size(self):
        return self._hidden

    @property
    def num_recurrent_layers(self):
        return 1

    def forward(self, observations, rnn_hidden_states, prev_actions, masks):
        """-> (features [B,hidden], rnn_hidden_states [1,B,hidden])  (policy.py:152-163)."""
        with torch.no_grad():
            feats, hout, _, _ = self._policy()._net(observations, rnn_hidden_states, masks)
        return feats, hout


class PointNavBaselinePolicy(nn.Module):
    def __init__(self, observation_space, action_space, goal_sensor_uuid, hidden_size=512):
        super().__init__()
        spaces = observation_space.spaces
        shapes = {k: tuple(int(v) for v in spaces[k].shape) for k in ("rgb", "depth") if k in spaces}
        self._n_rgb = shapes["rgb"][2] if "rgb" in shapes else 0
        self._n_depth = shapes["depth"][2] if "depth" in shapes else 0
        if self._n_rgb not in (0, 3) or self._n_depth not in (0, 1):
            raise NotImplementedError(f"observation space with {self._n_rgb} rgb and {self._n_depth} depth channels: the HIP baseline "
                                      "policy takes rgb [H,W,3] and / or depth [H,W,1]")
        self._vis_keys = [k for k, n in (("rgb", self._n_rgb), ("depth", self._n_depth)) if n]
        self._blind = not self._vis_keys
        self._H = self._W = 0
        if not self._blind:
            self._H, self._W = shapes[self._vis_keys[0]][:2]       # the rgb frame's when both are there (simple_cnn.py:50-57)
            for k in self._vis_keys:
                if shapes[k][:2] != (self._H, self._W):
                    raise ValueError(f"observation space {k!r} has shape {shapes[k]}, expected {(self._H, self._W)} frames: the visual "
                                     "inputs are concatenated on the channel axis (simple_cnn.py:158)")
            if min(self._H, self._W) < MIN_FRAME:
                raise ValueError(f"frames of {self._W}x{self._H}: the baseline policy's SimpleCNN needs width and height >= {MIN_FRAME} "
                                 "(conv3 would have no output pixel)")
        self.goal_sensor_uuid = goal_sensor_uuid
        self._goal_dim = int(spaces[goal_sensor_uuid].shape[0])
        self.dim_actions = int(action_space.n)
        self._hidden = int(hidden_size)
        if self._hidden <= 0 or self._hidden % 8:
            raise ValueError(f"hidden_size {hidden_size}: the HIP baseline policy takes positive multiples of 8")
        if not 1 <= self.dim_actions <= 32 or not 1 <= self._goal_dim <= 8:
            raise ValueError(f"action_space.n {self.dim_actions} (1 to 32) / goal size {self._goal_dim} (1 to 8) outside the built range")
        self._spec = baseline_state_dict_spec(width=self._W, height=self._H, rgb_channels=self._n_rgb, depth_channels=self._n_depth,
                                              hidden=self._hidden, n_actions=self.dim_actions, goal_dim=self._goal_dim)
        net = _Net()
        self.add_module("net", net)
        enc = _Encoder()
        net.add_module("visual_encoder", enc)
        enc.add_module("cnn", _Holder())                     # nn.Sequential() without entries when blind (simple_cnn.py:59-60)
        for name, shape in self._spec:
            parts = name.split(".")
            mod = self
            for p in parts[:-1]:
                if not hasattr(mod, p):
                    mod.add_module(p, _Holder())
                mod = getattr(mod, p)
            mod.register_parameter(parts[-1], nn.Parameter(_init(name, tuple(shape))))
        for part in (net, enc):
            part._policy_ref, part._blind = weakref.ref(self), self._blind
        net._hidden = self._hidden
        self._handle = None
        self._handle_dev = None
        self._loaded_sig = None
        self._spec_tensors = None
        self._train_step = None                              # ppo.BaselineTrainStep once attached: the weights then live in its flat buffer

    # ------------------------------------------------------------------ libpnvo plumbing
    def _ensure(self, device):
        if self._train_step is not None:                     # the library reads the train step's flat buffer: nothing to upload
            if self._handle_dev != device.index:
                raise RuntimeError("the policy moved to another device after a BaselineTrainStep was attached")
            self._train_step._sync_params()
            return
        if self._handle is None or self._handle_dev != device.index:
            self._release()
            cc = pnvo_baseline_config(width=self._W, height=self._H, rgb_channels=self._n_rgb, depth_channels=self._n_depth,
                                      hidden=self._hidden, n_actions=self.dim_actions, goal_dim=self._goal_dim)
            h = C.c_void_p()
            _lib.check(_lib.lib.pnvo_baseline_create(C.byref(cc), int(device.index or 0), C.byref(h)))
            self._handle, self._handle_dev, self._loaded_sig = h, device.index, None
        tensors = self._spec_tensors                        # (the walk over the module tree is kept until _apply)
        if tensors is None:
            sd = dict(self.named_parameters())
            tensors = self._spec_tensors = [(n, sd[n]) for n, _ in self._spec]
        sig = tuple([(t.data_ptr(), t._version) for _, t in tensors])
        if sig != self._loaded_sig:                          # parameters changed (load_state_dict, an optimiser step): re-read them
            blob, toc = _lib.pack_tensors(tensors)
            _lib.check(_lib.lib.pnvo_baseline_load_weights(self._handle, blob.ctypes.data_as(C.c_void_p), blob.size, toc, len(tensors)))
            self._loaded_sig = sig

    def _apply(self, fn, *a, **k):                          # .to() / .cuda() / .float(): parameters may be replaced
        self._spec_tensors = None
        return super()._apply(fn, *a, **k)

    def _release(self):
        if getattr(self, "_handle", None) is not None:
            _lib.lib.pnvo_baseline_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _device(self):
        ref = next(self.parameters())
        if ref.device.type != "cuda":
            raise RuntimeError("pointnav_vo_amd policies run on an MI355X only: move the policy with .to('cuda') "
                               "(there is no CPU fallback)")
        return ref.device

    def _frames(self, observations, dev):
        """(rgb, rgb_is_u8, depth, B) as the library takes them, checked before anything is launched."""
        out = {"rgb": None, "depth": None}
        B = None
        for k, n in (("rgb", self._n_rgb), ("depth", self._n_depth)):
            if not n:
                continue
            if k not in observations:
                raise ValueError(f"observations hold no {k!r} (keys: {sorted(observations.keys())})")
            t = observations[k]
            if k == "rgb" and t.dtype not in (torch.uint8, torch.float32):
                raise ValueError(f"observations['rgb'] has dtype {t.dtype}, expected torch.uint8 or torch.float32 (values 0..255)")
            if t.dim() != 4 or tuple(t.shape[1:]) != (self._H, self._W, n):
                raise ValueError(f"observations[{k!r}] has shape {tuple(t.shape)}, expected [B,{self._H},{self._W},{n}]")
            if B is not None and t.shape[0] != B:
                raise ValueError(f"observations['rgb'] holds {B} frames, observations['depth'] {t.shape[0]}")
            B = int(t.shape[0])
            out[k] = (t.to(device=dev) if k == "rgb" else t.to(device=dev, dtype=torch.float32)).contiguous()
        return out["rgb"], int(out["rgb"] is not None and out["rgb"].dtype == torch.uint8), out["depth"], B

    # ------------------------------------------------------------------ forward
    def _encode(self, observations):
        dev = self._device()
        if self._blind:
            raise RuntimeError("a blind policy has no visual encoder (net.is_blind)")
        rgb, u8, depth, B = self._frames(observations, dev)
        self._ensure(dev)
        out = torch.empty((B, self._hidden), device=dev, dtype=torch.float32)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        if B:
            with torch.cuda.device(dev):
                stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                _lib.check(_lib.lib.pnvo_baseline_encode(self._handle, p(rgb), u8, p(depth), B, p(out), stream))
        return out

    def _net(self, observations, rnn_hidden_states, masks, want_features=True):
        dev = self._device()
        rgb, u8, depth, B = self._frames(observations, dev)
        goal = observations[self.goal_sensor_uuid].to(device=dev, dtype=torch.float32).contiguous()
        if B is None:
            B = int(goal.shape[0])
        goal = goal.reshape(B, self._goal_dim)
        self._ensure(dev)
        mk = masks.to(device=dev, dtype=torch.float32).contiguous().reshape(B)
        hin = rnn_hidden_states.to(device=dev, dtype=torch.float32).contiguous()
        assert tuple(hin.shape) == (1, B, self._hidden), tuple(hin.shape)
        hout = torch.empty_like(hin)
        feats = torch.empty((B, self._hidden), device=dev, dtype=torch.float32) if want_features else None
        logits = torch.empty((B, self.dim_actions), device=dev, dtype=torch.float32)
        value = torch.empty((B, 1), device=dev, dtype=torch.float32)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(_lib.lib.pnvo_baseline_act(self._handle, p(rgb), u8, p(depth), p(goal), p(mk), p(hin), B, p(hout), p(feats),
                                                  p(logits), p(value), stream))
        return feats, hout, logits, value

    def forward(self, *x):
        raise NotImplementedError                          # as the reference (policy.py:31-32)

    def act(self, observations, rnn_hidden_states, prev_actions, masks, deterministic=False):
        """-> (value [B,1], action [B,1] int64, action_log_probs [B,1], rnn_hidden_states [1,B,hidden])  (policy.py:34-50);
        prev_actions is accepted and ignored, as in the reference's net."""
        with torch.no_grad():
            _, hout, logits, value = self._net(observations, rnn_hidden_states, masks, want_features=False)
            logp_all = torch.log_softmax(logits, dim=-1)    # CategoricalNet's distribution, written out as in policy.py of this package
            probs = logp_all.exp()
            action = probs.argmax(dim=-1, keepdim=True) if deterministic else torch.multinomial(probs, 1, True)
            logp = logp_all.gather(-1, action)
        return value, action, logp, hout

    def get_value(self, observations, rnn_hidden_states, prev_actions, masks):
        with torch.no_grad():
            return self._net(observations, rnn_hidden_states, masks, want_features=False)[3]

    def features_and_logits(self, observations, rnn_hidden_states, prev_actions, masks):
        """(features [B,hidden], rnn_hidden_states, logits [B,n], value [B,1]) — for checkers."""
        with torch.no_grad():
            return self._net(observations, rnn_hidden_states, masks)

    def evaluate_actions(self, observations, rnn_hidden_states, prev_actions, masks, action):
        """-> (value [M,1], action_log_probs [M,1], distribution_entropy, rnn_hidden_states)  (policy.py:52-63), for a policy with a
        ppo.BaselineTrainStep attached; gradients come from that step's backward(), not from autograd."""
        if self._train_step is None:
            raise NotImplementedError("the PPO update of the baseline policy (policy.py:56-68) needs a train step: attach one with "
                                      "pointnav_vo_amd.ppo.BaselineTrainStep(policy) or ppo.PPO(policy, ...)")
        return self._train_step.evaluate_actions(observations, rnn_hidden_states, prev_actions, masks, action)
