"""PPO update of the HIP navigation policy: the reference's `PPO` agent (pointnav_vo/rl/ppo/ppo.py) on libpnvo.so.

The reference tunes the policy against the VO estimates with this update (configs/rl/ddppo_pointnav.yaml: TUNE_WITH_VO, train_encoder,
num_steps 128, num_mini_batch 2, 2-layer LSTM; a policy built with rnn_type="GRU" runs the same calls on the GRU kernels).  `PolicyTrainStep` is to the policy what `VOTrainStep` (train.py) is to a VO model:
it holds one flat_params.FlatParams (`store`: ONE flat parameter buffer and ONE flat gradient buffer on the device, the module's
parameters as views of them, Adam's moments and state dict; `flat`, `grad`, `exp_avg`, `exp_avg_sq`, `offsets` are the store's own
objects) and drives the C ABI —

    pnvo_policy_evaluate     rollout forward (encoder in train mode, LSTM or GRU over T x N with mask resets), activations kept
                             (pnvo_policy_evaluate_rgbd for rgb / rgb-d / normalised policies: in training mode the minibatch is
                             merged into RunningMeanAndVar's buffers first; they are buffers — no gradient, no Adam moments)
    pnvo_policy_ppo_loss     clipped surrogate / value loss / entropy and their gradient at the heads, from a kernel
    pnvo_policy_backward     heads, back-propagation through time, embeddings, the encoder's backward
    pnvo_policy_clip_grad_norm, pnvo_adam_step, pnvo_policy_train_refresh

— with no torch autograd anywhere.  `PPO` keeps the reference agent's constructor and `update(rollouts)` contract, so a trainer's
`self.agent.update(rollouts)` works; the loop over `rollouts.recurrent_generator` stays in Python and the loss sums stay on the device
until the end (one synchronisation per update).  The gradient is one flat buffer; the data-parallel agent is ddppo.DDPPO (the
reference's DecentralizedDistributedMixin in front of this PPO: its all-reduce rides on the ranges pnvo_policy_backward reports through
pnvo_policy_set_grad_hook, between `backward()` and `optimizer_step()`, and the division by the world size is folded into the clipping).

`rollouts` is rollout_storage.RolloutStorage (the reference's class on the device: insert, compute_returns and the minibatch gather
are one launch each); the agent reads only `returns`, `value_preds` and `recurrent_generator`.

A policy on another backbone than resnet18 (resnet50 .. se_resneXt101) trains with a FROZEN encoder only (RL.DDPPO.train_encoder:
False, the setting the distributed DD-PPO encoders come with): evaluate_actions on frames is net.visual_encoder's inference forward
followed by the visual_features path, and train_encoder=True is refused before anything is launched.

`BaselineTrainStep` is the same surface for baseline_policy.PointNavBaselinePolicy (the policy of the reference's plain PPOTrainer) on
pnvo_baseline_evaluate / _ppo_loss / _backward; `PPO` picks it by the policy's class.

Not here: the DD-PPO trainer and its pre-emption logic, an autograd bridge for the reference's own PPO.update, the encoder's backward
for Bottleneck / ResNeXt / SE policies.  No CPU fallback.
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from .flat_params import FlatParams, flat_offsets  # noqa: F401  (flat_offsets: the layout rule, public here too)
from .policy import GOAL_SENSOR, _Frames

EPS_PPO = 1e-5
ENCODER_PREFIX = "net.visual_encoder."


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _AdamView:
    """What a trainer reads of `agent.optimizer`: param_groups[0]['lr'] (read at every step), state_dict / load_state_dict."""

    def __init__(self, step):
        self._step = step
        self.param_groups = [{"lr": step.lr, "eps": step.eps, "betas": tuple(step.betas), "weight_decay": 0, "amsgrad": False}]

    def state_dict(self):
        return self._step.state_dict()

    def load_state_dict(self, sd):
        self._step.load_state_dict(sd)
        self.param_groups[0].update(lr=self._step.lr, eps=self._step.eps, betas=tuple(self._step.betas))

    def zero_grad(self, set_to_none=False):
        pass                                               # pnvo_policy_backward overwrites the gradient buffer


class PolicyTrainStep:
    _abi = "pnvo_policy_"                                   # prefix of the library's update-step entry points for this kind of policy

    def _fn(self, name):
        return getattr(_lib.lib, self._abi + name)

    def _attach(self):
        """-> (the library's attach, floats it wants behind the parameters: the encoder handle's padded stem and unused head)"""
        return _lib.lib.pnvo_policy_train_attach, int(_lib.lib.pnvo_policy_train_tail_floats(self.policy._handle))

    def _encoder_range(self):
        """Flat range [lo, hi) of net.visual_encoder's parameters; None when the policy has none (a blind baseline policy)."""
        enc = [self.offsets[n] for n, _ in self.store.named if n.startswith(ENCODER_PREFIX)]
        return (min(o for o, _ in enc), max(o + k for o, k in enc)) if enc else None

    def __init__(self, policy, lr=2.5e-4, eps=1e-5, max_grad_norm=0.5, train_encoder=True, betas=(0.9, 0.999)):
        self.policy = policy
        self.lr, self.eps, self.betas = float(lr), float(eps), tuple(betas)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.train_encoder = bool(train_encoder)
        self._frozen_backbone = getattr(policy, "_backbone", "resnet18") != "resnet18"
        if self._frozen_backbone and self.train_encoder:
            raise NotImplementedError(f"backbone {policy._backbone!r}: the encoder's backward exists for resnet18 only; train this policy "
                                      "with a frozen encoder (RL.DDPPO.train_encoder: False — no parameter of net.visual_encoder with "
                                      "requires_grad, or PolicyTrainStep(..., train_encoder=False))")
        ref = next(policy.parameters())
        if ref.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs on an MI355X only: move the policy with .to('cuda') first "
                               "(there is no CPU fallback)")
        self.dev = ref.device
        policy._ensure(self.dev)                                # handle + kernel operand buffers
        attach, tail = self._attach()
        self.store = FlatParams(list(policy.named_parameters()), self.dev, align=4, tail=tail)     # every tensor at a multiple of 4 floats
        self.flat, self.grad, self.exp_avg, self.exp_avg_sq = (self.store.flat, self.store.grad, self.store.exp_avg,
                                                               self.store.exp_avg_sq)
        self.offsets, self.n_params = self.store.offsets, self.store.n_params
        self.encoder_range = self._encoder_range()
        torch.cuda.synchronize(self.dev)
        with torch.cuda.device(self.dev):
            _lib.check(attach(policy._handle, _ptr(self.flat), _ptr(self.grad), self.flat.numel(), self.store.toc, len(self.store.named)))
        self.step_count = 0
        self._from_features = False                             # the last evaluate_actions took observations['visual_features']
        self._out3 = torch.zeros(3, device=self.dev, dtype=torch.float32)
        self._norm = torch.zeros(1, device=self.dev, dtype=torch.float32)
        policy._train_step = self                               # evaluate_actions delegates here; act reads the flat buffer

    # ------------------------------------------------------------------ parameter / optimizer state
    def _trainable(self):
        return [n for n, _ in self.store.named if self.train_encoder or not n.startswith(ENCODER_PREFIX)]

    def _ranges(self):
        """Flat ranges the optimiser steps over: everything, or everything but net.visual_encoder (the reference's _static_encoder).
        They end with the last parameter, not at n_params: the library's tail starts right behind the last parameter, inside the final
        alignment gap, and a copy the refresh rewrites must not collect Adam moments that no checkpoint carries."""
        end = max(o + k for o, k in self.offsets.values())
        # after an evaluate_actions from visual_features no encoder parameter has a gradient, whatever train_encoder says: the reference's
        # have `grad is None` there and torch's Adam skips them (no step, no moment update)
        if (self.train_encoder and not self._from_features) or self.encoder_range is None:
            return [(0, end)]
        lo, hi = self.encoder_range
        return [(a, b) for a, b in ((0, lo), (hi, end)) if b > a]

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def _sync_params(self):
        """Parameters edited outside the HIP Adam step (load_state_dict on resume, an in-place torch edit) land in the flat buffer but
        not in the encoder's packed operands: re-alias what was re-pointed and re-pack."""
        if not self.store.changed():
            return
        self.store.realias()
        self._repack()

    def _repack(self):
        """The kernel operands (the padded stem, the encoder's packed weights) from the flat buffer as it is now."""
        with torch.cuda.device(self.dev):
            if self._frozen_backbone:                          # the encoder keeps its own copy of the weights: re-read it from the flat buffer
                _lib.check(_lib.lib.pnvo_policy_train_reload_encoder(self.policy._handle, self.store.toc, len(self.store.named),
                                                                     self._stream()))
            for _ in range(3):                                 # three: flat_params.py, "The owner's part"
                _lib.check(self._fn("train_refresh")(self.policy._handle, self._stream()))
        torch.cuda.current_stream(self.dev).synchronize()
        self.store.mark()

    def state_dict(self):
        """Optimizer state in torch.optim.Adam's layout over the trainable parameters, in order (what the reference's
        optim.Adam(filter(requires_grad, actor_critic.parameters())) checkpoints)."""
        return self.store.adam_state_dict(self._trainable(), self.step_count, self.lr, self.betas, self.eps)

    def load_state_dict(self, sd):
        self.step_count, group = self.store.load_adam_state_dict(sd, self._trainable())
        self.lr, self.eps, self.betas = float(group["lr"]), float(group["eps"]), tuple(group["betas"])

    # ------------------------------------------------------------------ the update, piece by piece
    def evaluate_actions(self, observations, rnn_hidden_states, prev_actions, masks, action):
        """-> (value [M,1], action_log_probs [M,1], distribution_entropy (scalar), rnn_hidden_states) as Policy.evaluate_actions
        (policy.py:52-63).  Rows are T-major (row t*N + n); N = rnn_hidden_states.shape[1], T = M / N (T = 1: single_forward)."""
        pol, dev = self.policy, self.dev
        # visual_features when present, else the frames (and, in training mode, RunningMeanAndVar's buffers, which this call updates
        # before it whitens: once per minibatch, as the reference's evaluate_actions does); checked before any launch
        vis, from_features = pol._visual_input(observations, dev)
        self._sync_params()
        if self._frozen_backbone and not from_features:
            # no training forward for this encoder, and none needed: frozen, its output is what the inference forward gives (in training
            # mode RunningMeanAndVar merges the minibatch first, once, as the reference's evaluate_actions does)
            vis, from_features = pol._encode(observations), True
        M = vis.shape[0]
        hin = rnn_hidden_states.to(device=dev, dtype=torch.float32).contiguous()
        N = hin.shape[1]
        S = pol.num_recurrent_layers
        if tuple(hin.shape) != (S, N, pol._hidden) or N <= 0 or M % N != 0:
            raise ValueError(f"rnn_hidden_states {tuple(hin.shape)} does not fit {M} rows: expected [{S}, N, {pol._hidden}] "
                             "with N dividing the number of rows")
        T = M // N
        goal = observations[GOAL_SENSOR].to(device=dev, dtype=torch.float32).contiguous().reshape(M, 2)
        pa = prev_actions.to(device=dev, dtype=torch.int64).contiguous().reshape(M)
        mk = masks.to(device=dev, dtype=torch.float32).contiguous().reshape(M)
        act = action.to(device=dev, dtype=torch.int64).contiguous().reshape(M)
        hout = torch.empty_like(hin)
        value = torch.empty((M, 1), device=dev, dtype=torch.float32)
        logp = torch.empty((M, 1), device=dev, dtype=torch.float32)
        entropy = torch.empty((), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            if from_features:
                _lib.check(_lib.lib.pnvo_policy_evaluate_features(pol._handle, _ptr(vis), _ptr(goal), _ptr(pa), _ptr(mk), _ptr(hin), int(T),
                                                                  int(N), _ptr(act), _ptr(hout), _ptr(value), _ptr(logp), _ptr(entropy),
                                                                  self._stream()))
            elif isinstance(vis, _Frames):
                _lib.check(_lib.lib.pnvo_policy_evaluate_rgbd(pol._handle, *vis.args(), _ptr(goal), _ptr(pa), _ptr(mk), _ptr(hin), int(T),
                                                              int(N), _ptr(act), int(self.train_encoder), _ptr(hout), _ptr(value),
                                                              _ptr(logp), _ptr(entropy), self._stream()))
            else:
                _lib.check(_lib.lib.pnvo_policy_evaluate(pol._handle, _ptr(vis), _ptr(goal), _ptr(pa), _ptr(mk), _ptr(hin), int(T), int(N),
                                                         _ptr(act), int(self.train_encoder), _ptr(hout), _ptr(value), _ptr(logp),
                                                         _ptr(entropy), self._stream()))
        self._from_features = from_features
        return value, logp, entropy, hout

    def ppo_loss(self, old_action_log_probs, adv_targ, value_preds, returns, clip_param, value_loss_coef, entropy_coef,
                 use_clipped_value_loss=True):
        """The minibatch loss of rl/ppo/ppo.py:101-126 for the last evaluate_actions -> device tensor [3] = (value_loss, action_loss,
        dist_entropy); its gradient at the heads stays in the handle for backward().  The tensor is reused by the next call."""
        f = lambda t: None if t is None else t.to(device=self.dev, dtype=torch.float32).contiguous().reshape(-1)
        old, adv, vp, ret = f(old_action_log_probs), f(adv_targ), f(value_preds), f(returns)
        with torch.cuda.device(self.dev):
            _lib.check(self._fn("ppo_loss")(self.policy._handle, _ptr(old), _ptr(adv), _ptr(vp), _ptr(ret), float(clip_param),
                                            float(value_loss_coef), float(entropy_coef), int(bool(use_clipped_value_loss)),
                                            _ptr(self._out3), self._stream()))
        return self._out3

    def backward(self):
        """total_loss.backward(): fills self.grad (overwrites).  After an evaluate_actions from visual_features the encoder's range is
        exactly zero, whatever train_encoder says (the library knows which kind of evaluate came last); with train_encoder False it
        stays exactly zero too."""
        with torch.cuda.device(self.dev):
            _lib.check(self._fn("backward")(self.policy._handle, int(self.train_encoder), self._stream()))

    def clip_grad_norm(self):
        """nn.utils.clip_grad_norm_(parameters, max_grad_norm) on the device -> the norm as a device tensor [1] (no host sync)."""
        if self.max_grad_norm is None:
            return None
        with torch.cuda.device(self.dev):
            _lib.check(self._fn("clip_grad_norm")(self.policy._handle, float(self.max_grad_norm), _ptr(self._norm), self._stream()))
        return self._norm

    def timing(self, on=True):
        """Record HIP events at the phase boundaries of the update (tools/bench_ppo_update.py)."""
        _lib.check(self._fn("train_timing")(self.policy._handle, int(bool(on))))

    def phase_ms(self):
        """Milliseconds of the last evaluate_actions / ppo_loss / backward (waits for the backward): encoder forward, LSTM (or GRU) forward +
        heads, loss, heads + BPTT + embedding backward, encoder backward."""
        ms = (C.c_double * 5)()
        _lib.check(self._fn("train_timing_read")(self.policy._handle, ms))
        return dict(zip(("encoder_forward", "lstm_forward", "loss", "bptt", "encoder_backward"), (float(v) for v in ms)))

    def optimizer_step(self):
        """Adam over the trainable ranges, then the encoder's operands are re-packed from the flat buffer."""
        self.step_count += 1
        with torch.cuda.device(self.dev):
            stream = self._stream()
            self.store.adam_step(self._ranges(), self.lr, self.betas, self.eps, self.step_count, stream)
            _lib.check(self._fn("train_refresh")(self.policy._handle, stream))


class BaselineTrainStep(PolicyTrainStep):
    """PolicyTrainStep's public surface for baseline_policy.PointNavBaselinePolicy (pnvo_baseline_train_* / _evaluate / _ppo_loss /
    _backward / _clip_grad_norm): the same flat store, Adam and optimizer state dict; the parameters stay in torch's layouts in `flat`
    and the gradients land in `grad` in torch's layouts, the handle re-lays its kernel operands from `flat` on the device after every
    optimiser step (pnvo_baseline_train_refresh).  float32 frames-in only: no visual_features input, no bf16."""

    _abi = "pnvo_baseline_"

    def _attach(self):
        return _lib.lib.pnvo_baseline_train_attach, 0

    def _repack(self):
        """The handle's kernel-layout operands from the flat buffer as it is now (one pass is all: nothing here lags a refresh)."""
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib.pnvo_baseline_train_refresh(self.policy._handle, self._stream()))
        torch.cuda.current_stream(self.dev).synchronize()
        self.store.mark()

    def evaluate_actions(self, observations, rnn_hidden_states, prev_actions, masks, action):
        """-> (value [M,1], action_log_probs [M,1], distribution_entropy (scalar), rnn_hidden_states [1,N,hidden]) as
        Policy.evaluate_actions (policy.py:52-63).  Rows are T-major (row t*N + n); N = rnn_hidden_states.shape[1], T = M / N.
        prev_actions is accepted and ignored, as in the reference's net."""
        pol, dev = self.policy, self.dev
        rgb, u8, depth, M = pol._frames(observations, dev)      # checked before any launch
        goal = observations[pol.goal_sensor_uuid].to(device=dev, dtype=torch.float32).contiguous()
        if M is None:
            M = int(goal.shape[0])
        goal = goal.reshape(M, pol._goal_dim)
        self._sync_params()
        hin = rnn_hidden_states.to(device=dev, dtype=torch.float32).contiguous()
        N = hin.shape[1] if hin.dim() == 3 else 0
        if tuple(hin.shape) != (1, N, pol._hidden) or N <= 0 or M % N != 0:
            raise ValueError(f"rnn_hidden_states {tuple(hin.shape)} does not fit {M} rows: expected [1, N, {pol._hidden}] "
                             "with N dividing the number of rows")
        T = M // N
        mk = masks.to(device=dev, dtype=torch.float32).contiguous().reshape(M)
        act = action.to(device=dev, dtype=torch.int64).contiguous().reshape(M)
        hout = torch.empty_like(hin)
        value = torch.empty((M, 1), device=dev, dtype=torch.float32)
        logp = torch.empty((M, 1), device=dev, dtype=torch.float32)
        entropy = torch.empty((), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.pnvo_baseline_evaluate(pol._handle, _ptr(rgb), u8, _ptr(depth), _ptr(goal), _ptr(mk), _ptr(hin), int(T),
                                                       int(N), _ptr(act), _ptr(hout), _ptr(value), _ptr(logp), _ptr(entropy),
                                                       self._stream()))
        return value, logp, entropy, hout


class PPO(nn.Module):
    """The reference agent's contract (rl/ppo/ppo.py): same constructor keywords, get_advantages, update -> three floats."""

    def __init__(self, actor_critic, clip_param, ppo_epoch, num_mini_batch, value_loss_coef, entropy_coef, lr=None, eps=None,
                 max_grad_norm=None, use_clipped_value_loss=True, use_normalized_advantage=True):
        super().__init__()
        self.actor_critic = actor_critic
        self.clip_param = clip_param
        self.ppo_epoch = ppo_epoch
        self.num_mini_batch = num_mini_batch
        self.value_loss_coef = value_loss_coef
        self.entropy_coef = entropy_coef
        self.max_grad_norm = max_grad_norm
        self.use_clipped_value_loss = use_clipped_value_loss
        self.use_normalized_advantage = use_normalized_advantage
        # the reference's optimiser takes the parameters with requires_grad: a trainer freezes net.visual_encoder before it builds the agent
        train_encoder = any(p.requires_grad for n, p in actor_critic.named_parameters() if n.startswith(ENCODER_PREFIX))
        kw = {}
        if lr is not None:
            kw["lr"] = lr
        if eps is not None:
            kw["eps"] = eps
        from .baseline_policy import PointNavBaselinePolicy
        step_cls = BaselineTrainStep if isinstance(actor_critic, PointNavBaselinePolicy) else PolicyTrainStep
        self.train_step = step_cls(actor_critic, max_grad_norm=max_grad_norm, train_encoder=train_encoder, **kw)
        self.optimizer = _AdamView(self.train_step)
        self.device = next(actor_critic.parameters()).device

    def forward(self, *x):
        raise NotImplementedError

    def get_advantages(self, rollouts):
        advantages = rollouts.returns[:-1] - rollouts.value_preds[:-1]
        if not self.use_normalized_advantage:
            return advantages
        return (advantages - advantages.mean()) / (advantages.std() + EPS_PPO)

    def update(self, rollouts):
        advantages = self.get_advantages(rollouts)
        step = self.train_step
        sums = torch.zeros(3, device=self.device, dtype=torch.float32)
        for _ in range(self.ppo_epoch):
            for sample in rollouts.recurrent_generator(advantages, self.num_mini_batch):
                (obs_batch, recurrent_hidden_states_batch, actions_batch, prev_actions_batch, value_preds_batch, return_batch,
                 masks_batch, old_action_log_probs_batch, adv_targ) = sample
                step.evaluate_actions(obs_batch, recurrent_hidden_states_batch, prev_actions_batch, masks_batch, actions_batch)
                sums += step.ppo_loss(old_action_log_probs_batch, adv_targ, value_preds_batch, return_batch, self.clip_param,
                                      self.value_loss_coef, self.entropy_coef, self.use_clipped_value_loss)
                self.before_backward(None)
                step.backward()
                self.after_backward(None)
                self.before_step()
                step.lr = float(self.optimizer.param_groups[0]["lr"])
                step.optimizer_step()
                self.after_step()
        value_loss, action_loss, dist_entropy = (sums / (self.ppo_epoch * self.num_mini_batch)).tolist()   # the one synchronisation
        return value_loss, action_loss, dist_entropy

    def before_backward(self, loss):
        pass

    def after_backward(self, loss):
        pass

    def before_step(self):
        self.train_step.clip_grad_norm()

    def after_step(self):
        pass
