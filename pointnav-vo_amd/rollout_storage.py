"""RolloutStorage on the device: the reference's class (pointnav_vo/rl/common/rollout_storage.py) on libpnvo.so.

The object between `PointNavResNetPolicy.act` (policy.py) and `PPO.update` (ppo.py): a trainer inserts one simulator step at a
time, computes the returns once per rollout and hands the storage to the agent, which draws recurrent minibatches from it.  The
attributes are the reference's — plain torch tensors with its names, shapes and dtypes, so `rollouts.observations[s][0].copy_(...)`
and `rollouts.masks[rollouts.step]` work as before — and each method is one launch of a kernel of csrc/rollout.hip over the small
fields instead of a chain of tiny torch ops:

    insert               pnvo_rollout_insert (seven fields, one launch) + one device copy per stored sensor
    after_update         pnvo_rollout_after_update + one device copy per stored sensor
    compute_returns      pnvo_rollout_compute_returns (either branch, one launch; float32 in the reference's operation order)
    recurrent_generator  torch.randperm(num_envs) from the CPU default generator once per call, uploaded once; per minibatch
                         pnvo_rollout_gather (eight small fields) + pnvo_rollout_gather_frames per stored sensor

No method waits for the device.  One extension: `sensors=` keeps only the named sensors (the HIP policy reads `depth` and the goal
sensor; the reference would also hold `rgb` as float32 for num_steps + 1 steps).  Discrete action spaces only.  No CPU fallback:
the four methods raise RuntimeError on CPU-resident storage — build it, then `.to('cuda')`.
"""
import ctypes as C

import torch

from . import _lib


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class RolloutStorage:
    r"""Class for storing rollout information for RL trainers."""

    def __init__(self, num_steps, num_envs, observation_space, action_space, recurrent_hidden_state_size, num_recurrent_layers=1, *,
                 sensors=None):
        if action_space.__class__.__name__ != "ActionSpace":
            raise NotImplementedError(f"RolloutStorage stores discrete actions (an ActionSpace) only, got {action_space.__class__.__name__}: "
                                      "continuous action spaces are not built")
        if num_steps < 1 or num_envs < 1 or recurrent_hidden_state_size < 1 or num_recurrent_layers < 1:
            raise ValueError("num_steps, num_envs, recurrent_hidden_state_size and num_recurrent_layers must be positive")
        if sensors is not None:
            missing = [s for s in sensors if s not in observation_space.spaces]
            if missing:
                raise KeyError(f"sensors {missing} are not in the observation space {list(observation_space.spaces)}")
        self.observations = {}
        for sensor in observation_space.spaces:
            if sensors is None or sensor in sensors:
                self.observations[sensor] = torch.zeros(num_steps + 1, num_envs, *observation_space.spaces[sensor].shape)
        self.recurrent_hidden_states = torch.zeros(num_steps + 1, num_recurrent_layers, num_envs, recurrent_hidden_state_size)
        self.rewards = torch.zeros(num_steps, num_envs, 1)
        self.value_preds = torch.zeros(num_steps + 1, num_envs, 1)
        self.returns = torch.zeros(num_steps + 1, num_envs, 1)
        self.action_log_probs = torch.zeros(num_steps, num_envs, 1)
        self.actions = torch.zeros(num_steps, num_envs, 1, dtype=torch.int64)
        self.prev_actions = torch.zeros(num_steps + 1, num_envs, 1, dtype=torch.int64)
        self.masks = torch.zeros(num_steps + 1, num_envs, 1)
        self.num_steps = num_steps
        self.step = 0

    _FIELDS = ("recurrent_hidden_states", "rewards", "value_preds", "returns", "action_log_probs", "actions", "prev_actions", "masks")

    def to(self, device):
        for sensor in self.observations:
            self.observations[sensor] = self.observations[sensor].to(device)
        for name in self._FIELDS:
            setattr(self, name, getattr(self, name).to(device))

    # ------------------------------------------------------------------ helpers
    def _device(self, what):
        dev = self.rewards.device
        if dev.type != "cuda":
            raise RuntimeError(f"RolloutStorage.{what} runs on an MI355X only: move the storage with .to('cuda') first "
                               "(there is no CPU fallback)")
        T, N = self.num_steps, self.recurrent_hidden_states.shape[2]
        rows = {"recurrent_hidden_states": T + 1, "rewards": T, "value_preds": T + 1, "returns": T + 1, "action_log_probs": T,
                "actions": T, "prev_actions": T + 1, "masks": T + 1}
        for name in self._FIELDS:
            t = getattr(self, name)
            dtype = torch.int64 if name in ("actions", "prev_actions") else torch.float32
            shape_ok = t.shape[0] == rows[name] and (name == "recurrent_hidden_states" or tuple(t.shape[1:]) == (N, 1))
            if t.device != dev or not t.is_contiguous() or t.dtype != dtype or not shape_ok:
                raise RuntimeError(f"RolloutStorage.{name} was replaced by a tensor the kernels cannot take ({tuple(t.shape)}, {t.dtype}, "
                                   f"{t.device}): every field must keep its shape and dtype, contiguous on {dev}")
        return dev

    def _dims(self):
        _, L, N, H = self.recurrent_hidden_states.shape
        return int(N), int(L), int(H)

    @staticmethod
    def _stream(dev):
        return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    # ------------------------------------------------------------------ the reference's methods
    def insert(self, observations, recurrent_hidden_states, actions, action_log_probs, value_preds, rewards, masks):
        dev = self._device("insert")
        N, L, H = self._dims()
        if not 0 <= self.step < self.num_steps:
            raise IndexError(f"insert at step {self.step} of a storage of {self.num_steps} steps: call after_update() first")
        f32 = lambda t, n, what: self._row(t, dev, torch.float32, n, what)
        hid = f32(recurrent_hidden_states, L * N * H, "recurrent_hidden_states")
        act = self._row(actions, dev, torch.int64, N, "actions")
        small = {"action_log_probs": action_log_probs, "value_preds": value_preds, "rewards": rewards, "masks": masks}
        small = {k: torch.as_tensor(t) for k, t in small.items()}
        on_host = [k for k, t in small.items() if t.device.type == "cpu" and t.numel() == N]
        if len(on_host) > 1:                                    # the trainers build rewards and masks on the host: one upload for both
            packed = torch.stack([small[k].to(torch.float32).reshape(N) for k in on_host]).to(dev)
            small.update((k, packed[i]) for i, k in enumerate(on_host))
        logp, val, rew, msk = (f32(t, N, k) for k, t in small.items())
        for sensor in observations:
            if sensor in self.observations:
                self.observations[sensor][self.step + 1].copy_(observations[sensor], non_blocking=True)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.pnvo_rollout_insert(
                _ptr(self.recurrent_hidden_states), _ptr(self.actions), _ptr(self.prev_actions), _ptr(self.action_log_probs),
                _ptr(self.value_preds), _ptr(self.rewards), _ptr(self.masks), self.num_steps, N, L * N * H, self.step,
                _ptr(hid), _ptr(act), _ptr(logp), _ptr(val), _ptr(rew), _ptr(msk), self._stream(dev)))
        self.step = self.step + 1

    @staticmethod
    def _row(t, dev, dtype, numel, what):
        """One step's input as the kernel reads it: on the device, `dtype`, contiguous (inputs may sit on the host, be strided or of
        another dtype, as ppo.py normalises its own)."""
        t = torch.as_tensor(t).to(device=dev, dtype=dtype).contiguous()
        if t.numel() != numel:
            raise ValueError(f"{what} has {t.numel()} elements (shape {tuple(t.shape)}), the storage holds {numel} per step")
        return t

    def after_update(self):
        dev = self._device("after_update")
        N, L, H = self._dims()
        if not 0 <= self.step <= self.num_steps:
            raise IndexError(f"step {self.step} outside a storage of {self.num_steps} steps")
        if self.step > 0:
            for sensor in self.observations:
                self.observations[sensor][0].copy_(self.observations[sensor][self.step])
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.pnvo_rollout_after_update(_ptr(self.recurrent_hidden_states), _ptr(self.prev_actions), _ptr(self.masks),
                                                          self.num_steps, N, L * N * H, self.step, self._stream(dev)))
        self.step = 0

    def compute_returns(self, next_value, use_gae, gamma, tau):
        dev = self._device("compute_returns")
        N, _, _ = self._dims()
        if not 0 <= self.step <= self.num_steps:
            raise IndexError(f"step {self.step} outside a storage of {self.num_steps} steps")
        nv = self._row(next_value, dev, torch.float32, N, "next_value")
        # the reference multiplies float32 tensors by the Python doubles gamma and gamma * tau: each is rounded to float32 once
        # (ctypes does that rounding for a c_float argument)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.pnvo_rollout_compute_returns(_ptr(self.rewards), _ptr(self.value_preds), _ptr(self.masks),
                                                             _ptr(self.returns), _ptr(nv), self.num_steps, N, self.step,
                                                             int(bool(use_gae)), float(gamma), float(gamma) * float(tau),
                                                             self._stream(dev)))

    def recurrent_generator(self, advantages, num_mini_batch):
        dev = self._device("recurrent_generator")
        num_processes = self.rewards.size(1)
        assert num_processes >= num_mini_batch, (
            "Trainer requires the number of processes ({}) "
            "to be greater than or equal to the number of "
            "trainer mini batches ({}).".format(num_processes, num_mini_batch)
        )
        if num_processes % num_mini_batch != 0:
            raise ValueError(f"the number of processes ({num_processes}) is not a multiple of the number of trainer mini batches "
                             f"({num_mini_batch}): the reference would index past its permutation")
        steps = self.step
        if not 1 <= steps <= self.num_steps:
            raise ValueError(f"recurrent_generator at step {steps}: it needs between 1 and {self.num_steps} inserted steps")
        adv = torch.as_tensor(advantages).to(device=dev, dtype=torch.float32).contiguous()
        if adv.dim() < 2 or adv.shape[0] < steps or adv.shape[1] != num_processes or adv.numel() != adv.shape[0] * num_processes:
            raise ValueError(f"advantages has shape {tuple(adv.shape)}, expected [>= {steps}, {num_processes}, 1]")
        return self._minibatches(dev, adv, steps, num_processes // num_mini_batch)

    def _minibatches(self, dev, adv, steps, n_mb):
        N, L, H = self._dims()
        perm = torch.randperm(N)                                # the CPU default generator, once per call, as the reference
        if perm.dtype != torch.int64 or int(perm.min()) < 0 or int(perm.max()) >= N:      # host tensor: no device wait
            raise RuntimeError("torch.randperm returned indices outside the environments")
        perm_dev = perm.to(dev)                                 # one upload per call
        M = steps * n_mb
        f32 = lambda: torch.empty((M, 1), device=dev, dtype=torch.float32)
        i64 = lambda: torch.empty((M, 1), device=dev, dtype=torch.int64)
        for start in range(0, N, n_mb):
            with torch.cuda.device(dev):                        # per minibatch: not held while the generator is suspended
                stream = self._stream(dev)
                obs = {}
                for sensor, frames in self.observations.items():
                    if (frames.device != dev or not frames.is_contiguous() or frames.dtype != torch.float32 or frames.dim() < 2
                            or frames.shape[0] < steps or frames.shape[1] != N):
                        raise RuntimeError(f"RolloutStorage.observations[{sensor!r}] must be a contiguous float32 "
                                           f"[>= {steps}, {N}, ...] tensor on {dev}")
                    shape = tuple(frames.shape[2:])
                    out = torch.empty((M,) + shape, device=dev, dtype=torch.float32)
                    F = 1
                    for s in shape:
                        F *= int(s)
                    if F > 0:
                        _lib.check(_lib.lib.pnvo_rollout_gather_frames(_ptr(frames), _ptr(perm_dev), N, F, steps, start, n_mb, _ptr(out),
                                                                       stream))
                    obs[sensor] = out
                hidden = torch.empty((L, n_mb, H), device=dev, dtype=torch.float32)
                actions, prev_actions = i64(), i64()
                value_preds, returns, masks, logp, adv_targ = f32(), f32(), f32(), f32(), f32()
                _lib.check(_lib.lib.pnvo_rollout_gather(
                    _ptr(self.recurrent_hidden_states), _ptr(self.actions), _ptr(self.prev_actions), _ptr(self.value_preds),
                    _ptr(self.returns), _ptr(self.masks), _ptr(self.action_log_probs), _ptr(adv), _ptr(perm_dev), N, L, H, steps, start,
                    n_mb, _ptr(hidden), _ptr(actions), _ptr(prev_actions), _ptr(value_preds), _ptr(returns), _ptr(masks), _ptr(logp),
                    _ptr(adv_targ), stream))
            yield (obs, hidden, actions, prev_actions, value_preds, returns, masks, logp, adv_targ)

    @staticmethod
    def _flatten_helper(t: int, n: int, tensor: torch.Tensor) -> torch.Tensor:
        r"""Given a tensor of size (t, n, ..), flatten it to size (t*n, ...)."""
        return tensor.view(t * n, *tensor.size()[2:]).contiguous()
