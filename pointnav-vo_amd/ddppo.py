"""DD-PPO: the reference's `DDPPO` agent (pointnav_vo/rl/ddppo/algo/ddppo.py) on the HIP update step — `DecentralizedDistributedMixin`
in front of this package's `PPO`, one process per GPU under torch.distributed (backend "nccl" = RCCL on the GPU box, "gloo" in the tests).

`PPO.update` is unchanged; the mixin overrides the four hooks it calls.  What the reference gets from torch's DistributedDataParallel
(`Guard`, `reducer.prepare_for_backward`) is done on the flat buffers instead — there is no DDP wrapper and no `reducer`:

    init_distributed   broadcast of the flat parameter range (one call) and of RunningMeanAndVar's three buffers from rank 0, re-pack of
                       the kernel operands, the distributed `get_advantages`, the gradient-ready hook (pnvo_policy_set_grad_hook) and the
                       policy's opt-in to the statistics reduction (policy.distributed_statistics)
    backward           the library reports each flat gradient range when it is final; its all-reduce (sum) starts on one communication
                       stream (parallel.BucketAllReduce) while the encoder's backward still runs: embeddings + recurrent tensors + heads
                       first, then the encoder and visual_fc, the stem weight last
    after_backward     the launch stream waits for those all-reduces
    before_step        pnvo_policy_clip_grad_norm_scaled with 1 / world_size: the mean over the ranks and clip_grad_norm_ in one pass
                       (max_grad_norm None: the scaling alone)

The sequence and the sizes of the collectives depend on the policy's configuration only (never on T, N or the data), so ranks whose
rollouts ended at different steps stay in step as long as they run the same number of minibatches; ranks with different numbers of
environments, the trainer, its pre-emption store and requeue logic are not here.
"""
import ctypes as C

import torch
import torch.distributed as distrib

from . import _lib
from .parallel import BucketAllReduce
from .ppo import EPS_PPO, PPO, _ptr


def distributed_mean_and_var(values):
    """(mean, variance) of `values` over the copies of ALL workers, as if they were concatenated first (the arithmetic of ddppo.py:18-42):
    the local means are summed and divided by the world size, then the local mean squared deviations from that global mean are — two
    all-reduces of one scalar, the population variance (no Bessel correction).  Every worker holds the same number of values.  Plain
    torch ops: CPU tensors under gloo work as well."""
    assert distrib.is_initialized(), "Distributed must be initialized"
    world = distrib.get_world_size()
    mean = values.mean()
    distrib.all_reduce(mean)
    mean /= world
    var = (values - mean).pow(2).mean()
    distrib.all_reduce(var)
    var /= world
    return mean, var


class DecentralizedDistributedMixin:
    def _get_advantages_distributed(self, rollouts):
        """PPO.get_advantages with the normalisation taken over all workers' rollouts (ddppo.py:46-53)."""
        adv = rollouts.returns[:-1] - rollouts.value_preds[:-1]
        if self.use_normalized_advantage:
            mean, var = distributed_mean_and_var(adv)
            adv = (adv - mean) / (var.sqrt() + EPS_PPO)
        return adv

    def init_distributed(self, find_unused_params=True):
        """1. broadcasts the weights (and the input statistics) from world rank 0; 2. installs the gradient hook; 3. turns on the
        reduction of RunningMeanAndVar's batch moments.  find_unused_params is kept for the reference's signature: the ranges the
        library reports already leave out what has no gradient in a backward."""
        assert distrib.is_initialized(), "Distributed must be initialized"
        step, pol = self.train_step, self.actor_critic
        self.find_unused_params = find_unused_params
        self.world_size = distrib.get_world_size()
        end = max(o + k for o, k in step.offsets.values())
        step._sync_params()                                    # (a load_state_dict before this call is in the flat buffer first)
        torch.cuda.current_stream(step.dev).synchronize()
        distrib.broadcast(step.flat[:end], 0)                  # every parameter in one call (the library's tail is re-derived below)
        if pol._normalize:
            rmv = pol.net.visual_encoder.running_mean_and_var
            for b in (rmv._mean, rmv._var, rmv._count):
                distrib.broadcast(b, 0)
        torch.cuda.current_stream(step.dev).synchronize()
        step._repack()                                         # the padded stem and the packed operands follow the flat buffer
        self.get_advantages = self._get_advantages_distributed
        self.bucketed = True                                   # False: ONE flat all-reduce behind the backward (the A/B of the schedules)
        self._buckets = BucketAllReduce(step.dev)
        self._hook = _lib.GRAD_READY_FN(self._on_grad_ready)
        _lib.check(_lib.lib.pnvo_policy_set_grad_hook(pol._handle, C.cast(self._hook, C.c_void_p), None))
        pol.distributed_statistics(True)

    # ------------------------------------------------------------------ gradient all-reduce
    def _reducing(self):
        return getattr(self, "_buckets", None) is not None and distrib.is_initialized() and distrib.get_world_size() > 1

    def _on_grad_ready(self, user, first, count, stream):
        """pnvo_grad_ready_fn: called by pnvo_policy_backward on the host when a flat gradient range is final."""
        if self.bucketed and self._reducing():
            self._buckets.start(self.train_step.grad, int(first), int(count))

    def grad_ranges(self, train_encoder=None, from_features=None):
        """[(first, count)] the backward reports, in its order, without running one (pnvo_policy_grad_buckets); by default for the
        kind of backward that follows the last evaluate_actions."""
        step = self.train_step
        te = step.train_encoder if train_encoder is None else train_encoder
        ff = step._from_features if from_features is None else from_features
        first, count, n = (C.c_uint64 * 16)(), (C.c_uint64 * 16)(), C.c_int(0)
        _lib.check(_lib.lib.pnvo_policy_grad_buckets(self.actor_critic._handle, int(bool(te)), int(bool(ff)), first, count, 16,
                                                     C.byref(n)))
        return [(int(first[k]), int(count[k])) for k in range(min(n.value, 16))]

    def before_backward(self, loss):
        super().before_backward(loss)

    def after_backward(self, loss):
        super().after_backward(loss)
        if not self._reducing():
            return
        if self.bucketed:
            self._buckets.wait()                               # the launch stream waits for the communication stream
        else:                                                  # the ranges a bucketed backward would have sent, as one span
            r = self.grad_ranges()
            lo, hi = min(f for f, _ in r), max(f + c for f, c in r)
            distrib.all_reduce(self.train_step.grad[lo:hi])

    def before_step(self):
        """The mean over the ranks and nn.utils.clip_grad_norm_ in one pass over the gradient."""
        if getattr(self, "_buckets", None) is None:            # init_distributed was not called: the single-process agent
            return super().before_step()
        step = self.train_step
        world = distrib.get_world_size()
        if world == 1 and step.max_grad_norm is None:
            return None
        with torch.cuda.device(step.dev):
            _lib.check(_lib.lib.pnvo_policy_clip_grad_norm_scaled(self.actor_critic._handle, 1.0 / world, float(step.max_grad_norm or 0.0),
                                                                  _ptr(step._norm), step._stream()))
        return step._norm


class DDPPO(DecentralizedDistributedMixin, PPO):
    def __init__(self, actor_critic, *args, **kwargs):
        from .baseline_policy import PointNavBaselinePolicy
        if isinstance(actor_critic, PointNavBaselinePolicy):   # before anything is attached or launched
            raise NotImplementedError("DDPPO on a PointNavBaselinePolicy: the data-parallel update (gradient-ready ranges, the all-reduce "
                                      "schedule) is built for PointNavResNetPolicy only, as the reference's DD-PPO trainer never builds "
                                      "the baseline policy; use ppo.PPO")
        super().__init__(actor_critic, *args, **kwargs)
