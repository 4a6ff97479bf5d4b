"""CPU: the host side of the data-parallel PPO agent (pointnav_vo_amd.ddppo), without a device.

  - distributed_mean_and_var under a two-process gloo group on CPU tensors equals numpy's population mean and variance of the
    concatenation, and _get_advantages_distributed normalises with them;
  - DDPPO is a PPO with the mixin first in the MRO; init_distributed without a process group fails with the reference's assertion;
  - a normalising policy in training mode under a process group is still refused unless it opted in (distributed_statistics), and one
    that did hands the library its statistics with training = 1.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from pointnav_vo_amd.ddppo import DDPPO, DecentralizedDistributedMixin, distributed_mean_and_var
from pointnav_vo_amd.policy import PointNavResNetPolicy
from pointnav_vo_amd.ppo import EPS_PPO, PPO

GOAL = "pointgoal_with_gps_compass"
CPU = torch.device("cpu")
T, N = 5, 3                                              # 15 values per rank


def rank_values(rank):
    """Advantage-like values of a rank: another offset and spread per rank, so that the global mean is neither rank's own."""
    g = np.random.default_rng(100 + rank)
    ret = g.normal(loc=0.5 + 2.0 * rank, scale=1.0 + rank, size=(T + 1, N, 1)).astype(np.float32)
    vp = g.normal(loc=0.1, scale=0.5, size=(T + 1, N, 1)).astype(np.float32)
    return ret, vp


class _Rollouts:
    def __init__(self, ret, vp):
        self.returns, self.value_preds = torch.from_numpy(ret), torch.from_numpy(vp)


class _Agent(DecentralizedDistributedMixin):
    use_normalized_advantage = True


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ret, vp = rank_values(rank)
    adv = torch.from_numpy(ret[:-1] - vp[:-1])
    mean, var = distributed_mean_and_var(adv)
    norm = _Agent()._get_advantages_distributed(_Rollouts(ret, vp))
    agent = _Agent()
    agent.use_normalized_advantage = False
    raw = agent._get_advantages_distributed(_Rollouts(ret, vp))
    q.put((rank, float(mean), float(var), norm.numpy(), raw.numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_distributed_mean_and_var_equal_numpy_on_the_concatenation():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r[0], r[1:]) for r in (q.get(), q.get()))
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    advs32 = [rank_values(r)[0][:-1] - rank_values(r)[1][:-1] for r in range(2)]       # float32, as each rank forms them
    both = np.concatenate([a.astype(np.float64) for a in advs32])
    mean, var = both.mean(), both.var()                  # population variance (ddof = 0)
    eps = 2.0 ** -24
    n = both.size // 2
    # float32: each rank's mean of n values (pairwise sum: log2(n) + 1 roundings and the division), the sum of two and the division by
    # the world size — (log2(n) + 4) half-ulps of the largest |value|; the variance likewise on squared deviations, plus twice the
    # mean's error times the largest deviation
    k = np.log2(n) + 4
    tol_mean = k * eps * np.abs(both).max()
    dev = np.abs(both - mean).max()
    tol_var = (k + 2) * eps * dev ** 2 + 2 * tol_mean * dev
    for rank in range(2):
        m, v, norm, raw = got[rank]
        assert (m, v) == got[0][:2]                      # both ranks hold the same pair
        assert abs(m - mean) <= tol_mean, (m, mean, tol_mean)
        assert abs(v - var) <= tol_var, (v, var, tol_var)
        np.testing.assert_array_equal(raw, advs32[rank])                          # use_normalized_advantage False: untouched
        want = (advs32[rank].astype(np.float64) - mean) / (np.sqrt(var) + EPS_PPO)
        # (a - mean) / (std + eps): the errors of mean and std above, and three float32 roundings of the result
        std = np.sqrt(var)
        tol = (tol_mean + dev * (tol_var / (2 * var))) / std + 3 * eps * np.abs(want).max()
        assert np.abs(norm.astype(np.float64) - want).max() <= tol, (np.abs(norm - want).max(), tol)


def test_ddppo_is_the_mixin_in_front_of_ppo():
    mro = DDPPO.__mro__
    assert issubclass(DDPPO, PPO) and mro[0] is DDPPO and mro[1] is DecentralizedDistributedMixin and mro[2] is PPO
    for name in ("before_backward", "after_backward", "before_step", "init_distributed", "_get_advantages_distributed"):
        assert name in DecentralizedDistributedMixin.__dict__, name
    assert "update" not in DecentralizedDistributedMixin.__dict__ and DDPPO.update is PPO.update
    assert not dist.is_initialized()
    agent = object.__new__(DDPPO)                        # (a PPO needs a device; the assertion comes before anything is touched)
    with pytest.raises(AssertionError, match="Distributed must be initialized"):
        agent.init_distributed()
    with pytest.raises(AssertionError, match="Distributed must be initialized"):
        distributed_mean_and_var(torch.zeros(3))


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class Act:
    def __init__(self, n):
        self.n = n


def make_policy(normalize=True, h=96, w=128):
    space = Space({"depth": Box((h, w, 1)), "rgb": Box((h, w, 3)), GOAL: Box((2,))})
    return PointNavResNetPolicy(observation_space=space, action_space=Act(4), hidden_size=128, num_recurrent_layers=2,
                                backbone="resnet18", goal_sensor_uuid=GOAL, normalize_visual_inputs=normalize, obs_transform=None,
                                vis_types=["rgb", "depth"])


def test_statistics_reduction_is_an_opt_in(tmp_path):
    pol, opted = make_policy(), make_policy()
    obs = {GOAL: torch.zeros(2, 2), "rgb": torch.zeros(2, 96, 128, 3, dtype=torch.uint8), "depth": torch.zeros(2, 96, 128, 1)}
    assert opted.distributed_statistics(True) is opted and opted._dist_stats and opted._handle is None       # no device touched
    plain = make_policy(normalize=False).distributed_statistics(True)
    assert not plain._dist_stats                           # nothing to reduce without normalisation
    dist.init_process_group("gloo", init_method=f"file://{os.path.join(str(tmp_path), 'pg')}", rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError, match="cross-process reduction") as e:
            pol._visual_input(obs, CPU)
        assert "distributed_statistics" in str(e.value)    # the refusal names the opt-in
        stats = opted._visual_input(obs, CPU)[0].stats
        rmv = opted.net.visual_encoder.running_mean_and_var
        assert stats[3] == 1 and stats[0] is rmv._mean and stats[1] is rmv._var and stats[2] is rmv._count
        assert opted._visual_input(obs, CPU)[0].args()[6] == 1
        opted.eval()
        assert opted._visual_input(obs, CPU)[0].stats[3] == 0
        opted.train().distributed_statistics(False)        # opting out brings the refusal back
        with pytest.raises(NotImplementedError, match="cross-process reduction"):
            opted._visual_input(obs, CPU)
    finally:
        dist.destroy_process_group()
