"""GPU (-m gpu): compute_local_delta_states_batch(..., to_host=False) — the batched boundary call that leaves its deltas on the device
(a CUDA float32 [n,3] tensor in the caller's order) and does not wait for the GPU.  Bit-exact against the default call; what the
default call's final synchronisation guards — the pinned staging and the depth-range assertion — is deferred to the next boundary
call on the trainer and to check_deferred().  Trainer, golden size and frames as tests/test_gpu_boundary_ring.py."""
import functools
import time

import numpy as np
import pytest
import torch

from conftest import load_golden
from pointnav_vo_amd.geometry import GoalTracker
from test_gpu_async import _backlog
from test_gpu_boundary_ring import frames
from test_gpu_parity import make_trainer

pytestmark = pytest.mark.gpu
E, T = 6, 4
DEPTH_MSG = r"depth must lie in \[0, 1\]"


@functools.lru_cache(maxsize=None)
def shared():
    """Two trainers with the same weights (one takes the device path, one is the host reference) and the frames of E environments."""
    rec = load_golden("boundary.npz")
    H, W = int(rec["height"]), int(rec["width"])
    seq = {e: [frames(H, W, e, t, fp16=(e % 2 == 0)) for t in range(T + 2)] for e in range(E)}
    return make_trainer(rec), make_trainer(rec), seq


def fresh():
    dev_t, host_t, seq = shared()
    for t in (dev_t, host_t):
        t.check_deferred()
        t.reset_frame_ring()
    return dev_t, host_t, seq


def steps(seq):
    """(prevs, curs, acts, env ids) of T steps; step 2 is a subset of the environments in another order."""
    rng = np.random.default_rng(3)
    acts_all = rng.integers(1, 4, size=(T, E))
    for t in range(T):
        envs = [4, 1, 5, 0] if t == 2 else list(range(E))
        yield [seq[e][t] for e in envs], [seq[e][t + 1] for e in envs], [int(acts_all[t, e]) for e in envs], envs


@pytest.mark.parametrize("ring", [False, True], ids=["no_env_ids", "env_ids"])
def test_device_deltas_are_the_host_deltas(ring):
    dev_t, host_t, seq = fresh()
    for t, (prevs, curs, acts, envs) in enumerate(steps(seq)):
        kw = dict(env_ids=envs) if ring else {}
        got = dev_t.compute_local_delta_states_batch(prevs, curs, acts, to_host=False, **kw)
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (len(envs), 3)
        want = host_t.compute_local_delta_states_batch(prevs, curs, acts, **kw)
        assert len(set(acts)) > 1                                       # several action models: the un-permute on the device is exercised
        assert np.array_equal(got.cpu().numpy(), want), (t, acts)
        if ring:
            assert dev_t._ring_stats == host_t._ring_stats and (dev_t._ring_stats["ring_hits"] > 0) == (t > 0)
    dev_t.check_deferred()


@pytest.mark.parametrize("ring", [False, True], ids=["no_env_ids", "env_ids"])
def test_default_call_right_after_a_device_call_reuses_the_staging_safely(ring):
    """The default call refills the pinned staging the device call's copies may still be reading: it waits for that call's event."""
    dev_t, host_t, seq = fresh()
    (p1, c1, a1, e1), (p2, c2, a2, e2) = list(steps(seq))[:2]
    kw1, kw2 = (dict(env_ids=e1), dict(env_ids=e2)) if ring else ({}, {})
    r1 = dev_t.compute_local_delta_states_batch(p1, c1, a1, to_host=False, **kw1)
    r2 = dev_t.compute_local_delta_states_batch(p2, c2, a2, **kw2)      # right behind it, no synchronisation in between
    assert isinstance(r2, np.ndarray)
    assert np.array_equal(r1.cpu().numpy(), host_t.compute_local_delta_states_batch(p1, c1, a1, **kw1))
    assert np.array_equal(r2, host_t.compute_local_delta_states_batch(p2, c2, a2, **kw2))
    if ring:
        assert dev_t._ring_stats == host_t._ring_stats and dev_t._ring_stats["ring_hits"] == E
    assert getattr(dev_t, "_deferred", None) is None                     # a default call leaves nothing pending


def test_depth_out_of_range_is_reported_by_check_deferred_and_by_the_next_call():
    dev_t, host_t, seq = fresh()
    (p1, c1, a1, _), (p2, c2, a2, _) = list(steps(seq))[:2]
    bad = {k: v.copy() for k, v in c1[3].items()}
    bad["depth"][5, 7] = 1.5
    c_bad = list(c1)
    c_bad[3] = bad
    out = dev_t.compute_local_delta_states_batch(p1, c_bad, a1, to_host=False)       # returns: nothing has looked at the flag yet
    assert out.is_cuda
    with pytest.raises(AssertionError, match=DEPTH_MSG):
        dev_t.check_deferred()
    dev_t.check_deferred()                                                          # reported once
    dev_t.compute_local_delta_states_batch(p1, c_bad, a1, to_host=False)
    with pytest.raises(AssertionError, match=DEPTH_MSG):
        dev_t.compute_local_delta_states_batch(p2, c2, a2)                           # the next boundary call, before it stages anything
    dev_t.compute_local_delta_states_batch(p1, c_bad, a1, to_host=False)
    with pytest.raises(AssertionError, match=DEPTH_MSG):
        dev_t.compute_local_delta_states_batch(p2, c2, a2, to_host=False)
    # and the trainer goes on: clean frames, clean result
    got = dev_t.compute_local_delta_states_batch(p2, c2, a2, to_host=False)
    dev_t.check_deferred()
    assert np.array_equal(got.cpu().numpy(), host_t.compute_local_delta_states_batch(p2, c2, a2))


def test_device_call_and_tracker_update_do_not_wait_for_the_gpu():
    """The backlog pattern of tests/test_gpu_async.py: ~150 ms of work queued ahead; the call and GoalTracker.update return while it is
    still running, in launch time."""
    dev_t, _, seq = fresh()
    p1, c1, a1, e1 = next(steps(seq))
    tracker = GoalTracker(E, dev_t.device)
    tracker.update(dev_t.compute_local_delta_states_batch(p1, c1, a1, env_ids=e1, to_host=False))      # warm: buffers, index caches
    dev_t.check_deferred()
    dev_t.reset_frame_ring()
    torch.cuda.synchronize()
    behind = _backlog()
    t0 = time.perf_counter()
    deltas = dev_t.compute_local_delta_states_batch(p1, c1, a1, env_ids=e1, to_host=False)
    tracker.update(deltas)
    host_ms = (time.perf_counter() - t0) * 1e3
    still_busy = not behind.query()
    torch.cuda.synchronize()
    dev_t.check_deferred()
    print(f"to_host=False call + tracker.update behind a backlog: {host_ms:.2f} ms on the host, backlog still busy: {still_busy}")
    assert still_busy, "the call returned only after the GPU had drained the work queued ahead of it"
    assert host_ms < 40.0, host_ms
    assert np.isfinite(tracker.cartesian()).all()


def test_unsupported_configurations_are_refused_before_anything_is_touched():
    dev_t, _, seq = fresh()
    p1, c1, a1, _ = next(steps(seq))
    rm = dev_t.config.VO.REGRESS_MODEL
    rm.mode = "rnd"
    try:
        with pytest.raises(ValueError, match="rnd"):
            dev_t.compute_local_delta_states_batch([None], [None], [1], to_host=False)      # (frames that no code may look at)
    finally:
        rm.mode = "det"
    dev_t.config.VO.OBS_TRANSFORM = "resize"
    dev_t._set_up_vo_obs_transformer()
    try:
        with pytest.raises(ValueError, match="resize"):
            dev_t.compute_local_delta_states_batch([None], [None], [1], to_host=False)
    finally:
        dev_t.config.VO.OBS_TRANSFORM = "none"
        dev_t._set_up_vo_obs_transformer()
    assert dev_t._vo_obs_transformer is None
    assert dev_t.compute_local_delta_states_batch(p1, c1, a1, to_host=False).shape == (E, 3)
    dev_t.check_deferred()
