"""GPU (-m gpu): geometry.NavEvalStats (csrc/nav_state.hip: pnvo_nav_update_eval / pnvo_nav_episode_end) against its host form
geometry.NavEvalBook, on the scripted run of tests/nav_eval_reference.py (5 environments: a zero-step episode, two environments that
end in one call, two episodes in one environment; permuted subset index tuples, deltas with a row stride of 4 floats) and on a run of
300 environments (a partial second 256-thread workgroup in the update; more rows than threads in the episode end).

  * the wrapped tracker's goal / rot / pos / polar after every step: torch.equal to a twin GoalTracker driven by plain update();
  * steps, abs_sum, std_sum per environment after every step, and episodes / steps / l2_sum / std_sum of the run after every
    end_episodes: bit-equal to the book (the kernels add in the book's order, without a*b+c fusion);
  * diff rows and diff_sum: x and z within 1e-11 absolute (tests/test_gpu_goal_tracker.py's bound on the pose after at most 64 steps;
    the simulator's pose is a common input), the yaw angle within 1e-10 (each dq component is four products with a factor that is
    within 1e-11; 2 atan2 on the unit circle is 2-Lipschitz);
  * trajectory records: delta, gt and std columns bit-equal, pose columns within 1e-11.

Largest |device - host| seen on an MI355X (the tests print them): 5 environments — diff x / z 0.0, diff yaw 8.7e-19, diff_sum x / z
0.0, diff_sum yaw 8.7e-19; 300 environments — diff x / z 0.0, diff yaw 6.9e-18, diff_sum 0.0; pose columns of the trajectory records
0.0 (on these inputs the device's sin / cos gave the host's bits).  update + end_episodes + reset behind a 150 ms backlog: 0.6 ms on
the host."""
import functools
import time

import numpy as np
import pytest
import torch

from nav_eval_reference import drive, make_run, small_run
from pointnav_vo_amd.geometry import GoalTracker, NavEvalBook, NavEvalStats
from test_gpu_async import _backlog
from test_gpu_goal_tracker import bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
POS_TOL, YAW_TOL = 1e-11, 1e-10


@functools.lru_cache(maxsize=None)
def big_run():
    """300 environments, 5 loop steps, no stds: 37 scattered environments end together in step 2, the others after step 5."""
    rows = [int(e) for e in np.random.default_rng(1).permutation(300)[:37]]
    return make_run(300, 5, {2: rows}, seed=17, with_std=False)


class Both:
    """The book's interface over the host book AND the device form with its twin tracker: every call goes to both and is compared."""

    def __init__(self, run, keep=False, max_steps=16):
        E = run["E"]
        self.book = NavEvalBook(E, max_steps, keep)
        self.tracker, self.twin = GoalTracker(E, DEV), GoalTracker(E, DEV)
        self.stats = NavEvalStats(self.tracker, max_steps, keep)
        self.keep = keep
        self.worst = {"diff x/z": 0.0, "diff yaw": 0.0, "diff_sum x/z": 0.0, "diff_sum yaw": 0.0, "record pose": 0.0}
        self.host_logs, self.dev_logs = [], []

    def see(self, key, value):
        self.worst[key] = max(self.worst[key], float(value))

    def reset(self, env_indices, pos, rot):
        idx = list(env_indices)
        self.book.reset(idx, pos, rot)
        goals = np.asarray(pos)[:, ::-1] * 0.5 + 1.0
        for t in (self.tracker, self.twin):
            t.reset(idx, goals, pos, rot)

    def step(self, env_indices, deltas, gt, stds=None):
        n = len(env_indices)
        self.book.step(env_indices, deltas, gt, stds)
        wide = torch.zeros((n, 4), device=DEV)                          # a row stride of four floats
        wide[:, :3] = torch.from_numpy(deltas).to(DEV)
        d = wide[:, :3]
        self.stats.update(d, gt, env_indices, None if stds is None else torch.from_numpy(stds).to(DEV))
        self.twin.update(d, env_indices)
        for name in ("goal", "rot", "pos", "polar"):
            assert torch.equal(getattr(self.tracker, name), getattr(self.twin, name)), name
        self.check_rows()

    def check_rows(self):
        st, bk = self.stats, self.book
        assert np.array_equal(st.steps.cpu().numpy(), bk.steps) and np.array_equal(st._host_steps, bk.steps)
        assert np.array_equal(bits(st.abs_sum.cpu().numpy()), bits(bk.abs_sum))
        assert np.array_equal(bits(st.std_sum.cpu().numpy()), bits(bk.std_sum))

    def end_episodes(self, env_indices, sim_pos, sim_rot):
        host = self.book.end_episodes(env_indices, sim_pos, sim_rot)
        dev = self.stats.end_episodes(env_indices, sim_pos, sim_rot)
        if self.keep:
            (host, hlogs), (dev, dlogs) = host, dev
            self.host_logs += hlogs
            self.dev_logs += dlogs
            assert [l.env for l in dlogs] == list(env_indices)
        st, bk = self.stats, self.book
        assert st.counts.tolist() == [bk.episodes, bk.steps_total]
        totals = st.totals.cpu().numpy()
        assert np.array_equal(bits(totals[0]), bits(bk.l2_sum)), (totals[0], bk.l2_sum)
        assert np.array_equal(bits(totals[1]), bits(bk.std_sum_total)), (totals[1], bk.std_sum_total)
        self.check_rows()                                               # the ended rows are cleared, the others untouched
        dev = dev.cpu().numpy()
        assert dev.shape == host.shape
        if self.keep:
            for i, log in enumerate(dlogs):                             # each log carries ITS row of this call's diff tensor
                assert np.array_equal(bits(log.diff), bits(dev[i])), (i, log.diff, dev[i])
        err, err_sum = np.abs(dev - host), np.abs(totals[2] - bk.diff_sum)
        self.see("diff x/z", err[:, :2].max())
        self.see("diff yaw", err[:, 2].max())
        self.see("diff_sum x/z", err_sum[:2].max())
        self.see("diff_sum yaw", err_sum[2])
        assert err[:, :2].max() <= POS_TOL and err[:, 2].max() <= YAW_TOL, err.max(axis=0)
        assert err_sum[:2].max() <= POS_TOL and err_sum[2] <= YAW_TOL, err_sum
        zero_step = ~(host != 0).any(axis=1)
        assert np.array_equal(dev[zero_step], host[zero_step])          # an episode without a VO step: an exact zero row
        return dev

    def check_result(self):
        r, w = self.stats.result(), self.book.result()
        assert set(r) == set(w)
        assert r["episodes"] == w["episodes"] and r["steps"] == w["steps"]
        for key in ("vo_l2_loss", "vo_pred_std", "l2_sum", "std_sum"):
            assert np.array_equal(bits(r[key]), bits(w[key])), key
        for key in ("vo_l2_gloabl_state", "diff_sum"):
            assert np.abs(r[key] - w[key])[:2].max() <= POS_TOL and abs(r[key][2] - w[key][2]) <= YAW_TOL, key
        return r


def test_scripted_run_matches_the_host_book():
    run = small_run()
    both = Both(run)
    ends = drive(run, both)
    assert [rows for rows, _ in ends][:4] == [[1], [4], [3, 2], [4]]    # 3 and 2 end in one call, in this order, as on the host
    r = both.check_result()
    assert r["episodes"] == 10 and r["steps"] == sum(len(s["live"]) for s in run["loop"])
    print("5 environments, largest |device - host|:", both.worst)


def test_three_hundred_environments_match_the_host_book():
    run = big_run()
    both = Both(run)
    ends = drive(run, both)
    assert [len(rows) for rows, _ in ends] == [37, 300]
    r = both.check_result()
    assert r["episodes"] == 337 and r["steps"] == 300 * 5 - 37
    assert (r["vo_pred_std"] == 0.0).all()                              # stds=None: zeros
    print("300 environments, largest |device - host|:", both.worst)


def test_trajectory_logs_match_the_host_book():
    run = small_run()
    both = Both(run, keep=True)
    drive(run, both)
    both.check_result()
    lengths = {}
    assert len(both.dev_logs) == len(both.host_logs) == 10
    for log, want in zip(both.dev_logs, both.host_logs):
        got = log.records
        lengths.setdefault(log.env, []).append(log.steps)
        assert got.shape == want.shape == (log.steps, 16) and got.dtype == np.float64
        assert np.array_equal(bits(got[:, :9]), bits(want[:, :9]))      # delta, gt, std
        if log.steps:
            both.see("record pose", np.abs(got[:, 9:] - want[:, 9:]).max())
        assert log.diff.shape == (3,)
    assert both.worst["record pose"] <= POS_TOL
    # an environment's later episode is shorter than its first in environments 2 and 3: its log holds its own rows only
    assert lengths == {0: [12], 1: [0, 11], 2: [6, 5], 3: [6, 5], 4: [4, 5, 1]}
    print("trajectory records, largest |device - host| in the pose columns:", both.worst["record pose"])


def test_update_without_indices_and_the_step_limit():
    E = 7
    rng = np.random.default_rng(3)
    d = torch.from_numpy(rng.uniform(-0.2, 0.2, size=(3, E, 3)).astype(np.float32)).to(DEV)
    gt = rng.uniform(-0.2, 0.2, size=(3, E, 3))
    a, b = NavEvalStats(GoalTracker(E, DEV), max_episode_steps=2), NavEvalStats(GoalTracker(E, DEV), max_episode_steps=2)
    for t in range(2):
        a.update(d[t], gt[t])
        b.update(d[t], gt[t], range(E))
    for name in ("steps", "abs_sum", "std_sum"):
        assert torch.equal(getattr(a, name), getattr(b, name))
    assert torch.equal(a.tracker.pos, b.tracker.pos) and torch.equal(a.tracker.polar, b.tracker.polar)
    before = [x.clone() for x in (a.steps, a.abs_sum, a.tracker.pos, a.tracker.goal)]
    with pytest.raises(ValueError, match="max_episode_steps"):
        a.update(d[2], gt[2])                                           # a third step of a two-step episode: nothing is launched
    with pytest.raises(ValueError, match="max_episode_steps"):
        a.update(d[2, :1], gt[2, :1], [4])
    for now, was in zip((a.steps, a.abs_sum, a.tracker.pos, a.tracker.goal), before):
        assert torch.equal(now, was)
    assert a.steps.tolist() == [2] * E
    a.end_episodes([4], np.zeros((1, 3)), [[0.0, 0.0, 0.0, 1.0]])
    a.update(d[2, :1], gt[2, :1], [4])                                  # the ended environment steps again
    assert a.steps.tolist() == [2, 2, 2, 2, 1, 2, 2] and a.result()["episodes"] == 1 and a.result()["steps"] == 2


def test_update_and_end_episodes_do_not_wait_for_the_gpu():
    """The backlog pattern of tests/test_gpu_boundary_device_deltas.py: ~150 ms of work queued ahead; update, end_episodes (with its
    trajectory copies) and the tracker's reset return while it is still running.  Reading a log and result() are what waits."""
    E = 6
    rng = np.random.default_rng(9)
    stats = NavEvalStats(GoalTracker(E, DEV), max_episode_steps=8, keep_trajectories=True)
    d = torch.from_numpy(rng.uniform(-0.2, 0.2, size=(E, 3)).astype(np.float32)).to(DEV)
    gt, pos, rot = rng.uniform(-0.2, 0.2, size=(E, 3)), np.zeros((2, 3)), np.tile([0.0, 0.0, 0.0, 1.0], (2, 1))
    stats.update(d, gt)                                                 # warm: kernels, pinned blocks, index caches
    stats.end_episodes([1, 4], pos, rot)
    stats.update(d, gt)
    torch.cuda.synchronize()
    behind = _backlog()
    t0 = time.perf_counter()
    stats.update(d, gt)
    _, logs = stats.end_episodes([1, 4], pos, rot)
    stats.tracker.reset([1, 4], pos, pos, rot)
    host_ms = (time.perf_counter() - t0) * 1e3
    still_busy = not behind.query()
    print(f"update + end_episodes + reset behind a backlog: {host_ms:.2f} ms on the host, backlog still busy: {still_busy}")
    assert still_busy, "the calls returned only after the GPU had drained the work queued ahead of them"
    assert host_ms < 40.0, host_ms
    assert logs[0].records.shape == (2, 16) and logs[1].steps == 2     # (this read waits)
    assert behind.query()
    assert stats.result()["episodes"] == 4
