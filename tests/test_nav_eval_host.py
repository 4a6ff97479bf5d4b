"""CPU: geometry.NavEvalBook (the evaluation loop's VO bookkeeping as running sums, the definition the device form follows) against the
reference's list-append form restated in tests/nav_eval_reference.py, on the scripted 5-environment run; angle_between_quaternions;
the argument refusals of NavEvalStats on a CPU tracker.

Both sides of the comparison are sequential float64; np.sum over the few rows of this run adds in the book's order, so the two agree
far inside the 1e-12 relative bound: the run showed a largest relative difference of 0.0 in result() and in every diff row (every
value bit-equal)."""
import numpy as np
import pytest
import torch

from nav_eval_reference import ListReference, drive, small_run
from pointnav_vo_amd import geometry
from pointnav_vo_amd.geometry import GoalTracker, NavEvalBook, NavEvalStats
from test_gpu_goal_tracker import yaw_quat

RTOL = 1e-12


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)))


def test_book_matches_the_list_form_on_the_scripted_run():
    run = small_run()
    book, ref = NavEvalBook(5), ListReference(5)
    got, want = drive(run, book), drive(run, ref)
    assert [rows for rows, _ in got] == [rows for rows, _ in want]
    assert [rows for rows, _ in got][:4] == [[1], [4], [3, 2], [4]] and sorted(got[-1][0]) == [0, 1, 2, 3, 4]
    worst = 0.0
    for (rows, a), (_, b) in zip(got, want):
        assert a.shape == (len(rows), 3)
        worst = max(worst, rel(a, b))
    assert np.array_equal(got[0][1], np.zeros((1, 3)))                 # environment 1 ended before any VO step
    assert all((a > 0).all() for _, a in got[1:])
    r, w = book.result(), ref.result()
    assert r["episodes"] == w["episodes"] == 10 and r["steps"] == w["steps"] == int(sum(len(s["live"]) for s in run["loop"]))
    for key in ("vo_l2_loss", "vo_pred_std", "vo_l2_gloabl_state"):
        assert r[key].shape == (3,) and (r[key] > 0).all()
        worst = max(worst, rel(r[key], w[key]))
    print(f"NavEvalBook vs the list form: largest relative difference {worst:.3g}")
    assert worst <= RTOL, worst
    assert np.array_equal(r["l2_sum"] / r["steps"], r["vo_l2_loss"]) and np.array_equal(r["diff_sum"] / 10, r["vo_l2_gloabl_state"])
    assert not book.steps.any() and not book.abs_sum.any() and not book.std_sum.any()      # every episode was closed


def test_order_of_two_simultaneous_episode_ends_reaches_the_bits_of_l2_sum():
    """Environments 3 and 2 end in the same loop step (the third end_episodes call).  Fed in the other order, l2_sum after that call
    differs in all three components for this seed (of seeds 0..11, seven change a bit there; this one was chosen for it): the device
    test's bit-equality of the totals after that call can therefore fail if the kernel walked the rows in another order.  Later
    additions round the one-ulp difference away again — the final sums of the two runs coincide — which is why the device test
    compares after every call and not at the end only."""
    run = small_run()
    seen = []
    for reverse_at in (None, 6):
        book, after = NavEvalBook(5), []
        ends = drive(run, book, reverse_at=reverse_at, on_end=lambda ending, order, got: after.append(book.l2_sum.copy()))
        seen.append((ends[2][0], after[2], book.result()["episodes"]))
    (rows_a, l2_a, n_a), (rows_b, l2_b, n_b) = seen
    assert rows_a == [3, 2] and rows_b == [2, 3] and n_a == n_b
    assert (l2_a.view(np.int64) != l2_b.view(np.int64)).all(), (l2_a, l2_b)
    assert rel(l2_a, l2_b) < 1e-15


def test_trajectories_hold_each_episode_and_nothing_of_the_one_before():
    run = small_run()
    book = NavEvalBook(5, max_episode_steps=16, keep_trajectories=True)
    ends = drive(run, book)
    lengths = {}
    for rows, (diff, logs) in ends:
        assert len(logs) == len(rows)
        for e, rec, d in zip(rows, logs, diff):
            lengths.setdefault(e, []).append(rec.shape[0])
            assert rec.shape[1] == 16
            if rec.shape[0]:
                assert np.array_equal(rec[:, 0:3].astype(np.float32).astype(np.float64), rec[:, 0:3])    # float32 deltas, widened
                assert np.allclose(np.linalg.norm(rec[:, 9:13], axis=1), 1.0, atol=1e-12)
    assert lengths == {0: [12], 1: [0, 11], 2: [6, 5], 3: [6, 5], 4: [4, 5, 1]}
    with pytest.raises(ValueError, match="max_episode_steps"):
        small = NavEvalBook(1, max_episode_steps=1)
        small.step([0], np.zeros((1, 3), np.float32), np.zeros((1, 3)))
        small.step([0], np.zeros((1, 3), np.float32), np.zeros((1, 3)))
    two = NavEvalBook(2, max_episode_steps=1)                          # a refused step leaves the rows in front of the full one alone
    two.step([1], np.ones((1, 3), np.float32), np.zeros((1, 3)))
    with pytest.raises(ValueError, match="max_episode_steps"):
        two.step([0, 1], np.ones((2, 3), np.float32), np.zeros((2, 3)))
    assert two.steps.tolist() == [0, 1] and not two.abs_sum[0].any() and not two.pos[0].any()
    with pytest.raises(ValueError, match="inside an episode"):
        small.reset([0], np.zeros((1, 3)), [[0.0, 0.0, 0.0, 1.0]])


def test_angle_between_quaternions():
    ang = geometry.angle_between_quaternions
    rng = np.random.default_rng(5)
    q = rng.normal(size=(8, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    for a in q:
        assert ang(a, a) <= 1e-7                                       # sqrt of a rounding residue, not an exact zero in general
    assert ang([0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 1.0]) == 0.0
    yaws = rng.uniform(-np.pi, np.pi, size=(16, 2))
    for y1, y2 in yaws:
        want = abs(y1 - y2)
        want = 2 * np.pi - want if want > np.pi else want              # |yaw1 - yaw2| wrapped to [0, pi]
        got = ang(yaw_quat(y1), yaw_quat(y2))
        assert 0.0 <= got <= np.pi and abs(got - want) <= 1e-12, (y1, y2, got, want)
    for a, b in zip(q[:4], q[4:]):
        assert abs(ang(a, b) - ang(b, a)) <= 1e-15                     # symmetric
        assert ang(-a, b) == ang(a, b) == ang(a, -b)                   # q and -q are one rotation


def test_stats_refuse_bad_arguments_on_a_cpu_tracker_before_the_gpu_is_asked_for():
    with pytest.raises(ValueError, match="track_pose=True"):
        NavEvalStats(GoalTracker(3, "cpu", track_pose=False))
    with pytest.raises(ValueError, match="track_pose=True"):
        NavEvalStats(object())
    with pytest.raises(ValueError, match="max_episode_steps"):
        NavEvalStats(GoalTracker(3, "cpu"), max_episode_steps=0)
    st = NavEvalStats(GoalTracker(3, "cpu"), max_episode_steps=4, keep_trajectories=True)
    assert st.traj.shape == (3, 4, 16) and st.steps.dtype == torch.int64
    d, gt = torch.zeros(3, 3), np.zeros((3, 3))
    bad_updates = [
        (dict(deltas=np.zeros((3, 3), np.float32), gt_deltas=gt), "deltas must be"),
        (dict(deltas=torch.zeros(3, 2), gt_deltas=gt), "float32 \\[n,3\\]"),
        (dict(deltas=d.double(), gt_deltas=gt), "float32 \\[n,3\\]"),
        (dict(deltas=d[:2], gt_deltas=gt[:2]), "pass env_indices"),
        (dict(deltas=d[:2], gt_deltas=gt[:2], env_indices=[0, 0]), "distinct"),
        (dict(deltas=d[:2], gt_deltas=gt[:2], env_indices=[0, 3]), "outside"),
        (dict(deltas=d[:2], gt_deltas=gt[:2], env_indices=[0]), "1 environment indices for 2 rows"),
        (dict(deltas=d, gt_deltas=gt[:2]), "gt_deltas must have shape"),
        (dict(deltas=d, gt_deltas=np.zeros((3, 4))), "gt_deltas must have shape"),
        (dict(deltas=d, gt_deltas="no"), "gt_deltas must be a numeric"),
        (dict(deltas=d, gt_deltas=gt, stds=np.zeros((3, 3), np.float32)), "stds must be"),
        (dict(deltas=d, gt_deltas=gt, stds=torch.zeros(3, 2)), "stds must be"),
        (dict(deltas=d, gt_deltas=gt, stds=torch.zeros(3, 3, dtype=torch.float64)), "stds must be"),
        (dict(deltas=d, gt_deltas=gt), "CUDA tensors"),                # a well-formed call with host deltas: still a ValueError
    ]
    for kw, msg in bad_updates:
        with pytest.raises(ValueError, match=msg):
            st.update(**kw)
    st._host_steps[1] = 4                                              # environment 1 has used up its max_episode_steps
    with pytest.raises(ValueError, match="max_episode_steps"):
        st.update(d, gt)
    st._host_steps[1] = 0
    ok_pos, ok_rot = np.zeros((2, 3)), np.tile([0.0, 0.0, 0.0, 1.0], (2, 1))
    for args, msg in [(([0, 0], ok_pos, ok_rot), "distinct"), (([0, 5], ok_pos, ok_rot), "outside"), (([0.5, 1], ok_pos, ok_rot), "integer"),
                      (([0, 1], ok_pos[:1], ok_rot), "sim_positions must have shape"), (([0, 1], ok_pos, ok_pos), "sim_rotations must have shape"),
                      ((3, ok_pos, ok_rot), "sequence")]:
        with pytest.raises(ValueError, match=msg):
            st.end_episodes(*args)
    with pytest.raises(RuntimeError, match="MI355X only"):             # well-formed: only now the missing GPU is reported
        st.end_episodes([0, 1], ok_pos, ok_rot)
    with pytest.raises(RuntimeError, match="MI355X only"):
        st.result()
    assert not st._host_steps.any()                                    # no refused call counted a step
