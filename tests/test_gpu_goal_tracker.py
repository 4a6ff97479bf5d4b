"""GPU (-m gpu): geometry.GoalTracker (csrc/nav_state.hip: pnvo_nav_update / pnvo_nav_reset) against the host functions it mirrors,
geometry.compute_goal_pos_batch / compute_goal_pos / compute_global_state, with the state carried on each side independently.

The kernel is float64 in the host functions' operation order and built without a*b+c fusion, so the two sides can differ only through
sin, cos, hypot and atan2.  A CPU simulation of the host functions with +-4 ulp noise on exactly those four results (300 environments,
64 steps) drifted 3.6e-14 in the cartesian state and changed 0 of 38 400 polar values.  The bounds below follow from that:
  * goal, pos, rot within 1e-11 absolute after 64 steps;
  * polar within one float32 ulp, the angle after wrapping the difference into (-pi, pi] (a few values lie within 1e-3 of the cut);
  * at most 1 in 1000 polar values differ at all — a systematically different formula fails this even where each value is within an ulp.
Shapes: 1, 65 and 300 environments (one lane; more than one wave; a partial second 256-thread workgroup)."""
import functools

import numpy as np
import pytest
import torch

from pointnav_vo_amd import geometry
from pointnav_vo_amd.geometry import GoalTracker

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
T = 64
TOL = 1e-11


def yaw_quat(yaw):
    yaw = np.asarray(yaw, dtype=np.float64)
    z = np.zeros_like(yaw)
    return np.stack([z, np.sin(yaw / 2.0), z, np.cos(yaw / 2.0)], axis=-1)


def make_goals(E, rng):
    g = rng.uniform(-8.0, 8.0, size=(E, 3))
    g[:, 1] = rng.uniform(-0.5, 0.5, size=E)
    return g


def make_deltas(E, steps, rng, forward_only=False):
    """[steps, E, 3] float32 (dx, dz, dyaw): a forward step (dz ~ -0.25) or a turn of +-10 degrees, each with uniform noise of
    +-0.03 m / +-0.02 rad; forward_only: dyaw == 0.0 exactly."""
    d = np.empty((steps, E, 3))
    d[..., 0] = rng.uniform(-0.03, 0.03, size=(steps, E))
    d[..., 1] = rng.uniform(-0.03, 0.03, size=(steps, E))
    d[..., 2] = rng.uniform(-0.02, 0.02, size=(steps, E))
    fwd = rng.random((steps, E)) < 0.6
    d[..., 1] += np.where(fwd, -0.25, 0.0)
    d[..., 2] += np.where(fwd, 0.0, np.where(rng.random((steps, E)) < 0.5, 1.0, -1.0) * np.deg2rad(10.0))
    if forward_only:
        d[..., 1] = rng.uniform(-0.28, -0.22, size=(steps, E))
        d[..., 2] = 0.0
    return d.astype(np.float32)


def start_state(E, seed):
    """A host start state: world goals, start poses (a yaw about y), and the agent-frame goal compute_goal_pos derives from them."""
    rng = np.random.default_rng(seed)
    goals_world = make_goals(E, rng)
    pos = rng.uniform(-3.0, 3.0, size=(E, 3))
    rot = yaw_quat(rng.uniform(-np.pi, np.pi, size=E))
    goal = np.stack([geometry.compute_goal_pos(goals_world[e], [pos[e, 0], pos[e, 2], 2 * np.arctan2(rot[e, 1], rot[e, 3])])["cartesian"]
                     for e in range(E)])
    return goal, rot, pos, rng


def host_step(goal, rot, pos, d, rows=None):
    """One step of the host functions on float32 deltas d [n,3] for the given rows (all by default), in place -> polar [n,2]."""
    rows = np.arange(goal.shape[0]) if rows is None else np.asarray(rows)
    d = np.asarray(d, dtype=np.float64)                  # widened first, as the kernel does (float32 scalars would keep sin / cos in float32)
    res = geometry.compute_goal_pos_batch(goal[rows], d)
    goal[rows] = res["cartesian"]
    if rot is not None:
        for i, e in enumerate(rows):
            rot[e], pos[e] = geometry.compute_global_state((rot[e], pos[e]), d[i])
    return res["polar"]


@functools.lru_cache(maxsize=None)
def host_run(E, forward_only=False):
    """The shared host reference: T steps from start_state(E) -> (start, deltas, final goal / rot / pos, polar [T,E,2]).  Read only."""
    goal, rot, pos, rng = start_state(E, seed=100 + E)
    start = (goal.copy(), rot.copy(), pos.copy())
    deltas = make_deltas(E, T, rng, forward_only)
    polar = np.stack([host_step(goal, rot, pos, deltas[t]) for t in range(T)])
    for a in start + (deltas, goal, rot, pos, polar):
        a.setflags(write=False)
    return start, deltas, goal, rot, pos, polar


def tracker_from(start, track_pose=True):
    """A tracker whose state is, bit for bit, the host start state."""
    goal, rot, pos = start
    tr = GoalTracker(goal.shape[0], DEV, track_pose=track_pose)
    tr.goal.copy_(torch.from_numpy(np.array(goal)))
    if track_pose:
        tr.rot.copy_(torch.from_numpy(np.array(rot)))
        tr.pos.copy_(torch.from_numpy(np.array(pos)))
    return tr


def device_run(tr, deltas):
    """Every step of deltas [steps,E,3] on the tracker -> the polar goal after each step, host [steps,E,2]."""
    d = torch.from_numpy(np.array(deltas)).to(DEV)
    out = []
    for t in range(d.shape[0]):
        tr.update(d[t])
        out.append(tr.polar.clone())                     # (polar is updated in place by the next step)
    return torch.stack(out).cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def check_polar(dev, host, what=""):
    """Both float32 [..., 2].  Within one float32 ulp (angle: wrapped difference), at most 1 in 1000 values different at all."""
    dev, host = np.asarray(dev), np.asarray(host)
    assert dev.dtype == np.float32 and host.dtype == np.float32 and dev.shape == host.shape
    ulp = np.spacing(np.maximum(np.abs(dev), np.abs(host))).astype(np.float64)
    diff = dev.astype(np.float64) - host.astype(np.float64)
    ang = diff[..., 1]
    ang = np.where(ang > np.pi, ang - 2 * np.pi, np.where(ang <= -np.pi, ang + 2 * np.pi, ang))
    over_rho = np.abs(diff[..., 0]) / ulp[..., 0]
    over_phi = np.abs(ang) / ulp[..., 1]
    changed = int((bits(dev) != bits(host)).sum())
    print(f"polar {what}: {dev.size} values, {changed} differ, worst rho {over_rho.max():.3g} ulp, worst angle {over_phi.max():.3g} ulp")
    assert over_rho.max() <= 1.0 and over_phi.max() <= 1.0, (over_rho.max(), over_phi.max())
    assert changed * 1000 <= dev.size, (changed, dev.size)
    return changed


def check_cartesian(tr, goal, rot, pos, what=""):
    g = tr.cartesian()
    errs = [np.abs(g - goal).max()]
    if rot is not None:
        r, p = tr.global_state()
        errs += [np.abs(r - rot).max(), np.abs(p - pos).max()]
    print(f"cartesian {what}: max |goal, rot, pos difference| = {errs}")
    assert max(errs) <= TOL, errs


@pytest.mark.parametrize("E", [1, 65, 300])
def test_sixty_four_steps_match_the_host_functions(E):
    start, deltas, goal, rot, pos, polar = host_run(E)
    tr = tracker_from(start)
    got = device_run(tr, deltas)
    check_cartesian(tr, goal, rot, pos, f"E={E}")
    check_polar(got, polar, f"E={E}")
    assert tr.polar.dtype == torch.float32 and tuple(tr.polar.shape) == (E, 2)


def test_forward_only_steps_are_bit_equal():
    """dyaw == 0.0: sin and cos are exact in any libm, so the cartesian state must match the host to the last bit (this is what
    -ffp-contract=off and the operation order buy)."""
    start, deltas, goal, rot, pos, polar = host_run(65, True)
    tr = tracker_from(start)
    got = device_run(tr, deltas)
    g = tr.cartesian()
    r, p = tr.global_state()
    assert np.array_equal(bits(g), bits(goal)), np.abs(g - goal).max()
    assert np.array_equal(bits(p), bits(pos)), np.abs(p - pos).max()
    assert np.array_equal(r, rot)
    check_polar(got, polar, "forward only")


def test_goal_only_tracker_gives_the_same_goal():
    start, deltas, *_ = host_run(65)
    full, goal_only = tracker_from(start), tracker_from(start, track_pose=False)
    assert goal_only.rot is None and goal_only.pos is None
    a, b = device_run(full, deltas[:16]), device_run(goal_only, deltas[:16])
    assert np.array_equal(bits(a), bits(b))
    assert torch.equal(full.goal, goal_only.goal) and torch.equal(full.polar, goal_only.polar)


def test_subset_update_touches_only_the_named_rows():
    E = 65
    start, deltas, *_ = host_run(E)
    goal, rot, pos = (np.array(a) for a in start)
    tr = tracker_from(start)
    rng = np.random.default_rng(7)
    for t in range(4):                                   # a few full steps first: every row holds a state of its own
        host_step(goal, rot, pos, deltas[t])
    device_run(tr, deltas[:4])
    polar_h = tr.polar.cpu().numpy()
    for rep in range(3):
        rows = rng.permutation(E)[:23]                   # shuffled, not sorted, spread over both waves
        d = make_deltas(len(rows), 1, rng)[0]
        big = torch.zeros((len(rows), 5), device=DEV)    # a row stride of five floats
        big[:, 1:4] = torch.from_numpy(d).to(DEV)
        before = [x.clone() for x in (tr.goal, tr.rot, tr.pos, tr.polar)]
        tr.update(big[:, 1:4], [int(e) for e in rows])
        polar_h[rows] = host_step(goal, rot, pos, d, rows)
        others = torch.ones(E, dtype=torch.bool, device=DEV)
        others[torch.from_numpy(rows).to(DEV)] = False
        for now, was in zip((tr.goal, tr.rot, tr.pos, tr.polar), before):
            same = torch.int64 if now.dtype == torch.float64 else torch.int32
            assert torch.equal(now[others].view(same), was[others].view(same))      # not a single byte
            assert not torch.equal(now, was)
        check_cartesian(tr, goal, rot, pos, f"subset {rep}")
        check_polar(tr.polar.cpu().numpy()[rows], polar_h[rows], f"subset {rep}")
    assert len(tr._index_cache) == 3
    tr.update(big[:, 1:4], [int(e) for e in rows])       # the same tuple again: its index tensor is reused
    assert len(tr._index_cache) == 3


def test_reset_mid_sequence_starts_three_episodes():
    E = 65
    start, deltas, *_ = host_run(E)
    goal, rot, pos = (np.array(a) for a in start)
    tr = tracker_from(start)
    for t in range(5):
        host_step(goal, rot, pos, deltas[t])
    device_run(tr, deltas[:5])
    rows = [7, 64, 0]
    rng = np.random.default_rng(11)
    goals_world = make_goals(3, rng)
    spos = rng.uniform(-3.0, 3.0, size=(3, 3))
    srot = yaw_quat(rng.uniform(-np.pi, np.pi, size=3))
    before = [x.clone() for x in (tr.goal, tr.rot, tr.pos, tr.polar)]
    tr.reset(rows, goals_world, spos, srot)
    want_polar = []
    for i, e in enumerate(rows):                         # ppo_trainer.py:727-740
        res = geometry.compute_goal_pos(goals_world[i], [spos[i, 0], spos[i, 2], 2 * np.arctan2(srot[i, 1], srot[i, 3])])
        goal[e], rot[e], pos[e] = res["cartesian"], srot[i], spos[i]
        want_polar.append(res["polar"])
    r, p = tr.global_state()
    assert np.array_equal(bits(r[rows]), bits(srot)) and np.array_equal(bits(p[rows]), bits(spos))
    check_cartesian(tr, goal, rot, pos, "after reset")
    check_polar(tr.polar.cpu().numpy()[rows], np.stack(want_polar), "after reset")
    others = torch.ones(E, dtype=torch.bool, device=DEV)
    others[rows] = False
    for now, was in zip((tr.goal, tr.rot, tr.pos, tr.polar), before):
        same = torch.int64 if now.dtype == torch.float64 else torch.int32
        assert torch.equal(now[others].view(same), was[others].view(same))
    # the episodes go on from there
    polar_h = np.stack([host_step(goal, rot, pos, deltas[t]) for t in range(5, 13)])
    got = device_run(tr, deltas[5:13])
    check_cartesian(tr, goal, rot, pos, "eight steps after reset")
    check_polar(got, polar_h, "eight steps after reset")


def test_update_replays_from_a_captured_graph():
    """update() captured in a graph and replayed on new delta values gives the eager result bit for bit.  A call that waits for the
    device raises inside a capture, so this also shows that update() does not wait."""
    E = 65
    start, deltas, *_ = host_run(E)
    eager, graphed = tracker_from(start), tracker_from(start)
    d = torch.from_numpy(np.array(deltas[:4])).to(DEV)
    tracker_from(start).update(d[0])                     # (the kernel has run once before anything is captured)
    static = torch.zeros((E, 3), device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.update(static)
    for t in range(4):
        static.copy_(d[t])
        g.replay()
        eager.update(d[t])
    torch.cuda.synchronize()
    for a, b in ((eager.goal, graphed.goal), (eager.rot, graphed.rot), (eager.pos, graphed.pos)):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert torch.equal(eager.polar.view(torch.int32), graphed.polar.view(torch.int32))
    assert not torch.equal(eager.goal, torch.from_numpy(np.array(start[0])).to(DEV))
