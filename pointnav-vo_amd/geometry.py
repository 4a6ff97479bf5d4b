"""Goal / pose bookkeeping that consumes the VO output in the nav loop.

Restates /root/reference/pointnav_vo/utils/geometry_utils.py:69-99 (`compute_global_state`) and :115-144
(`compute_goal_pos`).  The reference delegates the rotations to third-party packages that are absent from
/root/reference and from this image — `quaternion` (numpy-quaternion, unpinned, environment.yml) and habitat-lab's
`quaternion_rotate_vector` / `cartesian_to_polar` — so the arithmetic is restated here from their published
definitions (q v q^-1 rotation; polar = (hypot(x, y), atan2(y, x))) in closed form for rotations about the y axis.
PARITY UNPINNED (no golden vectors can be captured without those packages); covered by property tests.
Quaternions are numpy arrays [x, y, z, w] (habitat's `quaternion_to_list` order).

The functions below are the host form, and the definition of the arithmetic.  `GoalTracker` is the device form for the
navigation loop: it keeps goal, pose and the policy's polar goal of E environments in device tensors and advances them
straight from the VO output (csrc/nav_state.hip: pnvo_nav_update / pnvo_nav_reset, float64 in the operation order of
`compute_goal_pos_batch` and `compute_global_state`, bit-equal to them except through sin, cos, hypot and atan2), so the deltas
never travel to the host between the VO forward and the next `policy.act`.
"""
import ctypes as C

import numpy as np


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], dtype=np.float64)


def _quat_rotate(q, v):
    """q v q^-1 for a unit quaternion q = [x, y, z, w]."""
    qv = np.asarray(q[:3], dtype=np.float64)
    w = float(q[3])
    v = np.asarray(v, dtype=np.float64)
    t = 2.0 * np.cross(qv, v)
    return v + w * t + np.cross(qv, t)


def quat_from_angle_axis_y(theta):
    """quaternion.from_rotation_vector(theta * [0, 1, 0])  (geometry_utils.py:57-66)."""
    return np.array([0.0, np.sin(theta / 2.0), 0.0, np.cos(theta / 2.0)], dtype=np.float64)


def compute_global_state(prev_global_state, local_delta_state):
    """(rotation [x,y,z,w], position [3]) at t  +  (dx, dz, dyaw) in the local frame -> state at t+1
    (geometry_utils.py:69-99): v2 = v1 + q1 * [dx,0,dz] * q1^-1 ;  q2 = q1 * rot_y(dyaw)."""
    prev_rot, prev_pos = prev_global_state
    dx, dz, dyaw = local_delta_state
    cur_pos = np.asarray(prev_pos, dtype=np.float64) + _quat_rotate(prev_rot, [dx, 0.0, dz])
    cur_rot = _quat_mul(np.asarray(prev_rot, dtype=np.float64), quat_from_angle_axis_y(dyaw))
    return cur_rot, cur_pos


def compute_goal_pos(prev_goal_pos, local_delta_state):
    """Goal position in the agent frame at t+1 from the one at t and the VO estimate (geometry_utils.py:115-144):
    g' = q^-1 (g - [dx,0,dz]) q with q = rot_y(dyaw);  polar = (rho, -phi) of (-g'_z, g'_x)."""
    dx, dz, dyaw = local_delta_state
    q = quat_from_angle_axis_y(dyaw)
    qinv = np.array([-q[0], -q[1], -q[2], q[3]])
    cur = _quat_rotate(qinv, np.asarray(prev_goal_pos, dtype=np.float64) - np.array([dx, 0.0, dz]))
    rho = np.hypot(-cur[2], cur[0])
    phi = np.arctan2(cur[0], -cur[2])
    return {"cartesian": cur, "polar": np.array([rho, -phi], dtype=np.float32)}


def compute_goal_pos_batch(prev_goal_pos, local_delta_states):
    """compute_goal_pos for E environments at once: [E,3] goals in the agent frames, [E,3] VO estimates (dx, dz, dyaw) ->
    {"cartesian": [E,3] float64, "polar": [E,2] float32}.  The same operations in the same order as the per-environment
    function (q v q^-1 with v + w t + qv x t, t = 2 qv x v, written out for qv = (0, sin(-dyaw/2), 0)): results are identical,
    the per-call Python overhead of E quaternion objects is gone (nav loop: 8 environments 0.23 -> 0.03 ms)."""
    g = np.asarray(prev_goal_pos, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(local_delta_states, dtype=np.float64).reshape(-1, 3)
    vx, vy, vz = g[:, 0] - d[:, 0], g[:, 1] - 0.0, g[:, 2] - d[:, 1]
    qy, w = -np.sin(d[:, 2] / 2.0), np.cos(d[:, 2] / 2.0)
    # t = 2 * cross((0, qy, 0), v) = 2 * (qy*vz, 0, -qy*vx);  cross((0, qy, 0), t) = (qy*tz, 0, -qy*tx)
    tx, tz = 2.0 * (qy * vz), 2.0 * (-(qy * vx))
    cur = np.stack([vx + w * tx + qy * tz, vy + w * 0.0 + 0.0, vz + w * tz + (-(qy * tx))], axis=1)
    rho = np.hypot(-cur[:, 2], cur[:, 0])
    phi = np.arctan2(cur[:, 0], -cur[:, 2])
    return {"cartesian": cur, "polar": np.stack([rho, -phi], axis=1).astype(np.float32)}


def angle_between_quaternions(q1, q2):
    """Angle of the rotation that takes q1 to q2, in [0, pi]: habitat's `angle_between_quaternions` as the evaluation uses it for the
    yaw drift (ppo_trainer.py:772), restated from its published definition — dq = conj(q1) * q2, 2 atan2(|dq_xyz|, |dq_w|).  PARITY
    UNPINNED (habitat is absent, see the header).  The norm is written out in this order; the device form follows it."""
    q1 = np.asarray(q1, dtype=np.float64)
    q2 = np.asarray(q2, dtype=np.float64)
    dq = _quat_mul(np.array([-q1[0], -q1[1], -q1[2], q1[3]]), q2)
    n = np.sqrt((dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2])
    return 2 * np.arctan2(n, np.abs(dq[3]))


TRAJ_RECORD = 16      # one logged step: delta[3], gt[3], std[3], rot[4], pos[3] (the pose AFTER the step), float64


class NavEvalBook:
    """The evaluation loop's VO bookkeeping on the host, in array form, one row per environment: the per-step VO error against the
    simulator's delta and the prediction std (ppo_trainer.py:845-848), the pose integrated from the VO (:856-873), at every episode
    end the drift of that pose against the simulator's (:742-805), and the three numbers the run reports (:1104-1128).

    The reference appends to per-environment lists and reduces them with np.sum / np.mean; here every sum is kept running and is
    SEQUENTIAL — step order within an episode, completion order (the row order of `end_episodes`) across episodes.  This order is
    the definition of the arithmetic: `NavEvalStats` below reproduces it on the device bit for bit, except through sqrt / atan2 of
    the yaw drift and the sin / cos inside the pose.  (np.sum over a handful of rows adds in the same order; over many rows it adds
    pairwise, so the list form agrees to rounding, not to the bit: tests/test_nav_eval_host.py.)"""

    def __init__(self, num_envs, max_episode_steps=500, keep_trajectories=False):
        if int(num_envs) != num_envs or int(num_envs) < 1:
            raise ValueError(f"num_envs must be a positive integer, got {num_envs!r}")
        if int(max_episode_steps) != max_episode_steps or int(max_episode_steps) < 1:
            raise ValueError(f"max_episode_steps must be a positive integer, got {max_episode_steps!r}")
        E = self.num_envs = int(num_envs)
        self.max_episode_steps = int(max_episode_steps)
        self.keep_trajectories = bool(keep_trajectories)
        self.rot = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (E, 1))
        self.pos = np.zeros((E, 3))
        self.steps = np.zeros(E, dtype=np.int64)
        self.abs_sum = np.zeros((E, 3))
        self.std_sum = np.zeros((E, 3))
        self.traj = np.zeros((E, self.max_episode_steps, TRAJ_RECORD)) if self.keep_trajectories else None
        self.episodes = 0
        self.steps_total = 0
        self.l2_sum = np.zeros(3)
        self.std_sum_total = np.zeros(3)
        self.diff_sum = np.zeros(3)

    @staticmethod
    def _rows(a, n, cols, what):
        a = np.asarray(a, dtype=np.float64)
        if a.shape != (n, cols):
            raise ValueError(f"{what} must have shape ({n}, {cols}), got {a.shape}")
        return a

    def reset(self, env_indices, start_positions, start_rotations):
        """Episode start: the pose from the VO becomes the start pose (:737-740)."""
        idx = list(env_indices)
        spos = self._rows(start_positions, len(idx), 3, "start_positions")
        srot = self._rows(start_rotations, len(idx), 4, "start_rotations")
        for i, e in enumerate(idx):
            if self.steps[e] != 0 or self.abs_sum[e].any() or self.std_sum[e].any():
                raise ValueError(f"environment {e} is inside an episode: end it before it starts the next one")
            self.rot[e], self.pos[e] = srot[i], spos[i]

    def step(self, env_indices, deltas, gt_deltas, stds=None):
        """One VO step of the named environments: float32 deltas [n,3], the simulator's float64 deltas [n,3], stds [n,3] or None."""
        idx = list(env_indices)
        n = len(idx)
        deltas = np.asarray(deltas)
        if deltas.dtype != np.float32 or deltas.shape != (n, 3):
            raise ValueError(f"deltas must be float32 ({n}, 3), got {deltas.dtype} {deltas.shape}")
        d = deltas.astype(np.float64)                      # widened first, as the device form does
        gt = self._rows(gt_deltas, n, 3, "gt_deltas")
        sd = np.zeros((n, 3)) if stds is None else self._rows(stds, n, 3, "stds")
        over = [e for e in idx if self.steps[e] >= self.max_episode_steps]
        if over:                                           # refused before any row is touched, as the device form does
            raise ValueError(f"environments {over} are already at max_episode_steps = {self.max_episode_steps}")
        for i, e in enumerate(idx):
            self.abs_sum[e] += np.abs(d[i] - gt[i])                                          # :845-847
            self.std_sum[e] += sd[i]                                                         # :848
            self.rot[e], self.pos[e] = compute_global_state((self.rot[e], self.pos[e]), d[i])   # :864-871
            s = int(self.steps[e])
            self.steps[e] = s + 1
            if self.traj is not None:
                self.traj[e, s] = np.concatenate([d[i], gt[i], sd[i], self.rot[e], self.pos[e]])

    def end_episodes(self, env_indices, sim_positions, sim_rotations):
        """Episode end of the named environments, rows in the order given (:742-805) -> the diff rows [n,3] (|dx|, |dz|, yaw angle
        between the simulator's pose and the one from the VO); with keep_trajectories (diff rows, [one [steps,16] array per row])."""
        idx = list(env_indices)
        n = len(idx)
        spos = self._rows(sim_positions, n, 3, "sim_positions")
        srot = self._rows(sim_rotations, n, 4, "sim_rotations")
        diff = np.zeros((n, 3))
        logs = []
        for i, e in enumerate(idx):
            s = int(self.steps[e])
            if s >= 1:                                                                       # :744-783
                diff[i] = [abs(spos[i, 0] - self.pos[e, 0]), abs(spos[i, 2] - self.pos[e, 2]),
                           angle_between_quaternions(srot[i], self.rot[e])]
            self.steps_total += s                          # (an episode of zero steps adds (0, zeros) and a zero row, :789-805)
            self.l2_sum += self.abs_sum[e]
            self.std_sum_total += self.std_sum[e]
            self.diff_sum += diff[i]
            self.episodes += 1
            if self.traj is not None:
                logs.append(self.traj[e, :s].copy())
            self.steps[e] = 0
            self.abs_sum[e] = 0.0
            self.std_sum[e] = 0.0
        return (diff, logs) if self.traj is not None else diff

    def result(self):
        """The run's numbers (:1104-1128; `vo_l2_gloabl_state` is the reference's spelling of its key), the counts and the raw sums."""
        return _eval_result(self.episodes, self.steps_total, self.l2_sum, self.std_sum_total, self.diff_sum)


def _eval_result(episodes, steps_total, l2_sum, std_sum, diff_sum):
    episodes, steps_total = int(episodes), int(steps_total)
    l2_sum, std_sum, diff_sum = (np.array(a, dtype=np.float64) for a in (l2_sum, std_sum, diff_sum))
    with np.errstate(invalid="ignore", divide="ignore"):   # (a run without a step or an episode: nan, as the reference's 0 / 0)
        return {"vo_l2_loss": l2_sum / np.float64(steps_total), "vo_pred_std": std_sum / np.float64(steps_total),
                "vo_l2_gloabl_state": diff_sum / np.float64(episodes), "episodes": episodes, "steps": steps_total,
                "l2_sum": l2_sum, "std_sum": std_sum, "diff_sum": diff_sum}


class GoalTracker:
    """Goal, pose and polar goal of `num_envs` environments as device tensors, advanced by the VO deltas without a host round trip
    (the device form of the bookkeeping of rl/ppo/ppo_trainer.py:727-740, 856-878):

      goal   float64 [E,3]   goal position in the agent frame        (`compute_goal_pos(...)["cartesian"]`)
      rot    float64 [E,4]   global rotation [x,y,z,w] from the VO   (`compute_global_state(...)[0]`; None without track_pose)
      pos    float64 [E,3]   global position from the VO             (`compute_global_state(...)[1]`; None without track_pose)
      polar  float32 [E,2]   (rho, -phi): what the policy reads as `pointgoal_with_gps_compass`

    `polar` (like the other three) is ONE tensor for the tracker's lifetime, UPDATED IN PLACE by the next `update` / `reset`: feed it
    to `policy.act` of this step, and clone it if its values must outlive the next update.  `update` and `reset` are one launch each
    on the current stream and never wait for the device; `cartesian()` and `global_state()` copy to the host on demand (trajectory
    logging).  The launches need an MI355X: a tracker on a CPU device can be built and validates its arguments, but there is no CPU
    path behind it."""

    _INDEX_CACHE_MAX = 64

    def __init__(self, num_envs, device, track_pose=True):
        import torch
        if int(num_envs) != num_envs or int(num_envs) < 1:
            raise ValueError(f"num_envs must be a positive integer, got {num_envs!r}")
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:      # ("cuda" -> the current device, as tensors report it)
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.track_pose = bool(track_pose)
        E, dev = self.num_envs, self.device
        self.goal = torch.zeros((E, 3), dtype=torch.float64, device=dev)
        self.polar = torch.zeros((E, 2), dtype=torch.float32, device=dev)
        self.rot = self.pos = None
        if self.track_pose:
            self.rot = torch.zeros((E, 4), dtype=torch.float64, device=dev)
            self.rot[:, 3] = 1.0
            self.pos = torch.zeros((E, 3), dtype=torch.float64, device=dev)
        self._index_cache = {}

    # ------------------------------------------------------------------ argument checks (before anything is launched)
    def _check_indices(self, env_indices, n=None):
        try:
            idx = tuple(env_indices)
        except TypeError:
            raise ValueError(f"env_indices must be a sequence of environment indices, got {env_indices!r}") from None
        if n is not None and len(idx) != n:
            raise ValueError(f"{len(idx)} environment indices for {n} rows")
        for e in idx:
            if isinstance(e, (bool, np.bool_)) or not isinstance(e, (int, np.integer)):
                raise ValueError(f"environment index {e!r} is not an integer")
            if not 0 <= int(e) < self.num_envs:
                raise ValueError(f"environment index {int(e)} outside [0, {self.num_envs})")
        idx = tuple(int(e) for e in idx)
        if len(set(idx)) != len(idx):
            raise ValueError(f"environment indices must be distinct within a call, got {list(idx)}")
        return idx

    def _need_gpu(self):
        if self.device.type != "cuda":
            raise RuntimeError("GoalTracker runs its updates on an MI355X only (there is no CPU fallback); use compute_goal_pos_batch "
                               "/ compute_global_state on the host")

    def _device_indices(self, idx):
        """int32 device tensor of an index tuple, cached per tuple (the loop repeats a handful of them)."""
        import torch
        t = self._index_cache.get(idx)
        if t is None:
            if len(self._index_cache) >= self._INDEX_CACHE_MAX:
                self._index_cache.clear()
            t = self._index_cache[idx] = torch.tensor(idx, dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)
        return t

    @staticmethod
    def _ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    # ------------------------------------------------------------------ episode start and step
    def reset(self, env_indices, goal_positions, start_positions, start_rotations):
        """Episode start of the given environments (ppo_trainer.py:727-740), from host arrays: goal_positions [n,3] in the world
        frame, start_positions [n,3], start_rotations [n,4] as [x,y,z,w].  goal / polar rows become
        `compute_goal_pos(goal_position, (sx, sz, 2 atan2(r_y, r_w)))`, rot / pos rows the start pose.  The start delta is built
        here in numpy as the reference does; one pinned non-blocking upload, one launch."""
        import torch
        idx = self._check_indices(env_indices)
        n = len(idx)

        def host(a, cols, what):
            try:
                a = np.asarray(a, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"{what} must be a numeric array of shape ({n}, {cols})") from None
            if a.shape != (n, cols):
                raise ValueError(f"{what} must have shape ({n}, {cols}), got {a.shape}")
            return a

        goals = host(goal_positions, 3, "goal_positions")
        spos = host(start_positions, 3, "start_positions")
        srot = host(start_rotations, 4, "start_rotations")
        self._need_gpu()
        if n == 0:
            return
        # one pinned block: float64 goal [n,3] | start delta [n,3] | start rotation [n,4] | start position [n,3], then the int32
        # indices (torch's pinned allocator keeps the block alive until the copy below has run)
        h = torch.empty(n * 13 * 8 + n * 4, dtype=torch.uint8, pin_memory=True)
        hd = h[: n * 13 * 8].view(torch.float64).numpy()
        hd[0:3 * n].reshape(n, 3)[:] = goals
        delta = hd[3 * n:6 * n].reshape(n, 3)
        delta[:, 0] = spos[:, 0]
        delta[:, 1] = spos[:, 2]
        delta[:, 2] = 2 * np.arctan2(srot[:, 1], srot[:, 3])
        hd[6 * n:10 * n].reshape(n, 4)[:] = srot
        hd[10 * n:13 * n].reshape(n, 3)[:] = spos
        h[n * 13 * 8:].view(torch.int32).numpy()[:] = idx
        dev = self.device
        from . import _lib
        with torch.cuda.device(dev):
            d = h.to(dev, non_blocking=True)
            at = lambda doubles: C.c_void_p(d.data_ptr() + 8 * doubles)
            _lib.check(_lib.lib.pnvo_nav_reset(at(0), at(3 * n), at(6 * n), at(10 * n), at(13 * n), n, self._ptr(self.goal),
                                               self._ptr(self.rot), self._ptr(self.pos), self._ptr(self.polar),
                                               C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))

    def _check_deltas(self, deltas, env_indices):
        """Shape and dtype of an update's deltas and its indices -> (row count, index tuple or None for all environments)."""
        import torch
        if not isinstance(deltas, torch.Tensor):
            raise ValueError(f"deltas must be a CUDA float32 tensor [n,3], got {type(deltas).__name__}")
        if deltas.dim() != 2 or deltas.shape[1] != 3 or deltas.dtype != torch.float32:
            raise ValueError(f"deltas must be float32 [n,3], got {deltas.dtype} {tuple(deltas.shape)}")
        n = int(deltas.shape[0])
        if env_indices is None:
            if n != self.num_envs:
                raise ValueError(f"{n} delta rows for {self.num_envs} environments: pass env_indices to update a subset")
            return n, None
        return n, self._check_indices(env_indices, n)

    def update(self, deltas, env_indices=None):
        """One simulator step: row i of `deltas` — a CUDA float32 [n,3] tensor of (dx, dz, dyaw), any row stride, e.g. what
        `compute_local_delta_states_batch(..., to_host=False)` returns — advances environment env_indices[i] (all `num_envs`
        environments in order when env_indices is None).  Environments not named keep every byte of their state.  One launch on the
        current stream, no host wait; the index tensor of a repeated env_indices tuple is cached."""
        import torch
        n, idx = self._check_deltas(deltas, env_indices)
        if not deltas.is_cuda:
            raise ValueError("deltas must be a CUDA tensor (the host form of this update is compute_goal_pos_batch)")
        self._need_gpu()
        if deltas.device != self.device:
            raise ValueError(f"deltas are on {deltas.device}, the tracker on {self.device}")
        if n == 0:
            return
        if deltas.stride(1) != 1:
            deltas = deltas.contiguous()
        dev = self.device
        from . import _lib
        with torch.cuda.device(dev):
            env = self._device_indices(idx) if idx is not None else None
            _lib.check(_lib.lib.pnvo_nav_update(self._ptr(deltas), int(deltas.stride(0)) if n > 1 else 3, self._ptr(env), n,
                                                self._ptr(self.goal), self._ptr(self.rot), self._ptr(self.pos), self._ptr(self.polar),
                                                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))

    # ------------------------------------------------------------------ host copies (trajectory logging)
    def cartesian(self):
        """Host copy of the goal positions in the agent frames, float64 [E,3] (waits for the device)."""
        return self.goal.cpu().numpy()

    def global_state(self):
        """Host copies (rotations float64 [E,4] as [x,y,z,w], positions float64 [E,3]) of the pose from the VO (waits for the device)."""
        if not self.track_pose:
            raise RuntimeError("this GoalTracker was built with track_pose=False")
        return self.rot.cpu().numpy(), self.pos.cpu().numpy()


class EpisodeLog:
    """One ended episode of a `NavEvalStats(keep_trajectories=True)`: the environment, its step count (known on the host), and — copied
    asynchronously into pinned memory — its records float64 [steps,16] (delta[3], gt[3], std[3], rot[4], pos[3] after each step) and
    its diff row [3].  Reading `records` or `diff` waits for the copies' event; nothing else does."""

    def __init__(self, env, steps, records, diff, event):
        self.env, self.steps = env, steps
        self._records, self._diff, self._event = records, diff, event

    def _wait(self):
        if self._event is not None:
            self._event.synchronize()
            self._event = None

    @property
    def records(self):
        self._wait()
        return self._records.numpy()

    @property
    def diff(self):
        self._wait()
        return self._diff.numpy()


class NavEvalStats:
    """`NavEvalBook` on the device, around a `GoalTracker(track_pose=True)` whose pose IS the book's pose (csrc/nav_state.hip:
    pnvo_nav_update_eval / pnvo_nav_episode_end).  In the evaluation loop `update` takes the place of `tracker.update`, and
    `end_episodes` runs BEFORE `tracker.reset` of the same environments (stream order then lets it read the pose the episode ended
    with).  Both are one launch on the current stream and never wait for the device; `result()` waits once.

      steps    int64   [E]     VO steps of the running episode        abs_sum, std_sum  float64 [E,3]  its sums
      traj     float64 [E, max_episode_steps, 16]  (keep_trajectories) the running episode's records
      counts   int64   [2]     episodes, steps of the run             totals  float64 [3,3]  l2_sum, std_sum, diff_sum

    The host keeps a step counter of its own per environment (nothing is read back for it): it refuses a step beyond
    `max_episode_steps` before anything is launched and sizes the trajectory copies."""

    def __init__(self, tracker, max_episode_steps=500, keep_trajectories=False):
        import torch
        if not isinstance(tracker, GoalTracker) or not tracker.track_pose:
            raise ValueError("NavEvalStats needs a GoalTracker built with track_pose=True: the drift is measured on its pose")
        if int(max_episode_steps) != max_episode_steps or int(max_episode_steps) < 1:
            raise ValueError(f"max_episode_steps must be a positive integer, got {max_episode_steps!r}")
        self.tracker = tracker
        self.max_episode_steps = int(max_episode_steps)
        self.keep_trajectories = bool(keep_trajectories)
        E, dev = tracker.num_envs, tracker.device
        self.steps = torch.zeros(E, dtype=torch.int64, device=dev)
        self.abs_sum = torch.zeros((E, 3), dtype=torch.float64, device=dev)
        self.std_sum = torch.zeros((E, 3), dtype=torch.float64, device=dev)
        self.traj = (torch.zeros((E, self.max_episode_steps, TRAJ_RECORD), dtype=torch.float64, device=dev)
                     if self.keep_trajectories else None)
        self.counts = torch.zeros(2, dtype=torch.int64, device=dev)
        self.totals = torch.zeros((3, 3), dtype=torch.float64, device=dev)
        self._host_steps = np.zeros(E, dtype=np.int64)

    @staticmethod
    def _host_rows(a, n, cols, what):
        try:
            a = np.asarray(a, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{what} must be a numeric array of shape ({n}, {cols})") from None
        if a.shape != (n, cols):
            raise ValueError(f"{what} must have shape ({n}, {cols}), got {a.shape}")
        return a

    def update(self, deltas, gt_deltas, env_indices=None, stds=None):
        """`tracker.update(deltas, env_indices)` plus the book's step: gt_deltas is the simulator's float64 [n,3] (a host array: one
        pinned non-blocking upload), stds an optional CUDA float32 [n,3] tensor (zeros when None)."""
        import torch
        tr = self.tracker
        n, idx = tr._check_deltas(deltas, env_indices)
        gt = self._host_rows(gt_deltas, n, 3, "gt_deltas")
        if stds is not None:
            if not isinstance(stds, torch.Tensor) or stds.dtype != torch.float32 or tuple(stds.shape) != (n, 3):
                raise ValueError(f"stds must be a CUDA float32 tensor [{n},3] or None")
        rows = np.arange(n) if idx is None else np.asarray(idx, dtype=np.int64)
        over = rows[self._host_steps[rows] >= self.max_episode_steps]
        if over.size:
            raise ValueError(f"environments {over.tolist()} are already at max_episode_steps = {self.max_episode_steps}: "
                             "end their episodes first")
        if not deltas.is_cuda or (stds is not None and not stds.is_cuda):
            raise ValueError("deltas and stds must be CUDA tensors (the host form of this update is NavEvalBook.step)")
        tr._need_gpu()
        if deltas.device != tr.device or (stds is not None and stds.device != tr.device):
            raise ValueError(f"deltas / stds are not on the tracker's device {tr.device}")
        if n == 0:
            return
        if deltas.stride(1) != 1:
            deltas = deltas.contiguous()
        if stds is not None:
            stds = stds.contiguous()
        dev, p = tr.device, tr._ptr
        from . import _lib
        with torch.cuda.device(dev):
            env = tr._device_indices(idx) if idx is not None else None
            h = torch.empty((n, 3), dtype=torch.float64, pin_memory=True)
            h.numpy()[:] = gt
            g = h.to(dev, non_blocking=True)
            _lib.check(_lib.lib.pnvo_nav_update_eval(p(deltas), int(deltas.stride(0)) if n > 1 else 3, p(env), n, p(tr.goal), p(tr.rot),
                                                     p(tr.pos), p(tr.polar), p(g), p(stds), p(self.steps), p(self.abs_sum),
                                                     p(self.std_sum), p(self.traj), self.max_episode_steps,
                                                     C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        self._host_steps[rows] += 1                       # (only once the launch is enqueued: the counter mirrors the device's)

    def end_episodes(self, env_indices, sim_positions, sim_rotations):
        """Episode end of the named environments, in the order given, against the simulator's final pose (host arrays [n,3] and
        [n,4] as [x,y,z,w]) -> the diff rows as a device tensor float64 [n,3] (reading it waits, returning it does not); with
        keep_trajectories (that tensor, [one `EpisodeLog` per row])."""
        import torch
        tr = self.tracker
        idx = tr._check_indices(env_indices)
        n = len(idx)
        spos = self._host_rows(sim_positions, n, 3, "sim_positions")
        srot = self._host_rows(sim_rotations, n, 4, "sim_rotations")
        tr._need_gpu()
        if n == 0:
            diff = torch.empty((0, 3), dtype=torch.float64, device=tr.device)
            return (diff, []) if self.keep_trajectories else diff
        dev, p = tr.device, tr._ptr
        from . import _lib
        with torch.cuda.device(dev):
            env = tr._device_indices(idx)
            h = torch.empty(n * 7, dtype=torch.float64, pin_memory=True)
            h.numpy()[:3 * n].reshape(n, 3)[:] = spos
            h.numpy()[3 * n:].reshape(n, 4)[:] = srot
            d = h.to(dev, non_blocking=True)
            diff = torch.empty((n, 3), dtype=torch.float64, device=dev)
            stream = torch.cuda.current_stream(dev)
            _lib.check(_lib.lib.pnvo_nav_episode_end(p(env), n, p(d), C.c_void_p(d.data_ptr() + 8 * 3 * n), p(tr.rot), p(tr.pos),
                                                     p(self.steps), p(self.abs_sum), p(self.std_sum), p(self.counts),
                                                     C.c_void_p(self.counts.data_ptr() + 8), p(self.totals),
                                                     C.c_void_p(self.totals.data_ptr() + 24), C.c_void_p(self.totals.data_ptr() + 48),
                                                     p(diff), C.c_void_p(stream.cuda_stream)))
            ended = self._host_steps[list(idx)].copy()
            self._host_steps[list(idx)] = 0
            if not self.keep_trajectories:
                return diff
            hdiff = torch.empty((n, 3), dtype=torch.float64, pin_memory=True)
            hdiff.copy_(diff, non_blocking=True)
            recs = []
            for e, s in zip(idx, ended):                  # (the next update of e overwrites these rows only behind the copies)
                r = torch.empty((int(s), TRAJ_RECORD), dtype=torch.float64, pin_memory=True)
                if s:
                    r.copy_(self.traj[e, :int(s)], non_blocking=True)
                recs.append(r)
            event = torch.cuda.Event()
            event.record(stream)
            return diff, [EpisodeLog(e, int(s), r, hdiff[i], event) for i, (e, s, r) in enumerate(zip(idx, ended, recs))]

    def result(self):
        """The same dict as `NavEvalBook.result()`; one synchronising copy."""
        import torch
        self.tracker._need_gpu()
        flat = torch.cat([self.counts.to(torch.float64), self.totals.reshape(-1)]).cpu().numpy()   # (counts < 2^53: exact)
        return _eval_result(int(flat[0]), int(flat[1]), flat[2:5], flat[5:8], flat[8:11])
