"""Shared by tests/test_nav_eval_host.py and tests/test_gpu_nav_eval.py (not a test module):

  * `ListReference` — the evaluation loop's VO bookkeeping in the reference's own LIST-APPEND form (rl/ppo/ppo_trainer.py:742-805,
    845-873, 1104-1128), restated in this project's words: per-environment Python lists, reduced with np.mean / np.sum(..., axis=0)
    and zip(*...).  `geometry.NavEvalBook` keeps running sums instead; the two must agree to rounding.  It is independent of the
    book in the summing and the bookkeeping only: the pose step and the yaw angle are `geometry.compute_global_state` and
    `geometry.angle_between_quaternions` on both sides (habitat and numpy-quaternion are absent, so there is no second
    implementation to call); those two rest on their own property tests (tests/test_geometry.py, test_angle_between_quaternions).
  * `make_run` — a scripted evaluation run: which environments end and which step at every loop step, with seeded inputs.
  * `drive` — feeds a run to anything with the book's reset / step / end_episodes interface.
"""
import functools

import numpy as np

from pointnav_vo_amd import geometry
from test_gpu_goal_tracker import make_deltas, make_goals, yaw_quat


class ListReference:
    def __init__(self, num_envs):
        self.prev_global_state_from_vo = [None] * num_envs
        self.vo_l2_losses = [[] for _ in range(num_envs)]
        self.vo_pred_stds = [[] for _ in range(num_envs)]
        self.cur_agent_state_from_vo = [None] * num_envs
        self.all_vo_l2_losses, self.all_vo_pred_stds, self.all_diff_between_global_states = [], [], []

    def reset(self, env_indices, start_positions, start_rotations):
        for i, e in enumerate(env_indices):                                               # :737-740
            self.prev_global_state_from_vo[e] = (np.array(start_rotations[i]), np.array(start_positions[i]))

    def step(self, env_indices, deltas, gt_deltas, stds=None):
        for i, e in enumerate(env_indices):
            local_delta_states = [float(v) for v in deltas[i]]                            # the VO's floats, as a list
            std = [0.0, 0.0, 0.0] if stds is None else [float(v) for v in stds[i]]
            self.vo_l2_losses[e].append(np.abs(np.array(local_delta_states) - np.array(gt_deltas[i])))   # :845-847
            self.vo_pred_stds[e].append(std)                                              # :848
            cur = geometry.compute_global_state(self.prev_global_state_from_vo[e], local_delta_states)   # :864-866
            self.cur_agent_state_from_vo[e] = cur                                         # :867-870
            self.prev_global_state_from_vo[e] = cur                                       # :871

    def end_episodes(self, env_indices, sim_positions, sim_rotations):
        rows = []
        for i, e in enumerate(env_indices):
            if len(self.vo_l2_losses[e]) > 0:             # (the reference asks len(eval_traj_infos[i]) > 1: at least one VO step)
                self.all_vo_l2_losses.append((len(self.vo_l2_losses[e]), np.sum(np.array(self.vo_l2_losses[e]), axis=0)))   # :747-752
                self.all_vo_pred_stds.append((len(self.vo_pred_stds[e]), np.sum(np.array(self.vo_pred_stds[e]), axis=0)))   # :755-760
                rot, pos = self.cur_agent_state_from_vo[e]
                diff_pos = np.abs(np.array(sim_positions[i]) - np.array(pos))             # :768-771
                diff_yaw = geometry.angle_between_quaternions(sim_rotations[i], rot)      # :772-774
                rows.append([diff_pos[0], diff_pos[2], diff_yaw])                         # :776-783
            else:                                                                         # :789-805
                self.all_vo_l2_losses.append((0, (0.0, 0.0, 0.0)))
                self.all_vo_pred_stds.append((0, (0.0, 0.0, 0.0)))
                rows.append([0.0, 0.0, 0.0])
            self.all_diff_between_global_states.append(rows[-1])
            self.vo_l2_losses[e], self.vo_pred_stds[e] = [], []
        return np.array(rows, dtype=np.float64).reshape(len(rows), 3)

    def result(self):
        l2 = list(zip(*self.all_vo_l2_losses))                                            # :1106-1109
        all_steps = np.sum(l2[0])
        loss_sum = np.sum(np.array(l2[1]), axis=0)
        stds = list(zip(*self.all_vo_pred_stds))                                          # :1119-1121
        pred_std_sum = np.sum(np.array(stds[1]), axis=0)
        avg_diff = np.mean(np.array(self.all_diff_between_global_states), axis=0)         # :1124
        return {"vo_l2_loss": loss_sum / all_steps, "vo_pred_std": pred_std_sum / all_steps, "vo_l2_gloabl_state": avg_diff,
                "episodes": len(self.all_diff_between_global_states), "steps": int(all_steps)}


# The 5-environment script: loop step -> the environments that end there, IN THIS ORDER.  Environment 1 ends after its first loop
# step (an episode of zero VO steps), 3 and 2 end together in step 6, 4 runs two full episodes, and everything ends after step 12.
SMALL_ENDS = {0: [1], 4: [4], 6: [3, 2], 10: [4]}
SMALL_SEED = 0


def make_run(E, T, ends, seed, with_std=True):
    """-> {"E", "start": (goals, pos, rot), "loop": [one dict per loop step]}.  A loop step first ends `ended` (with the simulator's
    pose `sim_pos` / `sim_rot` of those rows and the start `new_goal` / `new_pos` / `new_rot` of their next episodes), then steps the
    `live` environments — every other one, as a shuffled index tuple — with float32 `deltas`, float64 `gt` = delta + noise and
    float32 `stds` (None without with_std).  The simulator's pose is the ground truth deltas integrated from the start pose.  After
    the last loop step every environment ends, in a shuffled order (`final`)."""
    rng = np.random.default_rng(seed)
    goals = make_goals(E, rng)
    pos = rng.uniform(-3.0, 3.0, size=(E, 3))
    rot = yaw_quat(rng.uniform(-np.pi, np.pi, size=E))
    run = {"E": E, "start": (goals.copy(), pos.copy(), rot.copy()), "loop": []}

    def ending(rows):
        k = len(rows)
        out = {"ended": [int(e) for e in rows], "sim_pos": pos[rows].copy(), "sim_rot": rot[rows].copy(), "new_goal": make_goals(k, rng),
               "new_pos": rng.uniform(-3.0, 3.0, size=(k, 3)), "new_rot": yaw_quat(rng.uniform(-np.pi, np.pi, size=k))}
        pos[rows], rot[rows] = out["new_pos"], out["new_rot"]
        return out

    for t in range(T):
        step = ending(list(ends.get(t, [])))
        live = rng.permutation([e for e in range(E) if e not in step["ended"]])
        n = len(live)
        deltas = make_deltas(n, 1, rng)[0]
        gt = deltas.astype(np.float64) + rng.normal(0.0, 0.01, size=(n, 3))
        for i, e in enumerate(live):
            rot[e], pos[e] = geometry.compute_global_state((rot[e], pos[e]), gt[i])
        step.update(live=tuple(int(e) for e in live), deltas=deltas, gt=gt,
                    stds=rng.uniform(0.001, 0.05, size=(n, 3)).astype(np.float32) if with_std else None)
        run["loop"].append(step)
    run["final"] = ending(list(rng.permutation(E)))
    return run


@functools.lru_cache(maxsize=None)
def small_run():
    """The scripted run of both test files (read only)."""
    return make_run(5, 12, SMALL_ENDS, SMALL_SEED)


def drive(run, book, reverse_at=None, on_step=None, on_end=None):
    """The run on `book` -> [(ended rows, what end_episodes returned)] in call order.  reverse_at: feed that loop step's ended
    rows in reversed order.  on_step(step) / on_end(ending, rows, returned) are called after each call (the GPU test compares
    there)."""
    out = []
    _, pos, rot = run["start"]
    book.reset(range(run["E"]), pos, rot)

    def end(ending, reverse=False):
        rows = list(ending["ended"])
        if not rows:
            return
        order = list(range(len(rows)))[::-1] if reverse else list(range(len(rows)))
        got = book.end_episodes([rows[i] for i in order], ending["sim_pos"][order], ending["sim_rot"][order])
        out.append(([rows[i] for i in order], got))
        if on_end is not None:
            on_end(ending, order, got)
        book.reset([rows[i] for i in order], ending["new_pos"][order], ending["new_rot"][order])

    for t, step in enumerate(run["loop"]):
        end(step, reverse=(t == reverse_at))
        book.step(step["live"], step["deltas"], step["gt"], step["stds"])
        if on_step is not None:
            on_step(step)
    end(run["final"])
    return out
