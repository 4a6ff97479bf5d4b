// nav_state.hip — goal and pose bookkeeping of the navigation loop on the device, gfx950 only.
//
// Between two simulator steps the reference turns the VO estimate (dx, dz, dyaw) of every environment into the goal position in
// the new agent frame (geometry_utils.py:115-144, compute_goal_pos) and, for the trajectory log, into the global pose
// (:69-99, compute_global_state) — about thirty flops per environment, on the host.  Here the state stays on the device behind
// stateless entry points (pointers, a row count and a stream, no handle: the tensors are plain torch tensors owned by
// pointnav_vo_amd.geometry.GoalTracker), so the deltas of the VO forward never cross PCIe:
//
//   pnvo_nav_update   rows env[i] of goal / rot / pos / polar advance by float32 delta row i      ppo_trainer.py:843-871
//   pnvo_nav_reset    rows env[i] start an episode: goal from the world goal and the start delta   ppo_trainer.py:727-740
//   pnvo_nav_update_eval   the update, with the evaluation book's step in front: VO error, std, log  ppo_trainer.py:845-873
//   pnvo_nav_episode_end   drift against the simulator's pose, run totals, the book's rows cleared   ppo_trainer.py:742-805
//
// One thread per row (the episode end: one workgroup, rows spread over it, then one thread per component), no atomics, no LDS.
// float64 in the operation order of pointnav_vo_amd.geometry (compute_goal_pos_batch, _quat_rotate, _quat_mul).  This file is built with -ffp-contract=off: numpy rounds after every multiply and add (no a*b+c
// fusion), so everything except sin, cos, hypot and atan2 is bit-equal to the host functions.  The literal `* 0.0` and `+ 0.0`
// terms of those functions are kept: they decide the sign of a zero.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/pnvo.h"
#include "pnvo_model.h"

namespace {

constexpr int kThreads = 256;

// compute_goal_pos_batch: g' = q^-1 (g - [dx,0,dz]) q with q = rot_y(dyaw), written out for qv = (0, sin(-dyaw/2), 0);
// polar = (rho, -phi) of (-g'_z, g'_x) in float32.
__device__ inline void goal_step(const double g[3], double dx, double dz, double dyaw, double *goal_row, float *polar_row) {
  const double vx = g[0] - dx, vy = g[1] - 0.0, vz = g[2] - dz;
  const double h = dyaw / 2.0;
  const double qy = -sin(h), w = cos(h);
  const double tx = 2.0 * (qy * vz), tz = 2.0 * (-(qy * vx));
  const double cx = (vx + w * tx) + qy * tz;
  const double cy = (vy + w * 0.0) + 0.0;
  const double cz = (vz + w * tz) + (-(qy * tx));
  goal_row[0] = cx, goal_row[1] = cy, goal_row[2] = cz;
  const double rho = hypot(-cz, cx);
  const double phi = atan2(cx, -cz);
  polar_row[0] = (float)rho;
  polar_row[1] = (float)(-phi);
}

// compute_global_state: v2 = v1 + q1 [dx,0,dz] q1^-1 (_quat_rotate: v + w t + qv x t, t = 2 qv x v, the general cross product);
// q2 = q1 * rot_y(dyaw) (_quat_mul, the general product with b = (0, sin(dyaw/2), 0, cos(dyaw/2))).
__device__ inline void pose_step(double dx, double dz, double dyaw, double *rot_row, double *pos_row) {
  const double ax = rot_row[0], ay = rot_row[1], az = rot_row[2], aw = rot_row[3];
  const double v0 = dx, v1 = 0.0, v2 = dz;
  const double t0 = 2.0 * (ay * v2 - az * v1), t1 = 2.0 * (az * v0 - ax * v2), t2 = 2.0 * (ax * v1 - ay * v0);
  const double u0 = ay * t2 - az * t1, u1 = az * t0 - ax * t2, u2 = ax * t1 - ay * t0;
  pos_row[0] = pos_row[0] + ((v0 + aw * t0) + u0);
  pos_row[1] = pos_row[1] + ((v1 + aw * t1) + u1);
  pos_row[2] = pos_row[2] + ((v2 + aw * t2) + u2);
  const double h = dyaw / 2.0;
  const double bx = 0.0, by = sin(h), bz = 0.0, bw = cos(h);
  rot_row[0] = ((aw * bx + ax * bw) + ay * bz) - az * by;
  rot_row[1] = ((aw * by - ax * bz) + ay * bw) + az * bx;
  rot_row[2] = ((aw * bz + ax * by) - ay * bx) + az * bw;
  rot_row[3] = ((aw * bw - ax * bx) - ay * by) - az * bz;
}

struct UpdateArgs {
  const float *deltas;       // [n, >= 3] float32, row stride in floats
  int64_t delta_row_stride;
  const int32_t *env;        // [n] state rows, or null: rows 0..n-1
  int n;
  double *goal, *rot, *pos;  // [E,3], [E,4] or null, [E,3] or null
  float *polar;              // [E,2]
};

__global__ __launch_bounds__(kThreads) void nav_update_kernel(UpdateArgs a) {
  const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (i >= a.n) return;
  const int64_t e = a.env ? (int64_t)a.env[i] : (int64_t)i;
  if (e < 0) return;                                       // (validated by the caller; never dereferenced)
  const float *d = a.deltas + (int64_t)i * a.delta_row_stride;
  const double dx = (double)d[0], dz = (double)d[1], dyaw = (double)d[2];
  double *g = a.goal + e * 3;
  const double prev[3] = {g[0], g[1], g[2]};
  goal_step(prev, dx, dz, dyaw, g, a.polar + e * 2);
  if (a.rot) pose_step(dx, dz, dyaw, a.rot + e * 4, a.pos + e * 3);
}

struct ResetArgs {
  const double *goal_world, *start_delta, *start_rot, *start_pos;   // [n,3], [n,3], [n,4] or null, [n,3] or null
  const int32_t *env;
  int n;
  double *goal, *rot, *pos;
  float *polar;
};

__global__ __launch_bounds__(kThreads) void nav_reset_kernel(ResetArgs a) {
  const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (i >= a.n) return;
  const int64_t e = a.env ? (int64_t)a.env[i] : (int64_t)i;
  if (e < 0) return;
  const double *gw = a.goal_world + (int64_t)i * 3, *sd = a.start_delta + (int64_t)i * 3;
  const double world[3] = {gw[0], gw[1], gw[2]};
  goal_step(world, sd[0], sd[1], sd[2], a.goal + e * 3, a.polar + e * 2);
  if (a.rot) {
    for (int k = 0; k < 4; ++k) a.rot[e * 4 + k] = a.start_rot[(int64_t)i * 4 + k];
    for (int k = 0; k < 3; ++k) a.pos[e * 3 + k] = a.start_pos[(int64_t)i * 3 + k];
  }
}

// The evaluation book (geometry.NavEvalBook is the host form): per-environment sums of the running episode, run totals.
struct EvalUpdateArgs {
  UpdateArgs u;              // rot and pos are not null here
  const double *gt;          // [n,3]
  const float *std;          // [n,3] or null: zeros
  int64_t *steps;            // [E]
  double *abs_sum, *std_sum; // [E,3]
  double *traj;              // [E, max_steps, 16] or null
  int max_steps;
};

// NavEvalBook.step, then the two device functions of nav_update_kernel on the same values.
__global__ __launch_bounds__(kThreads) void nav_update_eval_kernel(EvalUpdateArgs a) {
  const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (i >= a.u.n) return;
  const int64_t e = a.u.env ? (int64_t)a.u.env[i] : (int64_t)i;
  if (e < 0) return;
  const float *d = a.u.deltas + (int64_t)i * a.u.delta_row_stride;
  const double dl[3] = {(double)d[0], (double)d[1], (double)d[2]};
  const double *gt = a.gt + (int64_t)i * 3;
  const double g3[3] = {gt[0], gt[1], gt[2]};
  double sd[3] = {0.0, 0.0, 0.0};
  if (a.std)
    for (int k = 0; k < 3; ++k) sd[k] = (double)a.std[(int64_t)i * 3 + k];
  for (int k = 0; k < 3; ++k) a.abs_sum[e * 3 + k] = a.abs_sum[e * 3 + k] + fabs(dl[k] - g3[k]);
  for (int k = 0; k < 3; ++k) a.std_sum[e * 3 + k] = a.std_sum[e * 3 + k] + sd[k];
  double *g = a.u.goal + e * 3;
  const double prev[3] = {g[0], g[1], g[2]};
  goal_step(prev, dl[0], dl[1], dl[2], g, a.u.polar + e * 2);
  double *rot = a.u.rot + e * 4, *pos = a.u.pos + e * 3;
  pose_step(dl[0], dl[1], dl[2], rot, pos);
  const int64_t s = a.steps[e];
  a.steps[e] = s + 1;
  if (a.traj && s >= 0 && s < (int64_t)a.max_steps) {
    double *r = a.traj + (e * (int64_t)a.max_steps + s) * 16;
    for (int k = 0; k < 3; ++k) r[k] = dl[k], r[3 + k] = g3[k], r[6 + k] = sd[k];
    for (int k = 0; k < 4; ++k) r[9 + k] = rot[k];
    for (int k = 0; k < 3; ++k) r[13 + k] = pos[k];
  }
}

struct EpisodeEndArgs {
  const int32_t *env;
  int n;
  const double *sim_pos, *sim_rot;   // [n,3], [n,4]
  const double *rot, *pos;           // the tracker's [E,4], [E,3]
  int64_t *steps;
  double *abs_sum, *std_sum;
  int64_t *episodes, *steps_total;
  double *l2_sum, *std_sum_total, *diff_sum;   // [3] each
  double *diff;                      // [n,3]
};

// ONE workgroup.  First the diff rows, spread over the threads (geometry.angle_between_quaternions: dq = conj(sim) * vo through
// _quat_mul, 2 atan2(|dq_xyz|, |dq_w|)); behind a barrier, which also makes the rows visible to the workgroup, thread k < 3 walks
// the rows in call order for component k of the three totals and thread 3 for the two counts, each clearing what it has read.
// The totals therefore do not depend on how the threads were scheduled.  Nothing after the barrier reads `steps` except thread 3.
__global__ __launch_bounds__(kThreads) void nav_episode_end_kernel(EpisodeEndArgs a) {
  const int tid = (int)threadIdx.x;
  for (int i = tid; i < a.n; i += kThreads) {
    const int64_t e = a.env ? (int64_t)a.env[i] : (int64_t)i;
    double out[3] = {0.0, 0.0, 0.0};
    if (e >= 0 && a.steps[e] >= 1) {
      const double *sp = a.sim_pos + (int64_t)i * 3, *sr = a.sim_rot + (int64_t)i * 4;
      const double *vp = a.pos + e * 3, *vr = a.rot + e * 4;
      out[0] = fabs(sp[0] - vp[0]);
      out[1] = fabs(sp[2] - vp[2]);
      const double ax = -sr[0], ay = -sr[1], az = -sr[2], aw = sr[3];
      const double bx = vr[0], by = vr[1], bz = vr[2], bw = vr[3];
      const double qx = ((aw * bx + ax * bw) + ay * bz) - az * by;
      const double qy = ((aw * by - ax * bz) + ay * bw) + az * bx;
      const double qz = ((aw * bz + ax * by) - ay * bx) + az * bw;
      const double qw = ((aw * bw - ax * bx) - ay * by) - az * bz;
      const double nrm = sqrt((qx * qx + qy * qy) + qz * qz);
      out[2] = 2.0 * atan2(nrm, fabs(qw));
    }
    for (int k = 0; k < 3; ++k) a.diff[(int64_t)i * 3 + k] = out[k];
  }
  __syncthreads();
  if (tid < 3) {
    double l2 = a.l2_sum[tid], sd = a.std_sum_total[tid], df = a.diff_sum[tid];
    for (int i = 0; i < a.n; ++i) {
      const int64_t e = a.env ? (int64_t)a.env[i] : (int64_t)i;
      if (e < 0) continue;
      l2 = l2 + a.abs_sum[e * 3 + tid];
      sd = sd + a.std_sum[e * 3 + tid];
      df = df + a.diff[(int64_t)i * 3 + tid];
      a.abs_sum[e * 3 + tid] = 0.0;
      a.std_sum[e * 3 + tid] = 0.0;
    }
    a.l2_sum[tid] = l2, a.std_sum_total[tid] = sd, a.diff_sum[tid] = df;
  } else if (tid == 3) {
    int64_t total = *a.steps_total, episodes = *a.episodes;
    for (int i = 0; i < a.n; ++i) {
      const int64_t e = a.env ? (int64_t)a.env[i] : (int64_t)i;
      if (e < 0) continue;
      total += a.steps[e];
      episodes += 1;
      a.steps[e] = 0;
    }
    *a.steps_total = total, *a.episodes = episodes;
  }
}

inline int bad(const char *fn, const char *what) { return pnvo_fail(nullptr, PNVO_ERR_ARG, std::string(fn) + ": " + what); }

}  // namespace

extern "C" {

int pnvo_nav_update(const float *deltas, int64_t delta_row_stride, const int32_t *env, int n, double *goal, double *rot, double *pos,
                    float *polar, void *stream) {
  if (!deltas || !goal || !polar) return bad("pnvo_nav_update", "null pointer");
  if ((rot == nullptr) != (pos == nullptr)) return bad("pnvo_nav_update", "rot and pos are tracked together: both or neither");
  if (n < 0) return bad("pnvo_nav_update", "negative row count");
  if (n == 0) return PNVO_OK;
  UpdateArgs a;
  a.deltas = deltas, a.delta_row_stride = delta_row_stride, a.env = env, a.n = n;
  a.goal = goal, a.rot = rot, a.pos = pos, a.polar = polar;
  hipLaunchKernelGGL(nav_update_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, a);
  HIPCHK(nullptr, hipGetLastError());
  return PNVO_OK;
}

int pnvo_nav_reset(const double *goal_world, const double *start_delta, const double *start_rot, const double *start_pos,
                   const int32_t *env, int n, double *goal, double *rot, double *pos, float *polar, void *stream) {
  if (!goal_world || !start_delta || !goal || !polar) return bad("pnvo_nav_reset", "null pointer");
  if ((rot == nullptr) != (pos == nullptr)) return bad("pnvo_nav_reset", "rot and pos are tracked together: both or neither");
  if (rot && (!start_rot || !start_pos)) return bad("pnvo_nav_reset", "a tracked pose needs start_rot and start_pos");
  if (n < 0) return bad("pnvo_nav_reset", "negative row count");
  if (n == 0) return PNVO_OK;
  ResetArgs a;
  a.goal_world = goal_world, a.start_delta = start_delta, a.start_rot = start_rot, a.start_pos = start_pos, a.env = env, a.n = n;
  a.goal = goal, a.rot = rot, a.pos = pos, a.polar = polar;
  hipLaunchKernelGGL(nav_reset_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, a);
  HIPCHK(nullptr, hipGetLastError());
  return PNVO_OK;
}

int pnvo_nav_update_eval(const float *deltas, int64_t delta_row_stride, const int32_t *env, int n, double *goal, double *rot,
                         double *pos, float *polar, const double *gt, const float *std, int64_t *steps, double *abs_sum,
                         double *std_sum, double *traj, int max_steps, void *stream) {
  if (!deltas || !goal || !polar || !gt || !steps || !abs_sum || !std_sum) return bad("pnvo_nav_update_eval", "null pointer");
  if (!rot || !pos) return bad("pnvo_nav_update_eval", "the evaluation book needs a tracked pose (rot and pos)");
  if (n < 0) return bad("pnvo_nav_update_eval", "negative row count");
  if (traj && max_steps < 1) return bad("pnvo_nav_update_eval", "a trajectory buffer needs max_steps >= 1");
  if (n == 0) return PNVO_OK;
  EvalUpdateArgs a;
  a.u.deltas = deltas, a.u.delta_row_stride = delta_row_stride, a.u.env = env, a.u.n = n;
  a.u.goal = goal, a.u.rot = rot, a.u.pos = pos, a.u.polar = polar;
  a.gt = gt, a.std = std, a.steps = steps, a.abs_sum = abs_sum, a.std_sum = std_sum, a.traj = traj, a.max_steps = max_steps;
  hipLaunchKernelGGL(nav_update_eval_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, a);
  HIPCHK(nullptr, hipGetLastError());
  return PNVO_OK;
}

int pnvo_nav_episode_end(const int32_t *env, int n, const double *sim_pos, const double *sim_rot, const double *rot,
                         const double *pos, int64_t *steps, double *abs_sum, double *std_sum, int64_t *episodes,
                         int64_t *steps_total, double *l2_sum, double *std_sum_total, double *diff_sum, double *diff, void *stream) {
  if (!sim_pos || !sim_rot || !rot || !pos || !steps || !abs_sum || !std_sum || !episodes || !steps_total || !l2_sum ||
      !std_sum_total || !diff_sum || !diff)
    return bad("pnvo_nav_episode_end", "null pointer");
  if (n < 0) return bad("pnvo_nav_episode_end", "negative row count");
  if (n == 0) return PNVO_OK;
  EpisodeEndArgs a;
  a.env = env, a.n = n, a.sim_pos = sim_pos, a.sim_rot = sim_rot, a.rot = rot, a.pos = pos;
  a.steps = steps, a.abs_sum = abs_sum, a.std_sum = std_sum, a.episodes = episodes, a.steps_total = steps_total;
  a.l2_sum = l2_sum, a.std_sum_total = std_sum_total, a.diff_sum = diff_sum, a.diff = diff;
  hipLaunchKernelGGL(nav_episode_end_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, a);
  HIPCHK(nullptr, hipGetLastError());
  return PNVO_OK;
}

}  // extern "C"
