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
//
// One thread per row, no atomics, no LDS.  float64 in the operation order of pointnav_vo_amd.geometry (compute_goal_pos_batch,
// _quat_rotate, _quat_mul).  This file is built with -ffp-contract=off: numpy rounds after every multiply and add (no a*b+c
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

}  // extern "C"
