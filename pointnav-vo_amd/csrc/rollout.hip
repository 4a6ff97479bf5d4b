// rollout.hip — device-resident RolloutStorage (pointnav_vo/rl/common/rollout_storage.py), gfx950 only.
//
// The reference's class is a set of [T+1, N, ...] tensors and four methods that are long chains of tiny torch ops.  Here each
// method is ONE launch over the small fields (plus one copy / gather per sensor), behind stateless entry points: pointers, sizes
// and a stream, no handle (the tensors stay plain torch tensors, owned by pointnav_vo_amd.rollout_storage.RolloutStorage).
//
//   pnvo_rollout_insert            the seven small fields of insert()                       rollout_storage.py:83-89
//   pnvo_rollout_after_update      hidden state, masks, prev_actions: row `step` -> row 0   :97-99
//   pnvo_rollout_compute_returns   GAE / discounted returns, backward scan over t           :102-120
//   pnvo_rollout_gather            the eight small fields of one minibatch, T-major         :143-199
//   pnvo_rollout_gather_frames     one sensor's frames of one minibatch, T-major            :146-149, :169-189
//
// This file is built with -ffp-contract=off: the returns are float32 in the reference's operation order with one rounding per
// operation (no a*b+c fusion), so they are bit-equal to the reference's torch result.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/pnvo.h"
#include "pnvo_model.h"

namespace {

constexpr int kThreads = 256;
constexpr size_t kLdsBudget = 64 * 1024;     // bytes of LDS one returns workgroup may stage into
constexpr int kMaxTile = 64;                 // environments per returns workgroup (one wave scans them, a lane each)
constexpr int kMinTile = 16;                 // narrower rows than 64 bytes are not worth staging: read global memory instead

inline unsigned grid_for(int64_t items, int per_block, int cap) {
  int64_t g = (items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  return (unsigned)(g < cap ? g : cap);
}

// compute units of the current device (the grid bound of the grid-stride kernels)
int device_cus() {
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cus[dev] == 0) {
    int n = 0;
    cus[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
  }
  return cus[dev];
}

// ------------------------------------------------------------------------------------------------ insert / after_update
struct InsertArgs {
  float *hidden_dst;                        // row step + 1 of recurrent_hidden_states
  int64_t *actions_dst, *prev_actions_dst;  // row step of actions, row step + 1 of prev_actions
  float *logp_dst, *value_dst, *rewards_dst, *masks_dst;   // rows step, step, step, step + 1
  const float *hidden, *logp, *value, *rewards, *masks;
  const int64_t *actions;
  int64_t hidden_row;                       // L * N * H
  int N;
};

__global__ __launch_bounds__(kThreads) void rollout_insert_kernel(InsertArgs a) {
  const int64_t total = a.hidden_row + a.N;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    if (i < a.hidden_row) {
      a.hidden_dst[i] = a.hidden[i];
    } else {
      const int n = (int)(i - a.hidden_row);
      const int64_t act = a.actions[n];
      a.actions_dst[n] = act;
      a.prev_actions_dst[n] = act;
      a.logp_dst[n] = a.logp[n];
      a.value_dst[n] = a.value[n];
      a.rewards_dst[n] = a.rewards[n];
      a.masks_dst[n] = a.masks[n];
    }
  }
}

__global__ __launch_bounds__(kThreads) void rollout_after_update_kernel(float *hidden, int64_t *prev_actions, float *masks,
                                                                        int64_t hidden_row, int N, int step) {
  const int64_t total = hidden_row + N;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    if (i < hidden_row) {
      hidden[i] = hidden[(int64_t)step * hidden_row + i];
    } else {
      const int n = (int)(i - hidden_row);
      prev_actions[n] = prev_actions[(int64_t)step * N + n];
      masks[n] = masks[(int64_t)step * N + n];
    }
  }
}

// ------------------------------------------------------------------------------------------------ returns
// One step of either recursion, in the reference's operation order (this file has no a*b+c fusion):
//   GAE      delta = (r[t] + (g * v[t+1]) * m[t+1]) - v[t];   gae = delta + (gt * m[t+1]) * gae;   ret[t] = gae + v[t]
//   plain    ret[t] = ((ret[t+1] * g) * m[t+1]) + r[t]
__device__ inline float gae_step(float r, float v, float v1, float m1, float g, float gt, float &gae) {
  const float delta = (r + (g * v1) * m1) - v;
  gae = delta + (gt * m1) * gae;
  return gae + v;
}
__device__ inline float plain_step(float r, float ret1, float m1, float g) { return ((ret1 * g) * m1) + r; }

struct ReturnsArgs {
  const float *rewards;      // [T, N]
  float *value_preds;        // [T+1, N]   (GAE writes row `step`)
  const float *masks;        // [T+1, N]
  float *returns;            // [T+1, N]
  const float *next_value;   // [N]
  int N, step, use_gae;
  float g, gt;               // float32(gamma), float32(gamma * tau)
  int tile_log2;             // staged form: environments per workgroup = 1 << tile_log2
};

// Staged form.  A workgroup owns a tile of E = 1 << tile_log2 consecutive environments.  All 256 threads load the tile's
// [step, E] slab of rewards and [step + 1, E] slabs of values and masks into LDS (a row's E floats are adjacent in memory: lanes
// walk them, rows are independent loads in flight together), the first E lanes scan backwards out of LDS — a lane per
// environment, consecutive lanes on consecutive banks — leaving ret[t] where r[t] was, and all threads store the rows back.
__global__ __launch_bounds__(kThreads) void rollout_returns_lds_kernel(ReturnsArgs a) {
  extern __shared__ float lds[];
  const int E = 1 << a.tile_log2, S = a.step, N = a.N;
  const int n0 = (int)blockIdx.x * E;
  float *r = lds;                           // [S + 1, E]: rewards, then returns (row S: the plain form's ret[step])
  float *v = r + (size_t)(S + 1) * E;       // [S + 1, E]
  float *m = v + (size_t)(S + 1) * E;       // [S + 1, E]
  const int rows = S + 1;
  for (int i = threadIdx.x; i < rows * E; i += kThreads) {
    const int t = i >> a.tile_log2, e = i & (E - 1), n = n0 + e;
    if (n >= N) continue;
    const bool last = t == S;
    const float nv = last ? a.next_value[n] : 0.f;
    r[i] = last ? nv : a.rewards[(int64_t)t * N + n];
    v[i] = (last && a.use_gae) ? nv : a.value_preds[(int64_t)t * N + n];
    m[i] = a.masks[(int64_t)t * N + n];
  }
  __syncthreads();
  const int e = threadIdx.x;
  if (e < E && n0 + e < N) {
    if (a.use_gae) {
      float gae = 0.f;
      for (int t = S - 1; t >= 0; --t)
        r[t * E + e] = gae_step(r[t * E + e], v[t * E + e], v[(t + 1) * E + e], m[(t + 1) * E + e], a.g, a.gt, gae);
    } else {
      float ret = r[S * E + e];
      for (int t = S - 1; t >= 0; --t) r[t * E + e] = ret = plain_step(r[t * E + e], ret, m[(t + 1) * E + e], a.g);
    }
  }
  __syncthreads();
  // GAE: returns[0, step) and value_preds[step] = next_value;  plain: returns[0, step]
  const int out_rows = a.use_gae ? S : S + 1;
  for (int i = threadIdx.x; i < rows * E; i += kThreads) {
    const int t = i >> a.tile_log2, e2 = i & (E - 1), n = n0 + e2;
    if (n >= N) continue;
    if (t < out_rows) a.returns[(int64_t)t * N + n] = r[i];
    if (t == S && a.use_gae) a.value_preds[(int64_t)S * N + n] = v[i];
  }
}

// Direct form, for a rollout too long for the LDS budget: a lane per environment reads global memory (adjacent lanes read adjacent
// floats of a row) one step ahead of the scan.
__global__ __launch_bounds__(kThreads) void rollout_returns_direct_kernel(ReturnsArgs a) {
  const int n = (int)blockIdx.x * kThreads + threadIdx.x, N = a.N, S = a.step;
  if (n >= N) return;
  const float nv = a.next_value[n];
  if (a.use_gae) {
    a.value_preds[(int64_t)S * N + n] = nv;
    float gae = 0.f, v1 = nv;
    for (int t = S - 1; t >= 0; --t) {
      const float v = a.value_preds[(int64_t)t * N + n];
      a.returns[(int64_t)t * N + n] = gae_step(a.rewards[(int64_t)t * N + n], v, v1, a.masks[(int64_t)(t + 1) * N + n], a.g, a.gt, gae);
      v1 = v;
    }
  } else {
    float ret = nv;
    a.returns[(int64_t)S * N + n] = ret;
    for (int t = S - 1; t >= 0; --t)
      a.returns[(int64_t)t * N + n] = ret = plain_step(a.rewards[(int64_t)t * N + n], ret, a.masks[(int64_t)(t + 1) * N + n], a.g);
  }
}

// ------------------------------------------------------------------------------------------------ minibatch gather
struct GatherArgs {
  const float *hidden;                      // row 0 of recurrent_hidden_states: [L, N, H]
  const int64_t *actions, *prev_actions;    // [T, N], [T+1, N]
  const float *value_preds, *returns, *masks, *logp, *adv;
  const int64_t *perm;                      // [N], the minibatch is perm[start, start + n_mb)
  int N, L, H, steps, start, n_mb;
  float *hidden_out;                        // [L, n_mb, H]
  int64_t *actions_out, *prev_actions_out;  // [steps * n_mb], row t * n_mb + j
  float *value_preds_out, *returns_out, *masks_out, *logp_out, *adv_out;
};

__global__ __launch_bounds__(kThreads) void rollout_gather_kernel(GatherArgs a) {
  const int64_t rows = (int64_t)a.steps * a.n_mb, hid = (int64_t)a.L * a.n_mb * a.H;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < rows + hid; i += (int64_t)gridDim.x * kThreads) {
    if (i < rows) {
      const int t = (int)(i / a.n_mb), j = (int)(i % a.n_mb);
      const int64_t ind = a.perm[a.start + j];
      if ((uint64_t)ind >= (uint64_t)a.N) continue;         // the host validates the permutation; never read out of bounds
      const int64_t s = (int64_t)t * a.N + ind;
      a.actions_out[i] = a.actions[s];
      a.prev_actions_out[i] = a.prev_actions[s];
      a.value_preds_out[i] = a.value_preds[s];
      a.returns_out[i] = a.returns[s];
      a.masks_out[i] = a.masks[s];
      a.logp_out[i] = a.logp[s];
      a.adv_out[i] = a.adv[s];
    } else {
      const int64_t k = i - rows;
      const int h = (int)(k % a.H), j = (int)((k / a.H) % a.n_mb), l = (int)(k / ((int64_t)a.H * a.n_mb));
      const int64_t ind = a.perm[a.start + j];
      if ((uint64_t)ind >= (uint64_t)a.N) continue;
      a.hidden_out[k] = a.hidden[((int64_t)l * a.N + ind) * a.H + h];
    }
  }
}

struct FramesArgs {
  const float *src;          // [>= steps, N, F]
  const int64_t *perm;
  float *dst;                // [steps * n_mb, F], frame t * n_mb + j = src[t, perm[start + j]]
  int64_t F;
  int N, steps, start, n_mb;
};

// 16-byte form (F % 4 == 0, both bases 16-byte aligned).  The work is cut into (frame, chunk of 4 x 256 float4) units and the
// grid strides over the units, so a handful of large frames fills the chip as well as many small ones; a thread has four
// independent 16-byte loads in flight.
constexpr int kVecPerThread = 4;
constexpr int kChunkVec = kThreads * kVecPerThread;

__global__ __launch_bounds__(kThreads) void rollout_gather_frames_vec_kernel(FramesArgs a) {
  const int64_t F4 = a.F / 4, chunks = (F4 + kChunkVec - 1) / kChunkVec, units = (int64_t)a.steps * a.n_mb * chunks;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t frame = u / chunks, c0 = (u % chunks) * kChunkVec;
    const int t = (int)(frame / a.n_mb), j = (int)(frame % a.n_mb);
    const int64_t ind = a.perm[a.start + j];
    if ((uint64_t)ind >= (uint64_t)a.N) continue;
    const float4 *s = reinterpret_cast<const float4 *>(a.src + ((int64_t)t * a.N + ind) * a.F);
    float4 *d = reinterpret_cast<float4 *>(a.dst + frame * a.F);
    float4 x[kVecPerThread];
#pragma unroll
    for (int k = 0; k < kVecPerThread; ++k) {
      const int64_t c = c0 + k * kThreads + threadIdx.x;
      if (c < F4) x[k] = s[c];
    }
#pragma unroll
    for (int k = 0; k < kVecPerThread; ++k) {
      const int64_t c = c0 + k * kThreads + threadIdx.x;
      if (c < F4) d[c] = x[k];
    }
  }
}

__global__ __launch_bounds__(kThreads) void rollout_gather_frames_scalar_kernel(FramesArgs a) {
  const int64_t total = (int64_t)a.steps * a.n_mb * a.F;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t frame = i / a.F, f = i % a.F;
    const int t = (int)(frame / a.n_mb), j = (int)(frame % a.n_mb);
    const int64_t ind = a.perm[a.start + j];
    if ((uint64_t)ind >= (uint64_t)a.N) continue;
    a.dst[i] = a.src[((int64_t)t * a.N + ind) * a.F + f];
  }
}

inline int bad(const char *fn, const char *what) { return pnvo_fail(nullptr, PNVO_ERR_ARG, std::string(fn) + ": " + what); }

}  // namespace

extern "C" {

int pnvo_rollout_insert(float *recurrent_hidden_states, int64_t *actions, int64_t *prev_actions, float *action_log_probs,
                        float *value_preds, float *rewards, float *masks, int T, int N, int64_t hidden_row, int step,
                        const float *hidden_in, const int64_t *actions_in, const float *action_log_probs_in,
                        const float *value_preds_in, const float *rewards_in, const float *masks_in, void *stream) {
  if (!recurrent_hidden_states || !actions || !prev_actions || !action_log_probs || !value_preds || !rewards || !masks ||
      !hidden_in || !actions_in || !action_log_probs_in || !value_preds_in || !rewards_in || !masks_in)
    return bad("pnvo_rollout_insert", "null pointer");
  if (T <= 0 || N <= 0 || hidden_row <= 0) return bad("pnvo_rollout_insert", "num_steps, num_envs and the hidden row size must be positive");
  if (step < 0 || step >= T) return bad("pnvo_rollout_insert", "step outside [0, num_steps): the storage is full");
  InsertArgs a;
  a.hidden_dst = recurrent_hidden_states + (int64_t)(step + 1) * hidden_row;
  a.actions_dst = actions + (int64_t)step * N;
  a.prev_actions_dst = prev_actions + (int64_t)(step + 1) * N;
  a.logp_dst = action_log_probs + (int64_t)step * N;
  a.value_dst = value_preds + (int64_t)step * N;
  a.rewards_dst = rewards + (int64_t)step * N;
  a.masks_dst = masks + (int64_t)(step + 1) * N;
  a.hidden = hidden_in, a.logp = action_log_probs_in, a.value = value_preds_in, a.rewards = rewards_in, a.masks = masks_in;
  a.actions = actions_in;
  a.hidden_row = hidden_row, a.N = N;
  const unsigned grid = grid_for(hidden_row + N, kThreads, 4 * device_cus());
  hipLaunchKernelGGL(rollout_insert_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, a);
  HIPCHK(nullptr, hipGetLastError());
  return PNVO_OK;
}

int pnvo_rollout_after_update(float *recurrent_hidden_states, int64_t *prev_actions, float *masks, int T, int N, int64_t hidden_row,
                              int step, void *stream) {
  if (!recurrent_hidden_states || !prev_actions || !masks) return bad("pnvo_rollout_after_update", "null pointer");
  if (T <= 0 || N <= 0 || hidden_row <= 0)
    return bad("pnvo_rollout_after_update", "num_steps, num_envs and the hidden row size must be positive");
  if (step < 0 || step > T) return bad("pnvo_rollout_after_update", "step outside [0, num_steps]");
  if (step == 0) return PNVO_OK;                         // row 0 onto itself
  const unsigned grid = grid_for(hidden_row + N, kThreads, 4 * device_cus());
  hipLaunchKernelGGL(rollout_after_update_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, recurrent_hidden_states,
                     prev_actions, masks, hidden_row, N, step);
  HIPCHK(nullptr, hipGetLastError());
  return PNVO_OK;
}

int pnvo_rollout_compute_returns(const float *rewards, float *value_preds, const float *masks, float *returns, const float *next_value,
                                 int T, int N, int step, int use_gae, float gamma, float gamma_tau, void *stream) {
  if (!rewards || !value_preds || !masks || !returns || !next_value) return bad("pnvo_rollout_compute_returns", "null pointer");
  if (T <= 0 || N <= 0) return bad("pnvo_rollout_compute_returns", "num_steps and num_envs must be positive");
  if (step < 0 || step > T) return bad("pnvo_rollout_compute_returns", "step outside [0, num_steps]");
  ReturnsArgs a;
  a.rewards = rewards, a.value_preds = value_preds, a.masks = masks, a.returns = returns, a.next_value = next_value;
  a.N = N, a.step = step, a.use_gae = use_gae ? 1 : 0, a.g = gamma, a.gt = gamma_tau, a.tile_log2 = 0;
  // the widest tile (a power of two, no wider than the environments need) whose three [step + 1, E] slabs fit the budget
  int cover = 0;
  while ((1 << cover) < N && (1 << cover) < kMaxTile) ++cover;
  const int floor_log2 = (1 << cover) < kMinTile ? cover : 4;      // log2(kMinTile)
  int tl = cover;
  auto bytes = [&](int l) { return (size_t)3 * (step + 1) * ((size_t)1 << l) * sizeof(float); };
  while (tl > floor_log2 && bytes(tl) > kLdsBudget) --tl;
  if (bytes(tl) <= kLdsBudget) {
    a.tile_log2 = tl;
    const unsigned grid = (unsigned)((N + (1 << tl) - 1) >> tl);
    hipLaunchKernelGGL(rollout_returns_lds_kernel, dim3(grid), dim3(kThreads), bytes(tl), (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(rollout_returns_direct_kernel, dim3((N + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, a);
  }
  HIPCHK(nullptr, hipGetLastError());
  return PNVO_OK;
}

int pnvo_rollout_gather(const float *recurrent_hidden_states, const int64_t *actions, const int64_t *prev_actions,
                        const float *value_preds, const float *returns, const float *masks, const float *action_log_probs,
                        const float *advantages, const int64_t *perm, int N, int L, int H, int steps, int start, int n_mb,
                        float *hidden_out, int64_t *actions_out, int64_t *prev_actions_out, float *value_preds_out, float *returns_out,
                        float *masks_out, float *action_log_probs_out, float *advantages_out, void *stream) {
  if (!recurrent_hidden_states || !actions || !prev_actions || !value_preds || !returns || !masks || !action_log_probs ||
      !advantages || !perm || !hidden_out || !actions_out || !prev_actions_out || !value_preds_out || !returns_out || !masks_out ||
      !action_log_probs_out || !advantages_out)
    return bad("pnvo_rollout_gather", "null pointer");
  if (N <= 0 || L <= 0 || H <= 0 || steps <= 0 || n_mb <= 0) return bad("pnvo_rollout_gather", "sizes must be positive");
  if (start < 0 || (int64_t)start + n_mb > N) return bad("pnvo_rollout_gather", "minibatch [start, start + n_mb) outside the permutation");
  GatherArgs a;
  a.hidden = recurrent_hidden_states, a.actions = actions, a.prev_actions = prev_actions, a.value_preds = value_preds;
  a.returns = returns, a.masks = masks, a.logp = action_log_probs, a.adv = advantages, a.perm = perm;
  a.N = N, a.L = L, a.H = H, a.steps = steps, a.start = start, a.n_mb = n_mb;
  a.hidden_out = hidden_out, a.actions_out = actions_out, a.prev_actions_out = prev_actions_out, a.value_preds_out = value_preds_out;
  a.returns_out = returns_out, a.masks_out = masks_out, a.logp_out = action_log_probs_out, a.adv_out = advantages_out;
  const int64_t items = (int64_t)steps * n_mb + (int64_t)L * n_mb * H;
  hipLaunchKernelGGL(rollout_gather_kernel, dim3(grid_for(items, kThreads, 4 * device_cus())), dim3(kThreads), 0, (hipStream_t)stream, a);
  HIPCHK(nullptr, hipGetLastError());
  return PNVO_OK;
}

int pnvo_rollout_gather_frames(const float *frames, const int64_t *perm, int N, int64_t F, int steps, int start, int n_mb, float *out,
                               void *stream) {
  if (!frames || !perm || !out) return bad("pnvo_rollout_gather_frames", "null pointer");
  if (N <= 0 || F <= 0 || steps <= 0 || n_mb <= 0) return bad("pnvo_rollout_gather_frames", "sizes must be positive");
  if (start < 0 || (int64_t)start + n_mb > N)
    return bad("pnvo_rollout_gather_frames", "minibatch [start, start + n_mb) outside the permutation");
  FramesArgs a;
  a.src = frames, a.perm = perm, a.dst = out, a.F = F, a.N = N, a.steps = steps, a.start = start, a.n_mb = n_mb;
  const int cus = device_cus();
  const bool vec = F % 4 == 0 && (reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(out)) % 16 == 0;
  if (vec) {
    const int64_t units = (int64_t)steps * n_mb * ((F / 4 + kChunkVec - 1) / kChunkVec);
    hipLaunchKernelGGL(rollout_gather_frames_vec_kernel, dim3(grid_for(units, 1, 8 * cus)), dim3(kThreads), 0, (hipStream_t)stream, a);
  } else {
    const int64_t total = (int64_t)steps * n_mb * F;
    hipLaunchKernelGGL(rollout_gather_frames_scalar_kernel, dim3(grid_for(total, kThreads, 8 * cus)), dim3(kThreads), 0,
                       (hipStream_t)stream, a);
  }
  HIPCHK(nullptr, hipGetLastError());
  return PNVO_OK;
}

}  // extern "C"
