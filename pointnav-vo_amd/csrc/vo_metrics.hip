// The regression metrics of a VO evaluation pass on the device (pnvo_vo_metrics in include/pnvo.h).
//
// What the reference accumulates per action model, per data type and per delta component while it evaluates
// (pointnav_vo/vo/engine/vo_cnn_engine.py:135-198 _compute_loss, called by _compute_and_update_info,
// vo_cnn_regression_geo_invariance_engine.py:1259-1311, from _process_one_batch :618-751): every (action model, data type)
// subset of a batch is one SLOT of a table, and for each slot and each d in (dx, dz, dyaw), over the slot's entries S:
//
//   loss             = mean_S(diff^2 * [mask for dz] * w_d)
//   abs_diff         = mean(sqrt(diff^2 * [mask]))          for dz over the entries of S with mask == 1 only
//   target_magnitude = mean|target| + 1e-8                  over the same entries as abs_diff
//   relative_diff    = abs_diff / target_magnitude
//   dz without a mask == 1 entry: abs_diff = 0, target_magnitude = 1e-8, relative_diff = 0 (loss stays the mean over S)
//   table[slot][d][0..3] += multiplier * {loss, abs_diff, target_magnitude, relative_diff};  count[slot] += |S|
//
// Departure from the reference: a slot WITHOUT entries adds nothing and keeps its count (the reference takes the mean of an
// empty tensor there and carries NaN into its totals).
//
// One workgroup.  A batch is a few hundred entries and a table has at most kMaxSlots rows, so the kernel walks the slots one
// after the other: every thread adds up its strided share of the batch in float64, the partials meet in a fixed LDS tree, thread
// 0 finishes the slot.  No atomics, one summation order: two launches on the same inputs give the same bits.  Slot values are
// only ever COMPARED with the slot being summed, never used as an index, so -1 and any other value outside [0, n_slots) belong
// to no row.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/pnvo.h"
#include "pnvo_model.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSums = 11;      // per d: sum of the loss term, of sqrt(.), of |target| (9), then |S| and the dz mask == 1 count
constexpr double kEpsilon = 1e-8;      // common_vars.py EPSILON

struct MetricsArgs {
  const float *pred, *target, *weights, *dz_mask;
  const int32_t *slot;
  int M, n_slots;
  double multiplier;
  double *table;
  int64_t *count;
};

__global__ __launch_bounds__(kThreads) void vo_metrics_kernel(const MetricsArgs a) {
  __shared__ double red[kSums][kThreads];
  const int t = threadIdx.x;
  for (int s = 0; s < a.n_slots; ++s) {
    double acc[kSums];
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
    for (int e = t; e < a.M; e += kThreads) {
      if (a.slot[e] != s) continue;
      const double m = a.dz_mask ? (double)a.dz_mask[e] : 1.0;
      for (int d = 0; d < 3; ++d) {
        const size_t i = (size_t)e * 3 + d;
        const double tg = (double)a.target[i];
        const double df = tg - (double)a.pred[i];
        const double w = a.weights ? (double)a.weights[i] : 1.0;
        const double sq = d == 1 ? m * (df * df) : df * df;
        acc[3 * d] += sq * w;
        if (d != 1 || m == 1.0) {
          acc[3 * d + 1] += sqrt(sq);
          acc[3 * d + 2] += fabs(tg);
        }
      }
      acc[9] += 1.0;
      if (m == 1.0) acc[10] += 1.0;
    }
    for (int k = 0; k < kSums; ++k) red[k][t] = acc[k];
    __syncthreads();
    for (int o = kThreads / 2; o >= 1; o >>= 1) {
      if (t < o)
        for (int k = 0; k < kSums; ++k) red[k][t] += red[k][t + o];
      __syncthreads();
    }
    if (t == 0 && red[9][0] > 0.0) {
      const double n = red[9][0];
      for (int d = 0; d < 3; ++d) {
        const double nd = d == 1 ? red[10][0] : n;
        const double loss = red[3 * d][0] / n;
        const double abs_diff = nd > 0.0 ? red[3 * d + 1][0] / nd : 0.0;
        const double magnitude = (nd > 0.0 ? red[3 * d + 2][0] / nd : 0.0) + kEpsilon;
        double *row = a.table + ((size_t)s * 3 + d) * 4;
        row[0] += a.multiplier * loss;
        row[1] += a.multiplier * abs_diff;
        row[2] += a.multiplier * magnitude;
        row[3] += a.multiplier * (abs_diff / magnitude);
      }
      a.count[s] += (int64_t)n;
    }
    __syncthreads();      // red is rewritten by the next slot
  }
}

inline int bad(const char *what) { return pnvo_fail(nullptr, PNVO_ERR_ARG, std::string("pnvo_vo_metrics: ") + what); }

}  // namespace

extern "C" {

int pnvo_vo_metrics(const float *pred, const float *target, const int32_t *slot, const float *weights, const float *dz_mask, int M,
                    int n_slots, float multiplier, double *table, int64_t *count, void *stream) {
  if (!pred || !target || !slot || !table || !count) return bad("null pointer");
  if (M <= 0) return bad("a batch needs at least one entry");
  if (n_slots <= 0 || n_slots > PNVO_VO_METRICS_MAX_SLOTS) return bad("n_slots outside 1..PNVO_VO_METRICS_MAX_SLOTS");
  MetricsArgs a;
  a.pred = pred, a.target = target, a.weights = weights, a.dz_mask = dz_mask, a.slot = slot;
  a.M = M, a.n_slots = n_slots, a.multiplier = (double)multiplier, a.table = table, a.count = count;
  hipLaunchKernelGGL(vo_metrics_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, a);
  HIPCHK(nullptr, hipGetLastError());
  return PNVO_OK;
}

}  // extern "C"
