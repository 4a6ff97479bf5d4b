// ppo_core.hip — the PPO minibatch update's shared core (pnvo_ppo_core.h), gfx950 only, float32: what the ResNet policy
// (policy_train.hip) and the baseline policy (simple_cnn_train.hip) both run once their recurrent core's input rows x exist.
//
//   forward  : per layer G_x = X . W_ih^T + bias over all M = T*N rows            gemm_f32_kernel (v_mfma_f32_32x32x2_f32)
//              T launches of lstm_step_kernel / gru_step_kernel (the only sequential part): gates, (c,) h, masked h_prev kept
//              -> logits / value / log pi(a) / entropy per row                     heads_eval_kernel
//   ppo_loss : clipped surrogate, clipped or plain value loss, entropy mean; d total / d logits, d total / d value   ppo_loss_kernel
//   backward : heads -> per layer (top first) T launches of bptt_step_kernel / gru_bptt_step_kernel, then dW_ih / dW_hh / dX as GEMMs
//              over all rows and the bias gradients as column sums
//   clip     : sumsq_kernel, clip_scale_kernel
// Rows are T-major (row t*N + n: the order RolloutStorage.recurrent_generator yields), weights in torch's [G*H][K] layouts read straight
// from the caller's flat parameter buffer.  Every reduction runs in a fixed order (no float atomics): the same call gives the same bits
// twice.  Masking h and c at EVERY step equals the reference's segment-wise masking (model_utils/rnns/rnn_state_encoder.py:81-134):
// inside a segment all masks are 1.
//
// LSTM (gate order i, f, g, o; state [2L, N, H]): b_ih + b_hh both ride on the input GEMM; dW_ih = dG^T . X, dW_hh = dG^T . hm,
// db_ih = db_hh = colsum(dG), dX = dG . W_ih.
// GRU (torch.nn.GRU, gate order r, z, n; weights [3H][K]; state [L, N, H], h only): G_x = X . W_ih^T + b_ih ONLY (b_hn sits inside the
// product with r, so b_hh cannot ride on the input GEMM); gru_step_kernel adds the recurrent products and b_hh and keeps
// (r, z, n, q = W_hn hm + b_hn), y and hm per row.  gru_bptt_step_kernel fills dGx = (dr, dz, dn) and dGh = (dr, dz, dn * r);
// dW_ih = dGx^T . X, dW_hh = dGh^T . hm, db_ih = colsum(dGx), db_hh = colsum(dGh), dX = dGx . W_ih.
// The type is branched on per launch, on the host: one loop over the layers and the steps serves both.
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/pnvo.h"
#include "pnvo_internal.h"
#include "pnvo_model.h"
#include "pnvo_policy_state.h"
#include "pnvo_ppo_core.h"

namespace pnvo {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int SQ_BLOCKS = 1024;       // clip_grad_norm's partial sums

// ------------------------------------------------------------------------------------------------------------ float32 GEMM
// C[m][n] = sum_k A(m,k) B(k,n) (+ bias0[n] + bias1[n]) on the exact-float32 matrix instruction (one k-ordered fmaf chain per output,
// as conv_mfma.hip): workgroup = 64 x 64 outputs, wave = 32 x 32, K in steps of 32 staged through LDS as [k][m] / [k][n].  Both
// operands are addressed by two strides, so the four products of the LSTM (X . W^T, dG^T . X, dG . W) are one kernel; AKC / BKC say
// which index is contiguous in memory (k, else m / n) and pick the staging order that reads whole lines.  (GemmArgs: pnvo_ppo_core.h)
template <bool AKC, bool BKC>
__global__ __launch_bounds__(256) void gemm_f32_kernel(GemmArgs g) {
  __shared__ float As[32][65], Bs[32][65];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k0 = 0; k0 < g.K; k0 += 32) {
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int kk = AKC ? (tid & 31) : p * 4 + (tid >> 6);
      const int mm = AKC ? p * 8 + (tid >> 5) : (tid & 63);
      const int m = m0 + mm, k = k0 + kk;
      As[kk][mm] = (m < g.M && k < g.K) ? g.A[(long)m * g.a_sm + (long)k * g.a_sk] : 0.f;
    }
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int kk = BKC ? (tid & 31) : p * 4 + (tid >> 6);
      const int nn = BKC ? p * 8 + (tid >> 5) : (tid & 63);
      const int n = n0 + nn, k = k0 + kk;
      Bs[kk][nn] = (n < g.N && k < g.K) ? g.B[(long)k * g.b_sk + (long)n * g.b_sn] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const float a = As[2 * kk + (lane >> 5)][wm + (lane & 31)];
      const float b = Bs[2 * kk + (lane >> 5)][wn + (lane & 31)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  const int col = n0 + wn + (lane & 31);
  if (col >= g.N) return;
  float bias = 0.f;
  if (g.bias0) bias = g.bias0[col];
  if (g.bias1) bias += g.bias1[col];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    const float v = acc[r] + bias;
    if (row < g.M) g.C[(long)row * g.ldc + col] = g.relu ? fmaxf(v, 0.f) : v;
  }
}

template <bool AKC, bool BKC>
hipError_t launch_gemm(const GemmArgs &g, hipStream_t s) {
  hipLaunchKernelGGL((gemm_f32_kernel<AKC, BKC>), dim3((unsigned)((g.N + 63) / 64), (unsigned)((g.M + 63) / 64)), dim3(256), 0, s, g);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------ recurrent step
// One (t, layer): workgroup = hidden unit j, wave = gate (lstm_layer_kernel's shape).  g holds this step's N rows of G_x on entry and
// the ACTIVATED gates (i, f, g, o) on exit; y (= h[t], the layer's output rows), c[t] and hm = h[t-1] * mask[t] (dW_hh's operand)
// are written beside them.  h_fin / c_fin: the rollout's final state (last step only, else nullptr).
__global__ __launch_bounds__(256) void lstm_step_kernel(float *g, const float *h_prev, const float *c_prev, const float *w_hh,
                                                      const float *masks, int N, int Hd, float *y, float *c_out, float *hm, float *h_fin,
                                                      float *c_fin) {
  __shared__ float sg[4][64];
  const int lane = threadIdx.x & 63, gate = (int)(threadIdx.x >> 6), j = blockIdx.x;
  const int n = gate * Hd + j, H4 = Hd >> 2;
  const long G = 4L * Hd;
  const f32x4 *wh = reinterpret_cast<const f32x4 *>(w_hh + (long)n * Hd);
  for (int b0 = 0; b0 < N; b0 += 64) {
    const int nb = min(64, N - b0);
    for (int bb = 0; bb < nb; ++bb) {
      const int b = b0 + bb;
      const f32x4 *hr = reinterpret_cast<const f32x4 *>(h_prev + (long)b * Hd);
      float u = 0.f;
      for (int k = lane; k < H4; k += 64) {
        const f32x4 w = wh[k], v = hr[k];
        u = __builtin_fmaf(w[0], v[0], u);
        u = __builtin_fmaf(w[1], v[1], u);
        u = __builtin_fmaf(w[2], v[2], u);
        u = __builtin_fmaf(w[3], v[3], u);
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) u += __shfl_xor(u, o);
      if (lane == 0) sg[gate][bb] = g[b * G + n] + u * masks[b];
    }
    __syncthreads();
    if ((int)threadIdx.x < nb) {
      const int b = b0 + (int)threadIdx.x;
      const long e = (long)b * Hd + j;
      const float mk = masks[b];
      const float i_ = 1.f / (1.f + expf(-sg[0][threadIdx.x]));
      const float f_ = 1.f / (1.f + expf(-sg[1][threadIdx.x]));
      const float g_ = tanhf(sg[2][threadIdx.x]);
      const float o_ = 1.f / (1.f + expf(-sg[3][threadIdx.x]));
      const float c = f_ * (c_prev[e] * mk) + i_ * g_;
      const float h = o_ * tanhf(c);
      c_out[e] = c;
      y[e] = h;
      hm[e] = h_prev[e] * mk;
      g[b * G + j] = i_;
      g[b * G + Hd + j] = f_;
      g[b * G + 2 * Hd + j] = g_;
      g[b * G + 3 * Hd + j] = o_;
      if (h_fin != nullptr) {
        h_fin[e] = h;
        c_fin[e] = c;
      }
    }
    __syncthreads();
  }
}

// One (t, layer) of a GRU, in lstm_step_kernel's shape with three waves (r, z, n).  g: this step's N rows of the [M, 4H] gate workspace,
// holding G_x = X . W_ih^T + b_ih in blocks 0 .. 2 on entry and the ACTIVATED r, z, n and q = W_hn hm + b_hn (blocks 0 .. 3) on exit;
// y (= h[t]) and hm = h[t-1] * mask[t] are written beside them.  h_fin: the rollout's final state (last step only, else nullptr).
__global__ __launch_bounds__(192) void gru_step_kernel(float *g, const float *h_prev, const float *w_hh, const float *b_hh,
                                                     const float *masks, int N, int Hd, float *y, float *hm, float *h_fin) {
  __shared__ float sg[3][64];
  const int lane = threadIdx.x & 63, gate = (int)(threadIdx.x >> 6), j = blockIdx.x;
  const int n = gate * Hd + j, H4 = Hd >> 2;
  const long G = 4L * Hd;
  const f32x4 *wh = reinterpret_cast<const f32x4 *>(w_hh + (long)n * Hd);
  for (int b0 = 0; b0 < N; b0 += 64) {
    const int nb = min(64, N - b0);
    for (int bb = 0; bb < nb; ++bb) {
      const int b = b0 + bb;
      const f32x4 *hr = reinterpret_cast<const f32x4 *>(h_prev + (long)b * Hd);
      float u = 0.f;
      for (int k = lane; k < H4; k += 64) {
        const f32x4 w = wh[k], v = hr[k];
        u = __builtin_fmaf(w[0], v[0], u);
        u = __builtin_fmaf(w[1], v[1], u);
        u = __builtin_fmaf(w[2], v[2], u);
        u = __builtin_fmaf(w[3], v[3], u);
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) u += __shfl_xor(u, o);
      if (lane == 0) {
        const float rec = u * masks[b] + b_hh[n];
        sg[gate][bb] = gate == 2 ? rec : rec + g[b * G + n];     // the n gate's two sums stay apart until r is known
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < nb) {
      const int b = b0 + (int)threadIdx.x;
      const long e = (long)b * Hd + j;
      const float r_ = 1.f / (1.f + expf(-sg[0][threadIdx.x]));
      const float z_ = 1.f / (1.f + expf(-sg[1][threadIdx.x]));
      const float q_ = sg[2][threadIdx.x];
      const float n_ = tanhf(g[b * G + 2 * Hd + j] + r_ * q_);
      const float hmv = h_prev[e] * masks[b];
      float h;
      {                                                    // two rounded products and their sum, as gru_layer_kernel of the act path
#pragma clang fp contract(off)                             // (pnvo_policy.hip) forms them: the rollout has the bits of T act steps
        h = (1.f - z_) * n_ + z_ * hmv;
      }
      y[e] = h;
      hm[e] = hmv;
      g[b * G + j] = r_;
      g[b * G + Hd + j] = z_;
      g[b * G + 2 * Hd + j] = n_;
      g[b * G + 3 * Hd + j] = q_;
      if (h_fin != nullptr) h_fin[e] = h;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------ heads
// One wave per row: logits (lane o < A keeps logit o), value (lane A), then log-softmax, log pi(a) and the row entropy across the lanes
// (CategoricalNet / CustomFixedCategorical, utils/misc_utils.py:50-78; CriticHead, policy.py:66-74).  A <= 32.
__global__ __launch_bounds__(256) void heads_eval_kernel(const float *feat, const float *act_w, const float *act_b, const float *cr_w,
                                                       const float *cr_b, const int64_t *actions, int M, int Hd, int A, float *logits,
                                                       float *value, float *logp, float *ent) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (m >= M) return;
  const f32x4 *xr = reinterpret_cast<const f32x4 *>(feat + (long)m * Hd);
  const int H4 = Hd >> 2;
  float mine = 0.f;
  for (int o = 0; o <= A; ++o) {
    const f32x4 *wr = reinterpret_cast<const f32x4 *>(o < A ? act_w + (long)o * Hd : cr_w);
    float s = 0.f;
    for (int k = lane; k < H4; k += 64) {
      const f32x4 w = wr[k], v = xr[k];
      s = __builtin_fmaf(w[0], v[0], s);
      s = __builtin_fmaf(w[1], v[1], s);
      s = __builtin_fmaf(w[2], v[2], s);
      s = __builtin_fmaf(w[3], v[3], s);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if (lane == o) mine = s + (o < A ? act_b[o] : cr_b[0]);
  }
  const bool is_logit = lane < A;
  float mx = is_logit ? mine : -INFINITY;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
  float se = is_logit ? expf(mine - mx) : 0.f;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) se += __shfl_xor(se, d);
  const float lp = mine - (mx + logf(se));
  float pe = is_logit ? expf(lp) * lp : 0.f;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) pe += __shfl_xor(pe, d);
  long a = actions[m];
  a = a < 0 ? 0 : (a >= A ? A - 1 : a);
  const float lpa = __shfl(lp, (int)a);
  if (is_logit) logits[(long)m * A + lane] = mine;
  if (lane == A) value[m] = mine;
  if (lane == 0) {
    logp[m] = lpa;
    ent[m] = -pe;
  }
}

// out[0] = mean of x[0 .. n) — one workgroup, a fixed summation order
__global__ __launch_bounds__(256) void mean_kernel(const float *x, int n, float *out) {
  __shared__ double sd[256];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += (double)x[i];
  sd[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) sd[threadIdx.x] += sd[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(sd[0] / n);
}

// The minibatch loss of rl/ppo/ppo.py:101-126 and its gradient with respect to the logits and the value, one workgroup:
//   ratio = exp(logp - logp_old); action_loss = -mean(min(ratio * adv, clamp(ratio, 1 - clip, 1 + clip) * adv))
//   value_loss = 0.5 * mean(max((v - R)^2, (vp + clamp(v - vp, -clip, clip) - R)^2))   or   0.5 * mean((R - v)^2)
//   total = value_loss * vc + action_loss - mean(entropy) * ec;      out3 = {value_loss, action_loss, mean(entropy)}
// torch's gradient rules: min / max pass the gradient to the smaller / larger argument and half to each when they are equal, clamp
// passes it where lo <= x <= hi — inside the clip range both branches are equal and the full gradient passes.
__global__ __launch_bounds__(256) void ppo_loss_kernel(const float *logits, const float *value, const float *logp, const float *ent,
                                                     const int64_t *actions, const float *old_logp, const float *adv, const float *vpred,
                                                     const float *ret, int M, int A, float clip, float vc, float ec, int use_clipped,
                                                     float *out3, float *dlogits, float *dvalue) {
  __shared__ double sd[3][256];
  double sv = 0.0, sa = 0.0, se = 0.0;
  const float inv_m = 1.f / (float)M;
  for (int m = threadIdx.x; m < M; m += 256) {
    const float ratio = expf(logp[m] - old_logp[m]), ad = adv[m];
    const float lo = 1.f - clip, hi = 1.f + clip;
    const float s1 = ratio * ad, s2 = fminf(fmaxf(ratio, lo), hi) * ad;
    const bool inr = ratio >= lo && ratio <= hi;
    const float g2 = inr ? ad : 0.f;
    const float gr = s1 < s2 ? ad : (s1 > s2 ? g2 : 0.5f * ad + 0.5f * g2);
    sa += (double)fminf(s1, s2);
    const float g_lp = -(gr * ratio) * inv_m;                 // d total / d log pi(a)
    const float v = value[m], R = ret[m];
    if (use_clipped) {
      const float vp = vpred[m], d = v - vp;
      const float e1 = v - R, e2 = (vp + fminf(fmaxf(d, -clip), clip)) - R;
      const float l1 = e1 * e1, l2 = e2 * e2;
      const float ge2 = (d >= -clip && d <= clip) ? e2 : 0.f;
      sv += (double)fmaxf(l1, l2);
      const float gv = l1 > l2 ? 2.f * e1 : (l2 > l1 ? 2.f * ge2 : e1 + ge2);
      dvalue[m] = vc * 0.5f * gv * inv_m;
    } else {
      const float e = R - v;
      sv += (double)(e * e);
      dvalue[m] = vc * (v - R) * inv_m;
    }
    const float H = ent[m];
    se += (double)H;
    const float *l = logits + (long)m * A;
    float mx = l[0];
    for (int k = 1; k < A; ++k) mx = fmaxf(mx, l[k]);
    float sum = 0.f;
    for (int k = 0; k < A; ++k) sum += expf(l[k] - mx);
    const float lse = mx + logf(sum);
    long a = actions[m];
    a = a < 0 ? 0 : (a >= A ? A - 1 : a);
    for (int k = 0; k < A; ++k) {
      const float lpk = l[k] - lse, pk = expf(lpk);
      // d log pi(a) / d logit_k = [k == a] - p_k;   d entropy / d logit_k = -p_k (log p_k + entropy)
      dlogits[(long)m * A + k] = g_lp * ((k == a ? 1.f : 0.f) - pk) + ec * inv_m * pk * (lpk + H);
    }
  }
  sd[0][threadIdx.x] = sv;
  sd[1][threadIdx.x] = sa;
  sd[2][threadIdx.x] = se;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sd[0][threadIdx.x] += sd[0][threadIdx.x + o];
      sd[1][threadIdx.x] += sd[1][threadIdx.x + o];
      sd[2][threadIdx.x] += sd[2][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out3[0] = (float)(0.5 * sd[0][0] / M);
    out3[1] = (float)(-sd[1][0] / M);
    out3[2] = (float)(sd[2][0] / M);
  }
}

// head weight / bias gradients: one thread per (output o <= A, column k), rows summed in order
__global__ __launch_bounds__(256) void heads_bwd_w_kernel(const float *feat, const float *dlogits, const float *dvalue, int M, int Hd, int A,
                                                        float *g_act_w, float *g_act_b, float *g_cr_w, float *g_cr_b) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)(A + 1) * Hd) return;
  const int o = (int)(e / Hd), k = (int)(e % Hd);
  float s = 0.f, sb = 0.f;
  for (int m = 0; m < M; ++m) {
    const float d = o < A ? dlogits[(long)m * A + o] : dvalue[m];
    s = __builtin_fmaf(d, feat[(long)m * Hd + k], s);
    sb += d;
  }
  if (o < A) g_act_w[(long)o * Hd + k] = s; else g_cr_w[k] = s;
  if (k == 0) {
    if (o < A) g_act_b[o] = sb; else g_cr_b[0] = sb;
  }
}

// d features = dlogits . W_act + dvalue . W_cr
__global__ __launch_bounds__(256) void heads_bwd_x_kernel(const float *dlogits, const float *dvalue, const float *act_w, const float *cr_w,
                                                        int M, int Hd, int A, float *dfeat) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)M * Hd) return;
  const int m = (int)(e / Hd), k = (int)(e % Hd);
  float s = dvalue[m] * cr_w[k];
  for (int a = 0; a < A; ++a) s = __builtin_fmaf(dlogits[(long)m * A + a], act_w[(long)a * Hd + k], s);
  dfeat[e] = s;
}

// dst [C][R] = src [R][C]^T
__global__ __launch_bounds__(256) void transpose_kernel(const float *src, int R, int C, float *dst) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = (int)(threadIdx.x >> 5);
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  for (int i = ty; i < 32; i += 8)
    if (r0 + i < R && c0 + tx < C) tile[i][tx] = src[(long)(r0 + i) * C + c0 + tx];
  __syncthreads();
  for (int i = ty; i < 32; i += 8)
    if (c0 + i < C && r0 + tx < R) dst[(long)(c0 + i) * R + r0 + tx] = tile[tx][i];
}

// ------------------------------------------------------------------------------------------------------------ BPTT step
// One (t, layer), run for t = T-1 .. 0: workgroup = hidden unit j.  With the finished dgates[t+1] of the previous launch (dg_n; nullptr
// at t = T-1) the four waves form dh_rec[b] = mask[t+1][b] * (dgates[t+1][b] . W_hh[:, j]) — each wave one gate block of the
// transposed weight row whhT[j][0 .. 4H), summed in gate order — then the first lanes run the cell backward for (b, j):
//   dh = dY[t] + dh_rec;  dc = dh * o * (1 - tanh(c)^2) + mask[t+1] * f[t+1] * dc[t+1]
//   dgates[t] = (dc g i(1-i), dc c_prev f(1-f), dc i (1-g^2), dh tanh(c) o(1-o)),  c_prev = c[t-1] * mask[t]
__global__ __launch_bounds__(256) void bptt_step_kernel(const float *gates_t, const float *gates_n, const float *dg_n, const float *dc_n,
                                                      const float *mask_n, const float *c_t, const float *c_prev, const float *mask_t,
                                                      const float *whhT, const float *dY_t, int N, int Hd, float *dg_t, float *dc_t) {
  __shared__ float sg[4][64];
  const int lane = threadIdx.x & 63, gate = (int)(threadIdx.x >> 6), j = blockIdx.x;
  const int H4 = Hd >> 2;
  const long G = 4L * Hd;
  const f32x4 *wt = reinterpret_cast<const f32x4 *>(whhT + (long)j * G + (long)gate * Hd);
  for (int b0 = 0; b0 < N; b0 += 64) {
    const int nb = min(64, N - b0);
    if (dg_n != nullptr) {
      for (int bb = 0; bb < nb; ++bb) {
        const f32x4 *dr = reinterpret_cast<const f32x4 *>(dg_n + (long)(b0 + bb) * G + (long)gate * Hd);
        float u = 0.f;
        for (int k = lane; k < H4; k += 64) {
          const f32x4 w = wt[k], v = dr[k];
          u = __builtin_fmaf(w[0], v[0], u);
          u = __builtin_fmaf(w[1], v[1], u);
          u = __builtin_fmaf(w[2], v[2], u);
          u = __builtin_fmaf(w[3], v[3], u);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) u += __shfl_xor(u, o);
        if (lane == 0) sg[gate][bb] = u;
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < nb) {
      const int b = b0 + (int)threadIdx.x;
      const long e = (long)b * Hd + j;
      float dh = dY_t[e], dc_rec = 0.f;
      if (dg_n != nullptr) {
        const float mn = mask_n[b];
        dh += mn * (((sg[0][threadIdx.x] + sg[1][threadIdx.x]) + sg[2][threadIdx.x]) + sg[3][threadIdx.x]);
        dc_rec = mn * gates_n[b * G + Hd + j] * dc_n[e];
      }
      const float i_ = gates_t[b * G + j], f_ = gates_t[b * G + Hd + j], g_ = gates_t[b * G + 2 * Hd + j], o_ = gates_t[b * G + 3 * Hd + j];
      const float tc = tanhf(c_t[e]);
      const float dc = dh * o_ * (1.f - tc * tc) + dc_rec;
      const float cp = c_prev[e] * mask_t[b];
      dc_t[e] = dc;
      dg_t[b * G + j] = dc * g_ * i_ * (1.f - i_);
      dg_t[b * G + Hd + j] = dc * cp * f_ * (1.f - f_);
      dg_t[b * G + 2 * Hd + j] = dc * i_ * (1.f - g_ * g_);
      dg_t[b * G + 3 * Hd + j] = dh * tc * o_ * (1.f - o_);
    }
    __syncthreads();
  }
}

// One (t, layer) of a GRU, run for t = T-1 .. 0: workgroup = hidden unit j, three waves.  With the finished dGh[t+1] of the previous
// launch (dgh_n; nullptr at t = T-1) the waves form dGh[t+1][b] . W_hh[:, j] — each wave one gate block of the transposed weight row
// whhT[j][0 .. 3H), summed in gate order — then the first lanes run the cell backward for (b, j):
//   dh = dY[t] + mask[t+1] * (z[t+1] * dh[t+1] + dGh[t+1] . W_hh[:, j])      (hm enters h' directly through z and through W_hh)
//   dn_pre = dh (1 - z)(1 - n^2),  dz_pre = dh (hm - n) z (1 - z),  dr_pre = dn_pre q r (1 - r)
//   dGx[t] = (dr_pre, dz_pre, dn_pre),  dGh[t] = (dr_pre, dz_pre, dn_pre * r)
__global__ __launch_bounds__(192) void gru_bptt_step_kernel(const float *gates_t, const float *gates_n, const float *dgh_n,
                                                          const float *dh_n, const float *mask_n, const float *hm_t, const float *whhT,
                                                          const float *dY_t, int N, int Hd, float *dgx_t, float *dgh_t, float *dh_t) {
  __shared__ float sg[3][64];
  const int lane = threadIdx.x & 63, gate = (int)(threadIdx.x >> 6), j = blockIdx.x;
  const int H4 = Hd >> 2;
  const long G = 4L * Hd, G3 = 3L * Hd;
  const f32x4 *wt = reinterpret_cast<const f32x4 *>(whhT + (long)j * G3 + (long)gate * Hd);
  for (int b0 = 0; b0 < N; b0 += 64) {
    const int nb = min(64, N - b0);
    if (dgh_n != nullptr) {
      for (int bb = 0; bb < nb; ++bb) {
        const f32x4 *dr = reinterpret_cast<const f32x4 *>(dgh_n + (long)(b0 + bb) * G3 + (long)gate * Hd);
        float u = 0.f;
        for (int k = lane; k < H4; k += 64) {
          const f32x4 w = wt[k], v = dr[k];
          u = __builtin_fmaf(w[0], v[0], u);
          u = __builtin_fmaf(w[1], v[1], u);
          u = __builtin_fmaf(w[2], v[2], u);
          u = __builtin_fmaf(w[3], v[3], u);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) u += __shfl_xor(u, o);
        if (lane == 0) sg[gate][bb] = u;
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < nb) {
      const int b = b0 + (int)threadIdx.x;
      const long e = (long)b * Hd + j;
      float dh = dY_t[e];
      if (dgh_n != nullptr)
        dh += mask_n[b] * (gates_n[b * G + Hd + j] * dh_n[e] + ((sg[0][threadIdx.x] + sg[1][threadIdx.x]) + sg[2][threadIdx.x]));
      const float r_ = gates_t[b * G + j], z_ = gates_t[b * G + Hd + j], n_ = gates_t[b * G + 2 * Hd + j], q_ = gates_t[b * G + 3 * Hd + j];
      const float dn = dh * (1.f - z_) * (1.f - n_ * n_);
      const float dz = dh * (hm_t[e] - n_) * z_ * (1.f - z_);
      const float dr = dn * q_ * r_ * (1.f - r_);
      dh_t[e] = dh;
      dgx_t[b * G3 + j] = dr;
      dgx_t[b * G3 + Hd + j] = dz;
      dgx_t[b * G3 + 2 * Hd + j] = dn;
      dgh_t[b * G3 + j] = dr;
      dgh_t[b * G3 + Hd + j] = dz;
      dgh_t[b * G3 + 2 * Hd + j] = dn * r_;
    }
    __syncthreads();
  }
}

// clip_grad_norm_: partial sums of squares over fixed slices, then every workgroup folds the partials in the same order and scales
// (scale: pnvo_policy_clip_grad_norm_scaled — the norm of scale * g with each product rounded to float32, then ONE write of
// g * (scale * clip); scale = 1 multiplies by one, exactly)
__global__ __launch_bounds__(256) void sumsq_kernel(const float *g, long n, float scale, double *part) {
  __shared__ double sd[256];
  double a = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)SQ_BLOCKS * 256) {
    const double v = (double)(g[i] * scale);
    a += v * v;
  }
  sd[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) sd[threadIdx.x] += sd[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sd[0];
}
__global__ __launch_bounds__(256) void clip_scale_kernel(float *g, long n, const double *part, float scale, float max_norm, float *norm_out) {
  __shared__ double sd[256];
  double a = 0.0;
  for (int i = threadIdx.x; i < SQ_BLOCKS; i += 256) a += part[i];
  sd[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) sd[threadIdx.x] += sd[threadIdx.x + o];
    __syncthreads();
  }
  const float norm = (float)sqrt(sd[0]);
  if (norm_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = norm;
  const float coef = max_norm / (norm + 1e-6f);              // nn.utils.clip_grad_norm_: clamp(max_norm / (total + 1e-6), max = 1)
  const bool clip = max_norm > 0.f && coef < 1.f;            // (max_norm <= 0: scale only)
  if (!clip && scale == 1.f) return;
  const float f = clip ? scale * coef : scale;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) g[i] *= f;
}

}  // namespace

hipError_t launch_gemm_f32(const GemmArgs &g, bool akc, bool bkc, hipStream_t s) {
  if (akc) return bkc ? launch_gemm<true, true>(g, s) : launch_gemm<true, false>(g, s);
  return bkc ? launch_gemm<false, true>(g, s) : launch_gemm<false, false>(g, s);
}

hipError_t launch_transpose(const float *src, int R, int C, float *dst, hipStream_t s) {
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((C + 31) / 32), (unsigned)((R + 31) / 32)), dim3(256), 0, s, src, R, C, dst);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------ the host side
PpoCore::~PpoCore() {
  for (hipEvent_t &e : ev)
    if (e) (void)hipEventDestroy(e);
}

int core_init(PpoCore *c, const char *abi, int device, float *params, float *grads, size_t n, size_t n_named, int Hd, int L, int A, bool gru) {
  c->abi = abi, c->device = device;
  c->params = params, c->grads = grads, c->n = n, c->n_named = n_named;
  c->Hd = Hd, c->L = L, c->A = A, c->gru = gru;
  PCHK(c->whhT.alloc((size_t)(gru ? 3 : 4) * Hd * Hd));
  PCHK(c->sq_part.alloc(SQ_BLOCKS));
  return PNVO_OK;
}

int core_check_rollout(const char *fn, int T, int N, std::initializer_list<const void *> ptrs, const float *hidden_in,
                       const float *hidden_out, size_t state_floats, const char *state_desc) {
  if (T <= 0 || N <= 0 || (long)T * N > (1L << 20))
    return pfail(PNVO_ERR_ARG, "bad rollout shape T = " + std::to_string(T) + ", N = " + std::to_string(N));
  bool null = !hidden_in || !hidden_out;
  for (const void *q : ptrs) null = null || !q;
  if (null) return pfail(PNVO_ERR_ARG, "null argument");
  if (((uintptr_t)hidden_in & 15) || ((uintptr_t)hidden_out & 15))
    return pfail(PNVO_ERR_ARG, std::string(fn) + ": hidden_in / hidden_out must be 16-byte aligned");
  if (hidden_states_overlap(hidden_in, hidden_out, state_floats))
    return pfail(PNVO_ERR_ARG, std::string("hidden_out overlaps hidden_in (each holds ") + state_desc + " floats): pass separate buffers");
  return PNVO_OK;
}

void core_release(PpoCore *c) {
  for (DevBuf<float> *b : {&c->masks, &c->hid0, &c->logits, &c->value, &c->logp, &c->ent, &c->dlogits, &c->dvalue, &c->dY, &c->dG, &c->dGh, &c->dH})
    b->reset();
  c->actions.reset();
  for (auto *v : {&c->gates, &c->c, &c->y, &c->hm}) v->clear();
  c->capM = 0;
}

int core_reserve(PpoCore *c, int M, int N) {
  if (M > c->capM) core_release(c);
  PCHK(c->hid0.reserve(core_state_floats(*c, N)));             // (N can grow under an M that fits)
  if (M <= c->capM) return PNVO_OK;
  const size_t Hd = (size_t)c->Hd, L = (size_t)c->L, m = (size_t)M, A = (size_t)c->A, G = c->gru ? 3 : 4;
  PCHK(c->masks.alloc(m));
  PCHK(c->actions.alloc(m));
  for (auto *v : {&c->gates, &c->y, &c->hm}) v->resize(L);
  if (!c->gru) c->c.resize(L);
  for (size_t l = 0; l < L; ++l) {
    PCHK(c->gates[l].alloc(m * 4 * Hd));
    if (!c->gru) PCHK(c->c[l].alloc(m * Hd));
    PCHK(c->y[l].alloc(m * Hd));
    PCHK(c->hm[l].alloc(m * Hd));
  }
  PCHK(c->logits.alloc(m * A));
  PCHK(c->value.alloc(m));
  PCHK(c->logp.alloc(m));
  PCHK(c->ent.alloc(m));
  PCHK(c->dlogits.alloc(m * A));
  PCHK(c->dvalue.alloc(m));
  PCHK(c->dY.alloc(m * Hd));
  PCHK(c->dG.alloc(m * G * Hd));
  if (c->gru) PCHK(c->dGh.alloc(m * 3 * Hd));
  PCHK(c->dH.alloc(m * Hd));
  c->capM = M;
  return PNVO_OK;
}

int core_keep(PpoCore *c, int T, int N, const float *masks, const int64_t *actions, const float *hidden_in, hipStream_t s) {
  const size_t M = (size_t)T * N;
  c->T = T, c->N = N, c->M = (int)M;
  c->have_loss = false;
  PCHK(hipMemcpyAsync(c->masks, masks, M * sizeof(float), hipMemcpyDeviceToDevice, s));
  PCHK(hipMemcpyAsync(c->actions, actions, M * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  PCHK(hipMemcpyAsync(c->hid0, hidden_in, core_state_floats(*c, N) * sizeof(float), hipMemcpyDeviceToDevice, s));
  return PNVO_OK;
}

int core_recurrent_forward(PpoCore *c, const RnnLayer *layers, const float *x0, bool gx0_done, float *hidden_out, hipStream_t s) {
  const int Hd = c->Hd, L = c->L, T = c->T, N = c->N, M = c->M, G = c->gru ? 3 : 4;
  const float *xin = x0;
  for (int l = 0; l < L; ++l) {
    const RnnLayer &ly = layers[l];
    if (l > 0 || !gx0_done) {
      // G_x into the [M, 4H] gate rows.  GRU: blocks 0 .. 2, and b_hh is added by the step (b_hn belongs inside r * (...))
      GemmArgs g{xin, ly.w_ih, ly.b_ih, c->gru ? nullptr : ly.b_hh, c->gates[l], M, G * Hd, ly.K, (long)ly.ldx, 1, 1, (long)ly.K, 4L * Hd};
      PCHK(launch_gemm_f32(g, true, true, s));
    }
    float *h_fin = hidden_out + (size_t)l * N * Hd, *c_fin = hidden_out + (size_t)(L + l) * N * Hd;       // (c: LSTM only)
    for (int ts = 0; ts < T; ++ts) {
      const size_t r = (size_t)ts * N;
      const bool last = ts == T - 1;
      float *gates = c->gates[l] + r * 4 * Hd, *y = c->y[l] + r * Hd, *hm = c->hm[l] + r * Hd;
      const float *h_prev = ts ? c->y[l] + (r - N) * Hd : c->hid0 + (size_t)l * N * Hd;
      if (c->gru) {
        hipLaunchKernelGGL(gru_step_kernel, dim3((unsigned)Hd), dim3(192), 0, s, gates, h_prev, ly.w_hh, ly.b_hh, c->masks + r, N, Hd, y, hm,
                           last ? h_fin : nullptr);
      } else {
        const float *c_prev = ts ? c->c[l] + (r - N) * Hd : c->hid0 + (size_t)(L + l) * N * Hd;
        hipLaunchKernelGGL(lstm_step_kernel, dim3((unsigned)Hd), dim3(256), 0, s, gates, h_prev, c_prev, ly.w_hh, c->masks + r, N, Hd, y,
                           c->c[l] + r * Hd, hm, last ? h_fin : nullptr, last ? c_fin : nullptr);
      }
    }
    PCHK(hipGetLastError());
    xin = c->y[l];
  }
  return PNVO_OK;
}

int core_heads(PpoCore *c, const Heads &h, float *value, float *logp, float *entropy, hipStream_t s) {
  const int M = c->M;
  hipLaunchKernelGGL(heads_eval_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, c->y[c->L - 1], h.act_w, h.act_b, h.cr_w, h.cr_b,
                     c->actions, M, c->Hd, c->A, c->logits, c->value, c->logp, c->ent);
  if (value) PCHK(hipMemcpyAsync(value, c->value, (size_t)M * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (logp) PCHK(hipMemcpyAsync(logp, c->logp, (size_t)M * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (entropy) hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, s, c->ent, M, entropy);
  PCHK(hipGetLastError());
  PCHK(core_mark(c, 2, s));
  return PNVO_OK;
}

int core_ppo_loss(PpoCore *c, const float *actions_logp_old, const float *adv, const float *value_preds, const float *returns, float clip,
                  float value_coef, float entropy_coef, int use_clipped_value_loss, float *out3, hipStream_t s) {
  const std::string abi = c->abi;
  if (c->M <= 0) return pfail(PNVO_ERR_STATE, abi + "_ppo_loss before " + abi + "_evaluate");
  if (!actions_logp_old || !adv || !returns || !out3 || (use_clipped_value_loss && !value_preds)) return pfail(PNVO_ERR_ARG, "null argument");
  if (!(clip >= 0.f)) return pfail(PNVO_ERR_ARG, "clip_param " + std::to_string(clip) + " must be >= 0");
  PCHK(hipSetDevice(c->device));
  PCHK(core_mark(c, 3, s));
  hipLaunchKernelGGL(ppo_loss_kernel, dim3(1), dim3(256), 0, s, c->logits, c->value, c->logp, c->ent, c->actions, actions_logp_old, adv,
                     value_preds, returns, c->M, c->A, clip, value_coef, entropy_coef, use_clipped_value_loss ? 1 : 0, out3, c->dlogits,
                     c->dvalue);
  PCHK(hipGetLastError());
  PCHK(core_mark(c, 4, s));
  c->have_loss = true;
  return PNVO_OK;
}

int core_backward_ready(const PpoCore *c) {
  const std::string abi = c->abi;
  if (c->M <= 0 || !c->have_loss) return pfail(PNVO_ERR_STATE, abi + "_backward before " + abi + "_evaluate + " + abi + "_ppo_loss");
  return PNVO_OK;
}

int core_backward(PpoCore *c, const RnnLayer *layers, const Heads &h, const float *x0, float *dX0, hipStream_t s) {
  const int Hd = c->Hd, L = c->L, A = c->A, T = c->T, N = c->N, M = c->M, G = c->gru ? 3 : 4, GH = G * Hd;
  hipLaunchKernelGGL(heads_bwd_w_kernel, dim3((unsigned)(((long)(A + 1) * Hd + 255) / 256)), dim3(256), 0, s, c->y[L - 1], c->dlogits,
                     c->dvalue, M, Hd, A, grad_of(*c, h.act_w), grad_of(*c, h.act_b), grad_of(*c, h.cr_w), grad_of(*c, h.cr_b));
  hipLaunchKernelGGL(heads_bwd_x_kernel, dim3((unsigned)(((long)M * Hd + 255) / 256)), dim3(256), 0, s, c->dlogits, c->dvalue, h.act_w,
                     h.cr_w, M, Hd, A, c->dY);
  PCHK(hipGetLastError());
  for (int l = L - 1; l >= 0; --l) {
    const RnnLayer &ly = layers[l];
    const float *X = l == 0 ? x0 : c->y[l - 1];
    const float *dGrec = c->gru ? c->dGh : c->dG;              // the gate gradients on the recurrent side: what dW_hh and the step before read
    PCHK(launch_transpose(ly.w_hh, GH, Hd, c->whhT, s));
    for (int ts = T - 1; ts >= 0; --ts) {
      const size_t r = (size_t)ts * N, rn = r + N;
      const bool last = ts == T - 1;
      const float *gates_t = c->gates[l] + r * 4 * Hd, *gates_n = last ? nullptr : c->gates[l] + rn * 4 * Hd;
      const float *dg_n = last ? nullptr : dGrec + rn * GH, *dh_n = last ? nullptr : c->dH + rn * Hd, *mask_n = last ? nullptr : c->masks + rn;
      if (c->gru) {
        hipLaunchKernelGGL(gru_bptt_step_kernel, dim3((unsigned)Hd), dim3(192), 0, s, gates_t, gates_n, dg_n, dh_n, mask_n, c->hm[l] + r * Hd,
                           c->whhT, c->dY + r * Hd, N, Hd, c->dG + r * GH, c->dGh + r * GH, c->dH + r * Hd);
      } else {
        const float *c_prev = ts ? c->c[l] + (r - N) * Hd : c->hid0 + (size_t)(L + l) * N * Hd;
        hipLaunchKernelGGL(bptt_step_kernel, dim3((unsigned)Hd), dim3(256), 0, s, gates_t, gates_n, dg_n, dh_n, mask_n, c->c[l] + r * Hd, c_prev,
                           c->masks + r, c->whhT, c->dY + r * Hd, N, Hd, c->dG + r * GH, c->dH + r * Hd);
      }
    }
    PCHK(hipGetLastError());
    // dW_ih = dG^T . X,  dW_hh = dGrec^T . (h_prev * mask),  db_ih = colsum(dG),  db_hh = colsum(dGrec),  dX = dG . W_ih
    GemmArgs wi{c->dG, X, nullptr, nullptr, grad_of(*c, ly.w_ih), GH, ly.K, M, 1, (long)GH, (long)ly.ldx, 1, (long)ly.K};
    PCHK(launch_gemm_f32(wi, false, false, s));
    GemmArgs wh{dGrec, c->hm[l], nullptr, nullptr, grad_of(*c, ly.w_hh), GH, Hd, M, 1, (long)GH, (long)Hd, 1, (long)Hd};
    PCHK(launch_gemm_f32(wh, false, false, s));
    PCHK(launch_colsum(c->dG, M, GH, GH, grad_of(*c, ly.b_ih), s));
    if (c->gru)
      PCHK(launch_colsum(c->dGh, M, GH, GH, grad_of(*c, ly.b_hh), s));
    else
      PCHK(hipMemcpyAsync(grad_of(*c, ly.b_hh), grad_of(*c, ly.b_ih), (size_t)GH * sizeof(float), hipMemcpyDeviceToDevice, s));
    float *dX = l == 0 ? dX0 : (float *)c->dY;
    if (dX == nullptr) continue;
    GemmArgs dx{c->dG, ly.w_ih, nullptr, nullptr, dX, M, ly.K, GH, (long)GH, 1, (long)ly.K, 1, (long)ly.K};
    PCHK(launch_gemm_f32(dx, true, false, s));
  }
  return PNVO_OK;
}

int core_clip_grad_norm(PpoCore *c, float scale, float max_norm, float *norm_out, hipStream_t s) {
  PCHK(hipSetDevice(c->device));
  const long n = (long)c->n_named;
  hipLaunchKernelGGL(sumsq_kernel, dim3(SQ_BLOCKS), dim3(256), 0, s, c->grads, n, scale, c->sq_part);
  hipLaunchKernelGGL(clip_scale_kernel, dim3(SQ_BLOCKS), dim3(256), 0, s, c->grads, n, c->sq_part, scale, max_norm, norm_out);
  PCHK(hipGetLastError());
  return PNVO_OK;
}

int core_timing(PpoCore *c, int mode) {
  PCHK(hipSetDevice(c->device));
  if (mode)
    for (hipEvent_t &e : c->ev)
      if (!e) PCHK(hipEventCreate(&e));
  c->timing = mode != 0;
  return PNVO_OK;
}

int core_timing_read(PpoCore *c, double ms[5]) {
  if (!c->timing) return pfail(PNVO_ERR_STATE, std::string(c->abi) + "_train_timing(h, 1) first");
  PCHK(hipEventSynchronize(c->ev[7]));
  const int pairs[5][2] = {{0, 1}, {1, 2}, {3, 4}, {5, 6}, {6, 7}};
  for (int k = 0; k < 5; ++k) {
    float f = 0.f;
    PCHK(hipEventElapsedTime(&f, c->ev[pairs[k][0]], c->ev[pairs[k][1]]));
    ms[k] = (double)f;
  }
  return PNVO_OK;
}

}  // namespace pnvo
