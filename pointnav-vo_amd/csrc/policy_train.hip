// policy_train.hip — one PPO minibatch update of the navigation policy (rl/ppo/ppo.py:61-139 around Policy.evaluate_actions,
// rl/policies/policy.py:52-63), gfx950 only, float32.
//
//   evaluate : depth [T*N] -> avg_pool2d(2) (or, pnvo_policy_evaluate_rgbd: rgb / depth frames -> the input stage of pnvo_policy.hip, which
//              in training mode merges the T*N rows into RunningMeanAndVar's buffers first) -> the visual encoder's TRAIN-mode forward
//              (pnvo_train_forward: activations kept)
//              -> x = [visual | tgt_embeding | prev_action_embedding]                       policy_inputs_kernel, M = T*N rows
//              -> per LSTM layer: G_x = X . W_ih^T + b_ih + b_hh over all M rows            gemm_f32_kernel (v_mfma_f32_32x32x2_f32)
//                                 T launches of lstm_step_kernel (the only sequential part)  gates, c, h, masked h_prev kept
//              -> logits / value / log pi(a) / entropy per row                               heads_eval_kernel
//   ppo_loss : clipped surrogate, clipped or plain value loss, entropy mean; d total / d logits, d total / d value   ppo_loss_kernel
//   backward : heads -> per layer (top first) T launches of bptt_step_kernel, then dW_ih / dW_hh / dX as GEMMs over all rows and the
//              bias gradients as column sums -> embeddings -> d visual into the encoder's backward below its output head.
// Rows are T-major (row t*N + n: the order RolloutStorage.recurrent_generator yields), weights in torch's [4H][K] layouts read straight
// from the caller's flat parameter buffer, gate order i, f, g, o.  Every reduction runs in a fixed order (no float atomics): the same
// call gives the same bits twice.  Masking h and c at EVERY step equals the reference's segment-wise masking
// (model_utils/rnns/rnn_state_encoder.py:81-134): inside a segment all masks are 1.
//
// With cfg.rnn_type = GRU the recurrent core is torch.nn.GRU (gate order r, z, n; weights [3H][K]; state [L, N, H], h only):
//   evaluate : G_x = X . W_ih^T + b_ih ONLY (b_hn sits inside the product with r, so b_hh cannot ride on the input GEMM), then T launches
//              of gru_step_kernel, which add the recurrent products and b_hh and keep (r, z, n, q = W_hn hm + b_hn), y and hm per row
//   backward : T launches of gru_bptt_step_kernel filling dGx = (dr, dz, dn) and dGh = (dr, dz, dn * r); dW_ih = dGx^T . X,
//              dW_hh = dGh^T . hm, db_ih = colsum(dGx), db_hh = colsum(dGh), dX = dGx . W_ih
// Everything else (encoder, inputs, heads, loss, clipping) is shared; the type is branched on once per call, on the host.
//
// pnvo_policy_evaluate_features takes the encoder's output [M, C, fh, fw] (observations["visual_features"], the reference's frozen-encoder
// training) in place of depth: the encoder does not run, visual = relu(features . W_fc^T + b_fc) is launch_visual_fc (the row kernel of
// pnvo_policy.hip for few rows, gemm_f32_kernel with a ReLU epilogue otherwise) on torch's [hidden, F] weight, and the backward ends with
// the ReLU mask, dW_fc = d visual^T . features (the rows kept in the workspace) and db_fc = colsum: the encoder's range stays zero.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pnvo.h"
#include "pnvo_internal.h"
#include "pnvo_model.h"
#include "pnvo_policy_state.h"

namespace pnvo {

struct PolicyTrain {
  float *params = nullptr, *grads = nullptr;   // the caller's flat buffers (not owned)
  size_t n = 0, n_named = 0;          // floats handed over / floats covered by the parameter table (the rest is the tail below)
  size_t o_stem = 0;                  // the policy's stem weight [C0,C,7,7] (the one tensor read here that is not a Policy slot)
  size_t o_stem2 = 0;                 // tail: the stem weight zero-padded to the encoder handle's 2C input channels [C0,2C,7,7],
  int c0 = 0, stem_row = 49;          //       then the handle's unused output head (hidden weights + 1 bias, zeros); stem_row = C * 49
  // the last evaluate
  int T = 0, N = 0, M = 0;
  bool have_loss = false;
  // workspace, sized for capM rows
  int capM = 0;
  DevBuf<float> pooled, enc_out, x0, g3, masks, hid0;
  int cap_pooled = 0;                 // frames `pooled` holds: grown by the evaluate that takes depth only
  // the evaluate that takes visual_features: the feature rows [M, F] (kept: the caller's tensor may be gone by the backward) and
  // visual = relu(visual_fc(features)) [M, hidden]; from_features says which kind of evaluate came last
  DevBuf<float> feat, visual;
  int cap_feat = 0;
  bool from_features = false;
  DevBuf<int> rows;
  DevBuf<int64_t> actions;
  std::vector<DevBuf<float>> gates, c, y, hm;
  DevBuf<float> logits, value, logp, ent, dlogits, dvalue;
  DevBuf<float> dY, dX0, dG, dC, whhT;
  DevBuf<float> dGh;                  // GRU only: the recurrent side's gate gradients [M, 3H] (dG holds the input side's; dC holds dh)
  DevBuf<double> sq_part;             // clip_grad_norm partial sums
  // pnvo_policy_train_timing: events at the phase boundaries of evaluate / ppo_loss / backward (tools/bench_ppo_update.py)
  bool timing = false;
  hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // pnvo_policy_set_grad_hook.  The flat ranges of the parameter table by the side that produces their gradient, each list ascending and
  // disjoint (neighbouring tensors of one side are one range, alignment gaps included): `early` — embeddings, recurrent tensors, heads:
  // final before the encoder's backward; `enc` — net.visual_encoder without the stem weight; `vfc` — net.visual_fc; the stem weight is
  // [o_stem, o_stem + c0 * stem_row).  enc_pass: what the running backward lets through of the encoder handle's own reports
  // (0: nothing, 1: vfc, 2: vfc and enc).
  typedef std::vector<std::pair<size_t, size_t>> Ranges;    // (first, end)
  Ranges r_early, r_enc, r_vfc;
  pnvo_grad_ready_fn hook = nullptr;
  void *hook_user = nullptr;
  int enc_pass = 0;
};

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int SQ_BLOCKS = CLIP_PARTIALS;

// once attached every Policy slot points into the caller's flat parameter buffer: its gradient sits at the same offset of the other one
float *grad_of(const PolicyTrain *t, const float *slot) { return t->grads + (slot - t->params); }

// ------------------------------------------------------------------------------------------------------------ float32 GEMM
// C[m][n] = sum_k A(m,k) B(k,n) (+ bias0[n] + bias1[n]) on the exact-float32 matrix instruction (one k-ordered fmaf chain per output,
// as conv_mfma.hip): workgroup = 64 x 64 outputs, wave = 32 x 32, K in steps of 32 staged through LDS as [k][m] / [k][n].  Both
// operands are addressed by two strides, so the four products of the LSTM (X . W^T, dG^T . X, dG . W) are one kernel; AKC / BKC say
// which index is contiguous in memory (k, else m / n) and pick the staging order that reads whole lines.  (GemmArgs: pnvo_policy_state.h)
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

// ------------------------------------------------------------------------------------------------------------ input gradients
// From layer 0's dX [M, hidden + 64]: d visual (the first `hidden` columns, copied out contiguous), tgt_embeding's weight [32,3] and
// bias [32], and prev_action_embedding [n_emb, 32] as an ordered sum over the rows that gathered each entry (no atomics; an entry no
// row gathered gets exactly 0).
__global__ __launch_bounds__(256) void inputs_bwd_kernel(const float *dX0, const int *rows, const float *g3, int M, int Hd, int n_emb,
                                                       float *g_tgt_w, float *g_tgt_b, float *g_emb, float *dvis) {
  const int K = Hd + 64;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long ncopy = (long)M * Hd;
  if (e < ncopy) {
    dvis[e] = dX0[(e / Hd) * K + (e % Hd)];
    return;
  }
  const long q = e - ncopy;
  if (q < 96) {
    const int j = (int)(q / 3), c = (int)(q % 3);
    float s = 0.f;
    for (int m = 0; m < M; ++m) s = __builtin_fmaf(dX0[(long)m * K + Hd + j], g3[3 * m + c], s);
    g_tgt_w[q] = s;
  } else if (q < 128) {
    const int j = (int)(q - 96);
    float s = 0.f;
    for (int m = 0; m < M; ++m) s += dX0[(long)m * K + Hd + j];
    g_tgt_b[j] = s;
  } else if (q < 128 + (long)n_emb * 32) {
    const int r = (int)((q - 128) / 32), j = (int)((q - 128) % 32);
    float s = 0.f;
    for (int m = 0; m < M; ++m)
      if (rows[m] == r) s += dX0[(long)m * K + Hd + 32 + j];
    g_emb[(long)r * 32 + j] = s;
  }
}

// ReLU's backward in place: d[e] = 0 where the layer's output y[e] is not positive (torch: grad * (out > 0))
__global__ __launch_bounds__(256) void relu_mask_kernel(const float *y, long n, float *d) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e < n && !(y[e] > 0.f)) d[e] = 0.f;
}

// the policy's stem weight [C0,1,7,7] <-> channel 0 of the encoder handle's [C0,2,7,7] (channel 1 stays 0)
// row = C * 49 floats of one output channel of the policy's stem weight [C0,C,7,7]; the handle's [C0,2C,7,7] has rows of 2 * row
__global__ __launch_bounds__(256) void stem_pad_kernel(const float *w1, int c0, int row, float *w2) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= c0 * 2 * row) return;
  const int o = e / (2 * row), r = e % (2 * row);
  w2[e] = r < row ? w1[o * row + r] : 0.f;
}
__global__ __launch_bounds__(256) void stem_unpad_kernel(const float *w2, int c0, int row, float *w1) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= c0 * row) return;
  w1[e] = w2[(e / row) * 2 * row + (e % row)];
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

// ---- gradient-ready ranges (pnvo_policy_set_grad_hook)
void report(const PolicyTrain *t, const PolicyTrain::Ranges &r, hipStream_t s) {
  if (!t->hook) return;
  for (const auto &ab : r) t->hook(t->hook_user, (uint64_t)ab.first, (uint64_t)(ab.second - ab.first), (void *)s);
}
// the part of [first, end) inside the ranges of `r`, appended to `out`
void clip_ranges(size_t first, size_t end, const PolicyTrain::Ranges &r, PolicyTrain::Ranges *out) {
  for (const auto &ab : r) {
    const size_t a = std::max(first, ab.first), b = std::min(end, ab.second);
    if (b > a) out->push_back({a, b});
  }
}
// what one report [first, end) of the encoder handle means here: that handle was attached to the whole flat buffer (tail and all), so
// its ranges are cut down to the tensors its backward fills — net.visual_fc, and with a trained encoder net.visual_encoder without the
// stem weight, whose gradient is still in the tail's padded copy at that point
PolicyTrain::Ranges encoder_pieces(const PolicyTrain *t, int pass, size_t first, size_t end) {
  PolicyTrain::Ranges enc_vfc, out;
  if (pass >= 2) enc_vfc = t->r_enc;
  if (pass >= 1) enc_vfc.insert(enc_vfc.end(), t->r_vfc.begin(), t->r_vfc.end());
  std::sort(enc_vfc.begin(), enc_vfc.end());
  clip_ranges(first, end, enc_vfc, &out);
  return out;
}
void encoder_hook(void *user, uint64_t first, uint64_t count, void *stream) {
  const PolicyTrain *t = static_cast<const PolicyTrain *>(user);
  if (t->hook && t->enc_pass) report(t, encoder_pieces(t, t->enc_pass, (size_t)first, (size_t)(first + count)), (hipStream_t)stream);
}
// the table's entries sorted by offset -> the three lists; the stem weight splits the encoder's range where it lies
void build_ranges(PolicyTrain *t, const pnvo_tensor_desc *toc, int ntoc) {
  struct Ent { size_t a, b; int side; };
  std::vector<Ent> es;
  for (int k = 0; k < ntoc; ++k) {
    const std::string nm = toc[k].name;
    const size_t a = (size_t)toc[k].offset, b = a + numel(std::vector<int64_t>(toc[k].shape, toc[k].shape + toc[k].ndim));
    const int side = a == t->o_stem ? 3 : nm.rfind("net.visual_encoder.", 0) == 0 ? 1 : nm.rfind("net.visual_fc.", 0) == 0 ? 2 : 0;
    if (b > a) es.push_back({a, b, side});
  }
  std::sort(es.begin(), es.end(), [](const Ent &x, const Ent &y) { return x.a < y.a; });
  PolicyTrain::Ranges *lists[3] = {&t->r_early, &t->r_enc, &t->r_vfc};
  for (auto *l : lists) l->clear();
  int prev = -1;
  for (const Ent &e : es) {
    if (e.side < 3) {
      if (e.side == prev) lists[e.side]->back().second = e.b;
      else lists[e.side]->push_back({e.a, e.b});
    }
    prev = e.side;
  }
}
// every range one backward reports, in its order
PolicyTrain::Ranges backward_ranges(Policy &p, const PolicyTrain *t, bool train_encoder, bool from_features) {
  PolicyTrain::Ranges out = t->r_early;
  if (from_features || !train_encoder) {
    out.insert(out.end(), t->r_vfc.begin(), t->r_vfc.end());
    return out;
  }
  uint64_t first[8], count[8];
  int n = 0;
  if (pnvo_train_grad_buckets(p.enc, first, count, 8, &n) == PNVO_OK)
    for (int k = 0; k < n && k < 8; ++k) {
      const PolicyTrain::Ranges pc = encoder_pieces(t, 2, (size_t)first[k], (size_t)(first[k] + count[k]));
      out.insert(out.end(), pc.begin(), pc.end());
    }
  out.push_back({t->o_stem, t->o_stem + (size_t)t->c0 * t->stem_row});
  return out;
}

// phase boundary k of the update step (only while timing is on)
hipError_t mark(PolicyTrain *t, int k, hipStream_t s) { return t->timing ? hipEventRecord(t->ev[k], s) : hipSuccess; }

// Before a regrow: the old workspace goes first (not old and new side by side), and a failed regrow leaves capM = 0.
void free_ws(PolicyTrain *t) {
  for (DevBuf<float> *b : {&t->pooled, &t->feat, &t->visual, &t->enc_out, &t->x0, &t->g3, &t->masks, &t->hid0, &t->logits, &t->value, &t->logp, &t->ent, &t->dlogits,
                           &t->dvalue, &t->dY, &t->dX0, &t->dG, &t->dGh, &t->dC})
    b->reset();
  t->rows.reset();
  t->actions.reset();
  for (auto *v : {&t->gates, &t->c, &t->y, &t->hm}) v->clear();
  t->capM = t->cap_pooled = t->cap_feat = 0;
}

int ensure_ws(Policy &p, PolicyTrain *t, int M) {
  if (M <= t->capM) return PNVO_OK;
  free_ws(t);
  const pnvo_policy_config &c = p.cfg;
  const size_t Hd = (size_t)c.hidden, K0 = Hd + 64, L = (size_t)c.rnn_layers, m = (size_t)M, A = (size_t)c.n_actions;
  PCHK(t->enc_out.alloc(m));
  PCHK(t->x0.alloc(m * K0));
  PCHK(t->g3.alloc(m * 3));
  PCHK(t->masks.alloc(m));
  PCHK(t->hid0.alloc(rnn_state_floats(c, M)));
  PCHK(t->rows.alloc(m));
  PCHK(t->actions.alloc(m));
  for (auto *v : {&t->gates, &t->c, &t->y, &t->hm}) v->resize(L);
  for (size_t l = 0; l < L; ++l) {
    PCHK(t->gates[l].alloc(m * 4 * Hd));
    PCHK(t->c[l].alloc(m * Hd));
    PCHK(t->y[l].alloc(m * Hd));
    PCHK(t->hm[l].alloc(m * Hd));
  }
  PCHK(t->logits.alloc(m * A));
  PCHK(t->value.alloc(m));
  PCHK(t->logp.alloc(m));
  PCHK(t->ent.alloc(m));
  PCHK(t->dlogits.alloc(m * A));
  PCHK(t->dvalue.alloc(m));
  PCHK(t->dY.alloc(m * Hd));
  PCHK(t->dX0.alloc(m * K0));
  PCHK(t->dG.alloc(m * 4 * Hd));
  if (is_gru(c)) PCHK(t->dGh.alloc(m * 3 * Hd));
  PCHK(t->dC.alloc(m * Hd));
  t->capM = M;
  return PNVO_OK;
}

// the input side's workspace of the two kinds of evaluate: pooled frames, or feature rows and visual_fc's output
int ensure_pooled(Policy &p, PolicyTrain *t, int M) {
  if (M <= t->cap_pooled) return PNVO_OK;
  t->pooled.reset();
  t->cap_pooled = 0;
  PCHK(t->pooled.alloc(policy_pooled_floats(p.cfg, M)));
  t->cap_pooled = M;
  return PNVO_OK;
}
int ensure_feat(Policy &p, PolicyTrain *t, int M) {
  if (M <= t->cap_feat) return PNVO_OK;
  t->feat.reset();
  t->visual.reset();
  t->cap_feat = 0;
  PCHK(t->feat.alloc((size_t)M * policy_feature_floats(p)));
  PCHK(t->visual.alloc((size_t)M * p.cfg.hidden));
  t->cap_feat = M;
  return PNVO_OK;
}

// the encoder handle's own parameter table inside the policy's flat buffer: the caller's entries where they are, the padded stem and
// the unused head in the tail
int attach_encoder(Policy &p, PolicyTrain *t, const std::vector<EncoderEntry> &ent, const pnvo_tensor_desc *toc) {
  std::vector<size_t> offs;
  size_t o_head = t->o_stem2 + (size_t)t->c0 * 2 * t->stem_row;
  for (const EncoderEntry &e : ent) {
    offs.push_back(e.src == EncoderEntry::VIEW ? (size_t)toc[e.k].offset : e.src == EncoderEntry::STEM ? t->o_stem2 : o_head);
    if (e.src == EncoderEntry::ZEROS) o_head += numel(e.shape);
  }
  const std::vector<pnvo_tensor_desc> etoc = encoder_toc(ent, offs);
  const int rc = pnvo_train_attach(p.enc, t->params, t->grads, t->n, etoc.data(), (int)etoc.size());
  if (rc != PNVO_OK) return pfail(rc, std::string("policy visual encoder: ") + pnvo_last_error(p.enc));
  return PNVO_OK;
}

size_t tail_floats(const pnvo_policy_config &c) { return (size_t)c.baseplanes * 98 * policy_channels(c) + (size_t)c.hidden + 1; }

}  // namespace

hipError_t launch_visual_fc_gemm(const float *feat, const float *w, const float *b, int rows, int F, int hidden, float *out, hipStream_t s) {
  GemmArgs g{feat, w, b, nullptr, out, rows, hidden, F, (long)F, 1, 1, (long)F, (long)hidden, 1};
  return launch_gemm<true, true>(g, s);
}

// ---- the kernels above as launches for simple_cnn_train.hip (pnvo_policy_state.h)
hipError_t launch_gemm_f32(const GemmArgs &g, bool akc, bool bkc, hipStream_t s) {
  if (akc) return bkc ? launch_gemm<true, true>(g, s) : launch_gemm<true, false>(g, s);
  return bkc ? launch_gemm<false, true>(g, s) : launch_gemm<false, false>(g, s);
}
hipError_t launch_gru_step(float *g, const float *h_prev, const float *w_hh, const float *b_hh, const float *masks, int N, int Hd, float *y,
                           float *hm, float *h_fin, hipStream_t s) {
  hipLaunchKernelGGL(gru_step_kernel, dim3((unsigned)Hd), dim3(192), 0, s, g, h_prev, w_hh, b_hh, masks, N, Hd, y, hm, h_fin);
  return hipGetLastError();
}
hipError_t launch_gru_bptt_step(const float *gates_t, const float *gates_n, const float *dgh_n, const float *dh_n, const float *mask_n,
                                const float *hm_t, const float *whhT, const float *dY_t, int N, int Hd, float *dgx_t, float *dgh_t,
                                float *dh_t, hipStream_t s) {
  hipLaunchKernelGGL(gru_bptt_step_kernel, dim3((unsigned)Hd), dim3(192), 0, s, gates_t, gates_n, dgh_n, dh_n, mask_n, hm_t, whhT, dY_t, N, Hd,
                     dgx_t, dgh_t, dh_t);
  return hipGetLastError();
}
hipError_t launch_heads_eval(const float *feat, const float *act_w, const float *act_b, const float *cr_w, const float *cr_b,
                             const int64_t *actions, int M, int Hd, int A, float *logits, float *value, float *logp, float *ent,
                             hipStream_t s) {
  hipLaunchKernelGGL(heads_eval_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, feat, act_w, act_b, cr_w, cr_b, actions, M, Hd, A, logits,
                     value, logp, ent);
  return hipGetLastError();
}
hipError_t launch_mean(const float *x, int n, float *out, hipStream_t s) {
  hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, s, x, n, out);
  return hipGetLastError();
}
hipError_t launch_ppo_loss(const float *logits, const float *value, const float *logp, const float *ent, const int64_t *actions,
                           const float *old_logp, const float *adv, const float *vpred, const float *ret, int M, int A, float clip, float vc,
                           float ec, int use_clipped, float *out3, float *dlogits, float *dvalue, hipStream_t s) {
  hipLaunchKernelGGL(ppo_loss_kernel, dim3(1), dim3(256), 0, s, logits, value, logp, ent, actions, old_logp, adv, vpred, ret, M, A, clip, vc, ec,
                     use_clipped, out3, dlogits, dvalue);
  return hipGetLastError();
}
hipError_t launch_heads_bwd(const float *feat, const float *dlogits, const float *dvalue, const float *act_w, const float *cr_w, int M, int Hd,
                            int A, float *g_act_w, float *g_act_b, float *g_cr_w, float *g_cr_b, float *dfeat, hipStream_t s) {
  hipLaunchKernelGGL(heads_bwd_w_kernel, dim3((unsigned)(((long)(A + 1) * Hd + 255) / 256)), dim3(256), 0, s, feat, dlogits, dvalue, M, Hd, A,
                     g_act_w, g_act_b, g_cr_w, g_cr_b);
  hipLaunchKernelGGL(heads_bwd_x_kernel, dim3((unsigned)(((long)M * Hd + 255) / 256)), dim3(256), 0, s, dlogits, dvalue, act_w, cr_w, M, Hd, A,
                     dfeat);
  return hipGetLastError();
}
hipError_t launch_transpose(const float *src, int R, int C, float *dst, hipStream_t s) {
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((C + 31) / 32), (unsigned)((R + 31) / 32)), dim3(256), 0, s, src, R, C, dst);
  return hipGetLastError();
}
hipError_t launch_clip_grad_norm(float *g, long n, float scale, float max_norm, double *sq_part, float *norm_out, hipStream_t s) {
  hipLaunchKernelGGL(sumsq_kernel, dim3(SQ_BLOCKS), dim3(256), 0, s, g, n, scale, sq_part);
  hipLaunchKernelGGL(clip_scale_kernel, dim3(SQ_BLOCKS), dim3(256), 0, s, g, n, sq_part, scale, max_norm, norm_out);
  return hipGetLastError();
}

void pnvo_policy_train_free(Policy &p) {
  PolicyTrain *t = p.train;
  if (!t) return;
  for (hipEvent_t &e : t->ev)
    if (e) (void)hipEventDestroy(e);
  delete t;
  p.train = nullptr;
}

}  // namespace pnvo

using namespace pnvo;

static int policy_evaluate_impl(pnvo_policy_handle h, const float *depth, const PolicyObs *obs, const float *vfeat, const float *goal,
                                const int64_t *prev_actions, const float *masks, const float *hidden_in, int T, int N, const int64_t *actions,
                                float *hidden_out, float *value, float *logp, float *entropy, void *stream);

extern "C" {

size_t pnvo_policy_train_tail_floats(pnvo_policy_handle h) { return h ? tail_floats(h->p.cfg) : 0; }

int pnvo_policy_train_attach(pnvo_policy_handle h, float *params, float *grads, size_t n_floats, const pnvo_tensor_desc *toc, int ntoc) {
  if (!h || !params || !grads || !toc) return pfail(PNVO_ERR_ARG, "null argument");
  Policy &p = h->p;
  if (!p.loaded) return pfail(PNVO_ERR_STATE, "pnvo_policy_train_attach before pnvo_policy_load_weights");
  PCHK(hipSetDevice(p.device));
  const pnvo_policy_config &c = p.cfg;
  const int Hd = c.hidden;
  int rc = PNVO_OK;
  std::vector<EncoderEntry> ent;
  if ((rc = policy_encoder_table(p, toc, ntoc, n_floats, &ent)) != PNVO_OK) return rc;     // (checks every entry's range)
  size_t n_named = 0, o_stem = n_floats;
  for (int k = 0; k < ntoc; ++k)
    n_named = std::max(n_named, (size_t)toc[k].offset + numel(std::vector<int64_t>(toc[k].shape, toc[k].shape + toc[k].ndim)));
  for (const EncoderEntry &e : ent)
    if (e.src == EncoderEntry::STEM) o_stem = (size_t)toc[e.k].offset;
  if (o_stem == n_floats) return pfail(PNVO_ERR_WEIGHTS, "parameter table is missing the visual encoder's stem weight");
  if (n_floats < n_named + tail_floats(c))
    return pfail(PNVO_ERR_ARG, "flat buffers hold " + std::to_string(n_floats) + " floats; the " + std::to_string(n_named) +
                                   " of the parameter table need " + std::to_string(tail_floats(c)) +
                                   " more behind them (pnvo_policy_train_tail_floats)");
  if (((uintptr_t)params & 15) != 0) return pfail(PNVO_ERR_ARG, "flat parameter buffer is not 16-byte aligned");
  const std::vector<PolicyParam> tab = policy_params(p);
  std::vector<size_t> offs;
  for (const PolicyParam &e : tab) {
    const pnvo_tensor_desc *d = policy_find(toc, ntoc, e, n_floats, &rc);
    if (!d) return rc;
    if (e.rows_as_float4 && d->offset % 4 != 0)
      return pfail(PNVO_ERR_ARG, "parameter '" + e.name + "' starts at float " + std::to_string(d->offset) +
                                     ", not a multiple of 4 (its rows are read as float4)");
    offs.push_back((size_t)d->offset);
  }
  pnvo_policy_train_free(p);
  PolicyTrain *t = new PolicyTrain();
  p.train = t;
  t->params = params;
  t->grads = grads;
  t->n = n_floats;
  t->n_named = n_named;
  t->c0 = c.baseplanes;
  t->stem_row = 49 * policy_channels(c);
  t->o_stem = o_stem;
  t->o_stem2 = n_named;
  rc = [&]() -> int {
    // tail: zero-padded stem + zero output head, gradients zero
    PCHK(hipMemset(params + n_named, 0, tail_floats(c) * sizeof(float)));
    PCHK(hipMemset(grads + n_named, 0, tail_floats(c) * sizeof(float)));
    hipLaunchKernelGGL(stem_pad_kernel, dim3((unsigned)((t->c0 * 2 * t->stem_row + 255) / 256)), dim3(256), 0, nullptr, params + t->o_stem,
                       t->c0, t->stem_row, params + t->o_stem2);
    PCHK(hipGetLastError());
    PCHK(t->whhT.alloc((size_t)4 * Hd * Hd));
    PCHK(t->sq_part.alloc(SQ_BLOCKS));
    build_ranges(t, toc, ntoc);
    // a non-resnet18 encoder stays what pnvo_policy_load_weights made it: frozen, on its own copy of the weights
    // (pnvo_policy_train_reload_encoder re-reads them from the flat buffer)
    if (!policy_resnet18(c)) return PNVO_OK;
    const int rc2 = attach_encoder(p, t, ent, toc);
    if (rc2 != PNVO_OK) return rc2;
    // the encoder handle's reports pass through encoder_hook (a no-op until pnvo_policy_set_grad_hook names a receiver)
    if (pnvo_train_set_grad_hook(p.enc, encoder_hook, t) != PNVO_OK) return pfail(PNVO_ERR_STATE, std::string("policy visual encoder: ") + pnvo_last_error(p.enc));
    return PNVO_OK;
  }();
  if (rc != PNVO_OK) {                  // no half-built train step is left behind
    pnvo_policy_train_free(p);
    return rc;
  }
  // the recurrent part and the heads read the flat buffer from now on (pnvo_policy_act included): no second copy
  p.owned.clear();
  p.attached = true;
  for (size_t i = 0; i < tab.size(); ++i) *tab[i].slot = params + offs[i];
  PCHK(hipDeviceSynchronize());
  return PNVO_OK;
}

int pnvo_policy_train_refresh(pnvo_policy_handle h, void *stream) {
  if (!h || !h->p.train) return pfail(PNVO_ERR_STATE, "pnvo_policy_train_attach first");
  Policy &p = h->p;
  PolicyTrain *t = p.train;
  PCHK(hipSetDevice(p.device));
  hipLaunchKernelGGL(stem_pad_kernel, dim3((unsigned)((t->c0 * 2 * t->stem_row + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     t->params + t->o_stem, t->c0, t->stem_row, t->params + t->o_stem2);
  PCHK(hipGetLastError());
  if (!policy_resnet18(p.cfg)) return PNVO_OK;           // frozen encoder on its own copy of the weights: nothing moved
  const int rc = pnvo_train_refresh(p.enc, stream);
  if (rc != PNVO_OK) return pfail(rc, std::string("policy visual encoder: ") + pnvo_last_error(p.enc));
  return PNVO_OK;
}

int pnvo_policy_train_reload_encoder(pnvo_policy_handle h, const pnvo_tensor_desc *toc, int ntoc, void *stream) {
  if (!h || !h->p.train || !toc) return pfail(PNVO_ERR_STATE, "pnvo_policy_train_attach first");
  Policy &p = h->p;
  PolicyTrain *t = p.train;
  if (policy_resnet18(p.cfg)) return pnvo_policy_train_refresh(h, stream);   // attached encoders re-pack on the device
  PCHK(hipSetDevice(p.device));
  std::vector<EncoderEntry> ent;
  int rc = policy_encoder_table(p, toc, ntoc, t->n, &ent);
  if (rc != PNVO_OK) return rc;
  PCHK(hipStreamSynchronize((hipStream_t)stream));
  std::vector<float> host(t->n_named);
  PCHK(hipMemcpy(host.data(), t->params, t->n_named * sizeof(float), hipMemcpyDeviceToHost));
  std::vector<float> eblob;
  std::vector<size_t> offs;
  for (const EncoderEntry &e : ent) {
    offs.push_back(eblob.size());
    const size_t cnt = numel(e.shape);
    if (e.src == EncoderEntry::VIEW) {
      eblob.insert(eblob.end(), host.begin() + toc[e.k].offset, host.begin() + toc[e.k].offset + cnt);
    } else {
      eblob.insert(eblob.end(), cnt, 0.f);
      if (e.src == EncoderEntry::STEM) {
        const size_t row = (size_t)t->stem_row;
        for (int64_t o = 0; o < e.shape[0]; ++o)
          std::memcpy(&eblob[offs.back() + (size_t)o * 2 * row], host.data() + toc[e.k].offset + o * row, sizeof(float) * row);
      }
    }
  }
  if (p.cfg.normalize) {
    const int64_t C2 = 2 * policy_channels(p.cfg);
    for (int k = 0; k < 2; ++k) {
      ent.push_back({std::string("visual_encoder.running_mean_and_var.") + (k ? "_var" : "_mean"), {1, C2, 1, 1}, EncoderEntry::ZEROS, -1});
      offs.push_back(eblob.size());
      eblob.insert(eblob.end(), (size_t)C2, k ? 1.f : 0.f);
    }
  }
  const std::vector<pnvo_tensor_desc> etoc = encoder_toc(ent, offs);
  rc = pnvo_load_weights(p.enc, eblob.data(), eblob.size(), etoc.data(), (int)etoc.size());
  if (rc != PNVO_OK) return pfail(rc, std::string("policy visual encoder: ") + pnvo_last_error(p.enc));
  return PNVO_OK;
}

int pnvo_policy_evaluate(pnvo_policy_handle h, const float *depth, const float *goal, const int64_t *prev_actions, const float *masks,
                         const float *hidden_in, int T, int N, const int64_t *actions, int train_encoder, float *hidden_out,
                         float *value, float *logp, float *entropy, void *stream) {
  (void)train_encoder;                   // the forward is the same either way: visual_fc's gradient needs the saved activations
  if (!depth) return pfail(PNVO_ERR_ARG, "null argument");
  if (h && !policy_is_plain(h->p.cfg))
    return pfail(PNVO_ERR_STATE, "pnvo_policy_evaluate: this policy takes rgb and / or RunningMeanAndVar statistics: call pnvo_policy_evaluate_rgbd");
  return policy_evaluate_impl(h, depth, nullptr, nullptr, goal, prev_actions, masks, hidden_in, T, N, actions, hidden_out, value, logp, entropy, stream);
}

int pnvo_policy_evaluate_features(pnvo_policy_handle h, const float *visual_features, const float *goal, const int64_t *prev_actions,
                                  const float *masks, const float *hidden_in, int T, int N, const int64_t *actions, float *hidden_out,
                                  float *value, float *logp, float *entropy, void *stream) {
  if (!visual_features) return pfail(PNVO_ERR_ARG, "null argument");
  return policy_evaluate_impl(h, nullptr, nullptr, visual_features, goal, prev_actions, masks, hidden_in, T, N, actions, hidden_out, value, logp,
                              entropy, stream);
}

int pnvo_policy_evaluate_rgbd(pnvo_policy_handle h, const void *rgb, int rgb_is_u8, const float *depth, float *run_mean, float *run_var,
                              float *run_count, int training, const float *goal, const int64_t *prev_actions, const float *masks,
                              const float *hidden_in, int T, int N, const int64_t *actions, int train_encoder, float *hidden_out,
                              float *value, float *logp, float *entropy, void *stream) {
  if (!h) return pfail(PNVO_ERR_ARG, "null handle");
  if (policy_is_plain(h->p.cfg) && !rgb && !run_mean && !run_var && !run_count && !training)
    return pnvo_policy_evaluate(h, depth, goal, prev_actions, masks, hidden_in, T, N, actions, train_encoder, hidden_out, value, logp, entropy,
                                stream);
  PolicyObs o;
  o.rgb = rgb, o.rgb_is_u8 = rgb_is_u8, o.depth = depth, o.mean = run_mean, o.var = run_var, o.count = run_count, o.training = training;
  return policy_evaluate_impl(h, nullptr, &o, nullptr, goal, prev_actions, masks, hidden_in, T, N, actions, hidden_out, value, logp, entropy,
                              stream);
}

}  // extern "C"

// the shared body of pnvo_policy_evaluate (depth given), pnvo_policy_evaluate_rgbd (obs given) and pnvo_policy_evaluate_features (vfeat given)
static int policy_evaluate_impl(pnvo_policy_handle h, const float *depth, const PolicyObs *obs, const float *vfeat, const float *goal,
                                const int64_t *prev_actions, const float *masks, const float *hidden_in, int T, int N, const int64_t *actions,
                                float *hidden_out, float *value, float *logp, float *entropy, void *stream) {
  if (!h || !h->p.train) return pfail(PNVO_ERR_STATE, "pnvo_policy_train_attach first");
  Policy &p = h->p;
  PolicyTrain *t = p.train;
  if (!vfeat && !policy_resnet18(p.cfg))
    return pfail(PNVO_ERR_STATE, "evaluate from frames runs the encoder's training forward, which a non-resnet18 backbone does not have: encode the "
                                 "frames (pnvo_policy_encode / _encode_rgbd) and call pnvo_policy_evaluate_features (RL.DDPPO.train_encoder: False)");
  if (T <= 0 || N <= 0 || (long)T * N > (1L << 20))
    return pfail(PNVO_ERR_ARG, "bad rollout shape T = " + std::to_string(T) + ", N = " + std::to_string(N));
  if (obs)
    if (int rc0 = policy_obs_check(p, *obs, "pnvo_policy_evaluate_rgbd")) return rc0;
  if ((!depth && !obs && !vfeat) || !goal || !prev_actions || !masks || !hidden_in || !actions || !hidden_out)
    return pfail(PNVO_ERR_ARG, "null argument");
  const pnvo_policy_config &c = p.cfg;
  const int Hd = c.hidden, L = c.rnn_layers, K0 = Hd + 64, A = c.n_actions, M = T * N;
  const bool gru = is_gru(c);
  if (hidden_states_overlap(hidden_in, hidden_out, rnn_state_floats(c, N)))
    return pfail(PNVO_ERR_ARG, std::string("hidden_out overlaps hidden_in (each holds ") + (gru ? "" : "2 * ") +
                                   "rnn_layers * N * hidden floats): pass separate buffers");
  PCHK(hipSetDevice(p.device));
  hipStream_t s = (hipStream_t)stream;
  int rc = ensure_ws(p, t, M);
  if (rc != PNVO_OK) return rc;
  if ((rc = (depth || obs) ? ensure_pooled(p, t, M) : ensure_feat(p, t, M)) != PNVO_OK) return rc;
  t->from_features = vfeat != nullptr;
  t->T = T;
  t->N = N;
  t->M = M;
  t->have_loss = false;
  // what the backward reads later is kept here: the caller's tensors may be gone by then
  PCHK(hipMemcpyAsync(t->masks, masks, (size_t)M * sizeof(float), hipMemcpyDeviceToDevice, s));
  PCHK(hipMemcpyAsync(t->actions, actions, (size_t)M * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  PCHK(hipMemcpyAsync(t->hid0, hidden_in, rnn_state_floats(c, N) * sizeof(float), hipMemcpyDeviceToDevice, s));
  const float *visual = nullptr;
  if (depth || obs) {
    PCHK(mark(t, 0, s));
    // the M = T * N rows are ONE batch of RunningMeanAndVar (policy.py:52-63 runs the net once over the minibatch); the train-mode
    // forward takes the statistics over the handle's 2C channels, as the input stage padded them
    if ((rc = obs ? policy_input_stage(p, *obs, M, t->pooled, s) : pnvo_avgpool2(depth, M, c.height, c.width, t->pooled, stream)) != PNVO_OK)
      return rc;
    const bool norm = c.normalize != 0;
    rc = pnvo_train_forward(p.enc, nullptr, t->pooled, nullptr, nullptr, M, norm ? (const float *)p.mean_pad : nullptr,
                            norm ? (const float *)p.var_pad : nullptr, t->enc_out, stream);
    if (rc != PNVO_OK) return pfail(rc, std::string("policy visual encoder: ") + pnvo_last_error(p.enc));
    PCHK(mark(t, 1, s));
    visual = pnvo_train_hidden(p.enc);
    if (!visual) return pfail(PNVO_ERR_STATE, "policy visual encoder kept no hidden vector");
  } else {                               // the encoder does not run: visual_fc on the caller's features, kept for dW = d visual^T . features
    PCHK(hipMemcpyAsync(t->feat, vfeat, (size_t)M * policy_feature_floats(p) * sizeof(float), hipMemcpyDeviceToDevice, s));
    PCHK(mark(t, 0, s));
    if ((rc = launch_visual_fc(p, t->feat, M, t->visual, s)) != PNVO_OK) return rc;
    PCHK(mark(t, 1, s));
    visual = t->visual;
  }
  PCHK(launch_policy_inputs(p, visual, goal, prev_actions, t->masks, M, t->x0, t->rows, t->g3, s));
  const float *xin = t->x0;
  int K = K0;
  for (int l = 0; gru && l < L; ++l) {
    // G_x into blocks 0 .. 2 of the [M, 4H] gate rows; b_hh is added by the step (b_hn belongs inside r * (...))
    GemmArgs g{xin, p.w_ih[l], p.b_ih[l], nullptr, t->gates[l], M, 3 * Hd, K, (long)K, 1, 1, (long)K, 4L * Hd};
    PCHK((launch_gemm<true, true>(g, s)));
    for (int ts = 0; ts < T; ++ts) {
      const size_t r = (size_t)ts * N;
      const float *h_prev = ts ? t->y[l] + (r - N) * Hd : t->hid0 + (size_t)l * N * Hd;
      hipLaunchKernelGGL(gru_step_kernel, dim3((unsigned)Hd), dim3(192), 0, s, t->gates[l] + r * 4 * Hd, h_prev, p.w_hh[l], p.b_hh[l],
                         t->masks + r, N, Hd, t->y[l] + r * Hd, t->hm[l] + r * Hd, ts == T - 1 ? hidden_out + (size_t)l * N * Hd : nullptr);
    }
    xin = t->y[l];
    K = Hd;
  }
  for (int l = 0; !gru && l < L; ++l) {
    GemmArgs g{xin, p.w_ih[l], p.b_ih[l], p.b_hh[l], t->gates[l], M, 4 * Hd, K, (long)K, 1, 1, (long)K, 4L * Hd};
    PCHK((launch_gemm<true, true>(g, s)));
    for (int ts = 0; ts < T; ++ts) {
      const size_t r = (size_t)ts * N;
      const float *h_prev = ts ? t->y[l] + (r - N) * Hd : t->hid0 + (size_t)l * N * Hd;
      const float *c_prev = ts ? t->c[l] + (r - N) * Hd : t->hid0 + (size_t)(L + l) * N * Hd;
      const bool last = ts == T - 1;
      hipLaunchKernelGGL(lstm_step_kernel, dim3((unsigned)Hd), dim3(256), 0, s, t->gates[l] + r * 4 * Hd, h_prev, c_prev, p.w_hh[l],
                         t->masks + r, N, Hd, t->y[l] + r * Hd, t->c[l] + r * Hd, t->hm[l] + r * Hd,
                         last ? hidden_out + (size_t)l * N * Hd : nullptr, last ? hidden_out + (size_t)(L + l) * N * Hd : nullptr);
    }
    xin = t->y[l];
    K = Hd;
  }
  hipLaunchKernelGGL(heads_eval_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, t->y[L - 1], p.act_w, p.act_b, p.cr_w, p.cr_b,
                     t->actions, M, Hd, A, t->logits, t->value, t->logp, t->ent);
  if (value) PCHK(hipMemcpyAsync(value, t->value, (size_t)M * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (logp) PCHK(hipMemcpyAsync(logp, t->logp, (size_t)M * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (entropy) hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, s, t->ent, M, entropy);
  PCHK(hipGetLastError());
  PCHK(mark(t, 2, s));
  return PNVO_OK;
}

extern "C" {

int pnvo_policy_ppo_loss(pnvo_policy_handle h, const float *actions_logp_old, const float *adv, const float *value_preds,
                         const float *returns, float clip, float value_coef, float entropy_coef, int use_clipped_value_loss, float *out3,
                         void *stream) {
  if (!h || !h->p.train) return pfail(PNVO_ERR_STATE, "pnvo_policy_train_attach first");
  Policy &p = h->p;
  PolicyTrain *t = p.train;
  if (t->M <= 0) return pfail(PNVO_ERR_STATE, "pnvo_policy_ppo_loss before pnvo_policy_evaluate");
  if (!actions_logp_old || !adv || !returns || !out3 || (use_clipped_value_loss && !value_preds)) return pfail(PNVO_ERR_ARG, "null argument");
  if (!(clip >= 0.f)) return pfail(PNVO_ERR_ARG, "clip_param " + std::to_string(clip) + " must be >= 0");
  PCHK(hipSetDevice(p.device));
  PCHK(mark(t, 3, (hipStream_t)stream));
  hipLaunchKernelGGL(ppo_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, t->logits, t->value, t->logp, t->ent, t->actions,
                     actions_logp_old, adv, value_preds, returns, t->M, p.cfg.n_actions, clip, value_coef, entropy_coef,
                     use_clipped_value_loss ? 1 : 0, out3, t->dlogits, t->dvalue);
  PCHK(hipGetLastError());
  PCHK(mark(t, 4, (hipStream_t)stream));
  t->have_loss = true;
  return PNVO_OK;
}

int pnvo_policy_backward(pnvo_policy_handle h, int train_encoder, void *stream) {
  if (!h || !h->p.train) return pfail(PNVO_ERR_STATE, "pnvo_policy_train_attach first");
  Policy &p = h->p;
  PolicyTrain *t = p.train;
  if (t->M <= 0 || !t->have_loss) return pfail(PNVO_ERR_STATE, "pnvo_policy_backward before pnvo_policy_evaluate + pnvo_policy_ppo_loss");
  if (train_encoder && !policy_resnet18(p.cfg))
    return pfail(PNVO_ERR_STATE, "pnvo_policy_backward: a non-resnet18 encoder has no backward (RL.DDPPO.train_encoder: False)");
  PCHK(hipSetDevice(p.device));
  hipStream_t s = (hipStream_t)stream;
  const pnvo_policy_config &c = p.cfg;
  const int Hd = c.hidden, L = c.rnn_layers, K0 = Hd + 64, A = c.n_actions, M = t->M, T = t->T, N = t->N;
  float *G = t->grads;
  PCHK(mark(t, 5, s));
  PCHK(hipMemsetAsync(G, 0, t->n * sizeof(float), s));                 // overwrite semantics; a frozen encoder's range stays zero
  const float *feat = t->y[L - 1];
  hipLaunchKernelGGL(heads_bwd_w_kernel, dim3((unsigned)(((long)(A + 1) * Hd + 255) / 256)), dim3(256), 0, s, feat, t->dlogits, t->dvalue, M,
                     Hd, A, grad_of(t, p.act_w), grad_of(t, p.act_b), grad_of(t, p.cr_w), grad_of(t, p.cr_b));
  hipLaunchKernelGGL(heads_bwd_x_kernel, dim3((unsigned)(((long)M * Hd + 255) / 256)), dim3(256), 0, s, t->dlogits, t->dvalue, p.act_w,
                     p.cr_w, M, Hd, A, t->dY);
  const bool gru = is_gru(c);
  for (int l = L - 1; gru && l >= 0; --l) {
    const int K = l == 0 ? K0 : Hd, G3 = 3 * Hd;
    const float *X = l == 0 ? t->x0 : t->y[l - 1];
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((Hd + 31) / 32), (unsigned)((G3 + 31) / 32)), dim3(256), 0, s, p.w_hh[l], G3, Hd,
                       t->whhT);
    for (int ts = T - 1; ts >= 0; --ts) {
      const size_t r = (size_t)ts * N, rn = r + N;
      const bool last = ts == T - 1;
      hipLaunchKernelGGL(gru_bptt_step_kernel, dim3((unsigned)Hd), dim3(192), 0, s, t->gates[l] + r * 4 * Hd,
                         last ? nullptr : t->gates[l] + rn * 4 * Hd, last ? nullptr : t->dGh + rn * G3, last ? nullptr : t->dC + rn * Hd,
                         last ? nullptr : t->masks + rn, t->hm[l] + r * Hd, t->whhT, t->dY + r * Hd, N, Hd, t->dG + r * G3, t->dGh + r * G3,
                         t->dC + r * Hd);
    }
    // dW_ih = dGx^T . X,  dW_hh = dGh^T . (h_prev * mask),  db_ih = colsum(dGx),  db_hh = colsum(dGh),  dX = dGx . W_ih
    GemmArgs wi{t->dG, X, nullptr, nullptr, grad_of(t, p.w_ih[l]), G3, K, M, 1, (long)G3, (long)K, 1, (long)K};
    PCHK((launch_gemm<false, false>(wi, s)));
    GemmArgs wh{t->dGh, t->hm[l], nullptr, nullptr, grad_of(t, p.w_hh[l]), G3, Hd, M, 1, (long)G3, (long)Hd, 1, (long)Hd};
    PCHK((launch_gemm<false, false>(wh, s)));
    PCHK(launch_colsum(t->dG, M, G3, G3, grad_of(t, p.b_ih[l]), s));
    PCHK(launch_colsum(t->dGh, M, G3, G3, grad_of(t, p.b_hh[l]), s));
    GemmArgs dx{t->dG, p.w_ih[l], nullptr, nullptr, l == 0 ? t->dX0 : t->dY, M, K, G3, (long)G3, 1, (long)K, 1, (long)K};
    PCHK((launch_gemm<true, false>(dx, s)));
  }
  for (int l = L - 1; !gru && l >= 0; --l) {
    const int K = l == 0 ? K0 : Hd;
    const float *X = l == 0 ? t->x0 : t->y[l - 1];
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((Hd + 31) / 32), (unsigned)((4 * Hd + 31) / 32)), dim3(256), 0, s, p.w_hh[l], 4 * Hd,
                       Hd, t->whhT);
    for (int ts = T - 1; ts >= 0; --ts) {
      const size_t r = (size_t)ts * N, rn = r + N;
      const bool last = ts == T - 1;
      const float *c_prev = ts ? t->c[l] + (r - N) * Hd : t->hid0 + (size_t)(L + l) * N * Hd;
      hipLaunchKernelGGL(bptt_step_kernel, dim3((unsigned)Hd), dim3(256), 0, s, t->gates[l] + r * 4 * Hd,
                         last ? nullptr : t->gates[l] + rn * 4 * Hd, last ? nullptr : t->dG + rn * 4 * Hd, last ? nullptr : t->dC + rn * Hd,
                         last ? nullptr : t->masks + rn, t->c[l] + r * Hd, c_prev, t->masks + r, t->whhT, t->dY + r * Hd, N, Hd,
                         t->dG + r * 4 * Hd, t->dC + r * Hd);
    }
    // dW_ih = dG^T . X,  dW_hh = dG^T . (h_prev * mask),  db_ih = db_hh = colsum(dG),  dX = dG . W_ih
    GemmArgs wi{t->dG, X, nullptr, nullptr, grad_of(t, p.w_ih[l]), 4 * Hd, K, M, 1, 4L * Hd, (long)K, 1, (long)K};
    PCHK((launch_gemm<false, false>(wi, s)));
    GemmArgs wh{t->dG, t->hm[l], nullptr, nullptr, grad_of(t, p.w_hh[l]), 4 * Hd, Hd, M, 1, 4L * Hd, (long)Hd, 1, (long)Hd};
    PCHK((launch_gemm<false, false>(wh, s)));
    PCHK(launch_colsum(t->dG, M, 4 * Hd, 4 * Hd, grad_of(t, p.b_ih[l]), s));
    PCHK(hipMemcpyAsync(grad_of(t, p.b_hh[l]), grad_of(t, p.b_ih[l]), (size_t)4 * Hd * sizeof(float), hipMemcpyDeviceToDevice, s));
    GemmArgs dx{t->dG, p.w_ih[l], nullptr, nullptr, l == 0 ? t->dX0 : t->dY, M, K, 4 * Hd, 4L * Hd, 1, (long)K, 1, (long)K};
    PCHK((launch_gemm<true, false>(dx, s)));
  }
  // embeddings; d visual -> dY (contiguous [M, hidden]) -> the encoder's backward below its output head
  hipLaunchKernelGGL(inputs_bwd_kernel, dim3((unsigned)(((long)M * Hd + 128 + (long)(A + 1) * 32 + 255) / 256)), dim3(256), 0, s, t->dX0,
                     t->rows, t->g3, M, Hd, A + 1, grad_of(t, p.tgt_w), grad_of(t, p.tgt_b), grad_of(t, p.emb), t->dY);
  PCHK(hipGetLastError());
  PCHK(mark(t, 6, s));
  report(t, t->r_early, s);             // embeddings, recurrent tensors, heads: final; they can travel while the encoder's backward runs
  if (t->from_features) {
    // visual_fc alone, whatever train_encoder says: nothing of the encoder ran, and no gradient is taken with respect to the features.
    // d visual (t->dY) through the ReLU, dW = d visual^T . features, db = colsum(d visual); the encoder's range stays at the memset's zeros
    const int F = (int)policy_feature_floats(p);
    hipLaunchKernelGGL(relu_mask_kernel, dim3((unsigned)(((long)M * Hd + 255) / 256)), dim3(256), 0, s, t->visual, (long)M * Hd, t->dY);
    PCHK(hipGetLastError());
    GemmArgs dw{t->dY, t->feat, nullptr, nullptr, grad_of(t, p.vfc_w), Hd, F, M, 1, (long)Hd, (long)F, 1, (long)F};
    PCHK((launch_gemm<false, false>(dw, s)));
    PCHK(launch_colsum(t->dY, M, Hd, Hd, grad_of(t, p.vfc_b), s));
    report(t, t->r_vfc, s);
    PCHK(mark(t, 7, s));
    return PNVO_OK;
  }
  t->enc_pass = train_encoder ? 2 : 1;
  const int rc = pnvo_train_backward_from_hidden(p.enc, t->dY, train_encoder == 0, stream);
  t->enc_pass = 0;
  if (rc != PNVO_OK) return pfail(rc, std::string("policy visual encoder: ") + pnvo_last_error(p.enc));
  if (train_encoder) {
    hipLaunchKernelGGL(stem_unpad_kernel, dim3((unsigned)((t->c0 * t->stem_row + 255) / 256)), dim3(256), 0, s, G + t->o_stem2, t->c0, t->stem_row,
                       G + t->o_stem);
    PCHK(hipGetLastError());
    report(t, {{t->o_stem, t->o_stem + (size_t)t->c0 * t->stem_row}}, s);
  }
  PCHK(mark(t, 7, s));
  return PNVO_OK;
}

int pnvo_policy_train_timing(pnvo_policy_handle h, int mode) {
  if (!h || !h->p.train) return pfail(PNVO_ERR_STATE, "pnvo_policy_train_attach first");
  PolicyTrain *t = h->p.train;
  PCHK(hipSetDevice(h->p.device));
  if (mode)
    for (hipEvent_t &e : t->ev)
      if (!e) PCHK(hipEventCreate(&e));
  t->timing = mode != 0;
  return PNVO_OK;
}

int pnvo_policy_train_timing_read(pnvo_policy_handle h, double ms[5]) {
  if (!h || !h->p.train || !ms) return pfail(PNVO_ERR_STATE, "pnvo_policy_train_attach first");
  PolicyTrain *t = h->p.train;
  if (!t->timing) return pfail(PNVO_ERR_STATE, "pnvo_policy_train_timing(h, 1) first");
  PCHK(hipEventSynchronize(t->ev[7]));
  const int pairs[5][2] = {{0, 1}, {1, 2}, {3, 4}, {5, 6}, {6, 7}};
  for (int k = 0; k < 5; ++k) {
    float f = 0.f;
    PCHK(hipEventElapsedTime(&f, t->ev[pairs[k][0]], t->ev[pairs[k][1]]));
    ms[k] = (double)f;
  }
  return PNVO_OK;
}

static int clip_grad_norm_impl(pnvo_policy_handle h, float scale, float max_norm, float *norm_out, void *stream) {
  Policy &p = h->p;
  PolicyTrain *t = p.train;
  PCHK(hipSetDevice(p.device));
  const long n = (long)t->n_named;
  hipLaunchKernelGGL(sumsq_kernel, dim3(SQ_BLOCKS), dim3(256), 0, (hipStream_t)stream, t->grads, n, scale, t->sq_part);
  hipLaunchKernelGGL(clip_scale_kernel, dim3(SQ_BLOCKS), dim3(256), 0, (hipStream_t)stream, t->grads, n, t->sq_part, scale, max_norm, norm_out);
  PCHK(hipGetLastError());
  return PNVO_OK;
}

int pnvo_policy_clip_grad_norm(pnvo_policy_handle h, float max_norm, float *norm_out, void *stream) {
  if (!h || !h->p.train) return pfail(PNVO_ERR_STATE, "pnvo_policy_train_attach first");
  if (!(max_norm > 0.f)) return pfail(PNVO_ERR_ARG, "max_grad_norm " + std::to_string(max_norm) + " must be > 0");
  return clip_grad_norm_impl(h, 1.f, max_norm, norm_out, stream);
}

int pnvo_policy_clip_grad_norm_scaled(pnvo_policy_handle h, float scale, float max_norm, float *norm_out, void *stream) {
  if (!h || !h->p.train) return pfail(PNVO_ERR_STATE, "pnvo_policy_train_attach first");
  if (!std::isfinite(scale) || !(scale > 0.f)) return pfail(PNVO_ERR_ARG, "gradient scale " + std::to_string(scale) + " must be finite and > 0");
  if (std::isnan(max_norm)) return pfail(PNVO_ERR_ARG, "max_grad_norm is NaN");
  return clip_grad_norm_impl(h, scale, max_norm > 0.f ? max_norm : 0.f, norm_out, stream);
}

int pnvo_policy_set_grad_hook(pnvo_policy_handle h, pnvo_grad_ready_fn fn, void *user) {
  if (!h || !h->p.train) return pfail(PNVO_ERR_STATE, "pnvo_policy_train_attach first");
  h->p.train->hook = fn;
  h->p.train->hook_user = fn ? user : nullptr;
  return PNVO_OK;
}

int pnvo_policy_grad_buckets(pnvo_policy_handle h, int train_encoder, int from_features, uint64_t *first, uint64_t *count, int cap,
                             int *n_out) {
  if (!h || !h->p.train || !n_out) return pfail(PNVO_ERR_STATE, "pnvo_policy_train_attach first");
  const PolicyTrain::Ranges r = backward_ranges(h->p, h->p.train, train_encoder != 0, from_features != 0);
  *n_out = (int)r.size();
  for (int k = 0; k < *n_out && k < cap && first && count; ++k) {
    first[k] = (uint64_t)r[k].first;
    count[k] = (uint64_t)(r[k].second - r[k].first);
  }
  return PNVO_OK;
}

}  // extern "C"
