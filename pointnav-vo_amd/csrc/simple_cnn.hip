// simple_cnn.hip — the baseline navigation policy's per-step forward (pnvo_baseline_*), gfx950 only.
//
// PointNavBaselinePolicy (reference: pointnav_vo/rl/ppo/policy.py:82-163; SimpleCNN, model_utils/visual_encoders/simple_cnn.py:73-98,
// 140-160; RNNStateEncoder's defaults, model_utils/rnns/rnn_state_encoder.py:6-30):
//   cat([rgb / 255, depth]) NCHW -> Conv(C->32, 8x8, s4) + b + ReLU -> Conv(32->64, 4x4, s2) + b + ReLU -> Conv(64->32, 3x3, s1) + b
//   -> Flatten (NCHW) -> Linear(32 h w -> hidden) + b + ReLU;  x = [embed | goal] -> one GRU layer -> action logits and value.
// None of the encoder's kernels elsewhere fits: bias and no GroupNorm behind any conv, pad 0, strides 4 and 2, 1 / 3 / 4 input channels,
// and a Linear of 32 h w inputs (24 960 at 341 x 192: a 51 MB float32 weight) against 1 - 32 rows.  With no normalisation behind them the
// layers keep float32 operands throughout:
//   conv_tile_kernel   the three convs as one template: an implicit GEMM of (TM * 16 output pixels) x (all output channels) per workgroup
//                      on float32 FMA chains, K = (ky, kx, c) in 64-wide chunks through LDS.  Every output element is ONE chain over k in
//                      ascending order, so its bits depend neither on the tile shape nor on where its pixel sits in the batch.  conv1's
//                      loader reads the sensor frames themselves (NHWC rgb uint8 / float32 and depth): / 255 and the channel
//                      concatenation happen on the way into LDS, no assembled input tensor exists.  Activations are NHWC.
//   fc_splitk_kernel   the Linear on v_mfma_f32_16x16x4_f32: workgroup = 16 hidden units x one K slice x up to 32 batch rows, wave = every
//                      fourth 16-float step of the slice; the lanes load weight and activation rows straight into the MFMA operand
//                      layout (float4 = four consecutive k per lane), the four waves' tiles are added in wave order, one partial tile per
//                      slice goes to memory.  The slices depend on F alone: the weight is streamed once per call up to 32 rows.  The NCHW
//                      flatten order is met by permuting the weight's columns at load (conv3 writes NHWC).
//   fc_sum_inputs_kernel  partial sums in slice order + bias + ReLU -> the embedding, written (with the goal behind it and zeros up to a
//                      multiple of four floats) as the GRU's input row, and to `embed` when the caller wants it.
// The GRU layer and the heads are pnvo_policy.hip's gru_layer_kernel / policy_heads_kernel; weight_ih_l0 is re-laid to the padded pitch.
// No atomics anywhere: the same inputs give the same bits on every run and at every batch size.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pnvo.h"
#include "pnvo_internal.h"
#include "pnvo_model.h"
#include "pnvo_baseline_state.h"
#include "pnvo_policy_state.h"

namespace pnvo {
namespace {

// (TileArgs, KC, LDA and the loader of the activation tile: pnvo_baseline_state.h — the update step's weight gradient reads the same way)
// Threads = 16 pixel groups x COUT / 4 channel groups; a thread owns pixels tm + 16 i (i < TM) x 4 channels.
template <int SRC, int NRGB, int CIN, int KH, int KW, int S, int COUT, int TM, bool RELU>
__global__ __launch_bounds__(4 * COUT) void conv_tile_kernel(TileArgs a) {
  constexpr int BM = 16 * TM, TNG = COUT / 4, NT = 16 * TNG, K = KH * KW * CIN;
  static_assert(K % KC == 0 && (SRC != 0 || CIN % 4 == 0), "a chunk never straddles the end of K (nor a float4 a tap, for activations)");
  __shared__ __attribute__((aligned(16))) float As[BM * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[KC * COUT];
  __shared__ unsigned pix[BM];                   // (b * H + oy * S) * W + ox * S of the tile's pixels (past the end: the last pixel again)
  const int tid = threadIdx.x, tn = tid % TNG, tm = tid / TNG;
  const int m0 = blockIdx.x * BM;
  tile_pixels<S>(a, m0, BM, tid, NT, pix);
  float acc[TM][4];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int k0 = 0; k0 < K; k0 += KC) {
    __syncthreads();                             // the previous chunk has been read (first pass: pix is written)
    tile_load_a<SRC, NRGB, CIN, KW>(a, pix, k0, BM, tid, NT, As);
    for (int g = tid; g < KC * COUT / 4; g += NT)
      reinterpret_cast<f32x4 *>(Bs)[g] = reinterpret_cast<const f32x4 *>(a.wt + (size_t)k0 * COUT)[g];
    __syncthreads();
#pragma unroll 2
    for (int kk = 0; kk < KC; kk += 4) {
      f32x4 av[TM];
#pragma unroll
      for (int i = 0; i < TM; ++i) av[i] = *reinterpret_cast<const f32x4 *>(&As[(tm + 16 * i) * LDA + kk]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f32x4 bv = *reinterpret_cast<const f32x4 *>(&Bs[(kk + e) * COUT + 4 * tn]);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(av[i][e], bv[j], acc[i][j]);
      }
    }
  }
  const f32x4 bias = *reinterpret_cast<const f32x4 *>(a.bias + 4 * tn);
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = m0 + tm + 16 * i;
    if (m >= a.M) continue;
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = acc[i][j] + bias[j];
      if (RELU) v[j] = fmaxf(v[j], 0.f);
    }
    *reinterpret_cast<f32x4 *>(a.out + (size_t)m * COUT + 4 * tn) = v;
  }
}

// The tile by the number of output pixels: the largest of 64 / 32 / 16 pixels that still gives two to four workgroups per CU (the
// larger the tile, the more FMAs per LDS read; at the nav loop's batch sizes the step is latency-bound and the small tiles spread the
// few thousand pixels of a map over the chip).  A 128-pixel tile was measured slower at every size: two waves per workgroup and 43 KB
// of LDS leave a CU six waves.  Every tile gives the same bits.
template <int SRC, int NRGB, int CIN, int KH, int KW, int S, int COUT, bool RELU>
hipError_t launch_conv(const TileArgs &a, hipStream_t s) {
  const dim3 nt(4 * COUT);
  if (a.M >= 64 * 1024)
    hipLaunchKernelGGL((conv_tile_kernel<SRC, NRGB, CIN, KH, KW, S, COUT, 4, RELU>), dim3((unsigned)((a.M + 63) / 64)), nt, 0, s, a);
  else if (a.M >= 32 * 512)
    hipLaunchKernelGGL((conv_tile_kernel<SRC, NRGB, CIN, KH, KW, S, COUT, 2, RELU>), dim3((unsigned)((a.M + 31) / 32)), nt, 0, s, a);
  else
    hipLaunchKernelGGL((conv_tile_kernel<SRC, NRGB, CIN, KH, KW, S, COUT, 1, RELU>), dim3((unsigned)((a.M + 15) / 16)), nt, 0, s, a);
  return hipGetLastError();
}

// ---- the Linear: part[ks][b][n] = sum over slice ks of x[b][k] * w[n][k]   (x [B,F] = conv3's NHWC map, w [hidden,F] column-permuted)
// v_mfma_f32_16x16x4_f32: A[i][k] comes from lane (i = lane % 16, k = lane / 16), B[k][j] from lane (k = lane / 16, j = lane % 16),
// D[i][j] sits in lane (j = lane % 16), register r with i = 4 * (lane / 16) + r.  Here i = hidden unit, j = batch row; a lane loads
// four consecutive k of its row as one float4 and feeds them to four MFMAs, so the four lane groups cover 16 consecutive k per step
// (which k an MFMA sees is the same for both operands: the sum over the step is complete).  Rows past the end load the last row again
// and are never stored.
constexpr int FC_STEPS_PER_WG = 48;      // 16-float steps per workgroup: F = 24 960 -> 33 slices x 32 unit blocks = 1056 workgroups
constexpr int FC_ROWS = 32;              // batch rows per workgroup (two MFMA tiles sharing the weight registers)

__global__ __launch_bounds__(256) void fc_splitk_kernel(const float *x, const float *w, int B, int F, int hidden, int steps, float *part) {
  __shared__ f32x4 red[4][2][64];
  const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6);
  const int n0 = blockIdx.x * 16, ks = blockIdx.y, b0 = blockIdx.z * FC_ROWS;
  const int s0 = ks * FC_STEPS_PER_WG, s1 = min(steps, s0 + FC_STEPS_PER_WG);
  const int kl = 4 * (lane >> 4);
  const float *wr = w + (size_t)min(n0 + (lane & 15), hidden - 1) * F + kl;
  const float *x0 = x + (size_t)min(b0 + (lane & 15), B - 1) * F + kl;
  const float *x1 = x + (size_t)min(b0 + 16 + (lane & 15), B - 1) * F + kl;
  const bool two = b0 + 16 < B;            // (uniform over the workgroup)
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  if (two) {
    for (int s = s0 + wave; s < s1; s += 4) {
      const f32x4 wv = *reinterpret_cast<const f32x4 *>(wr + 16 * s);
      const f32x4 v0 = *reinterpret_cast<const f32x4 *>(x0 + 16 * s), v1 = *reinterpret_cast<const f32x4 *>(x1 + 16 * s);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[e], v0[e], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[e], v1[e], acc1, 0, 0, 0);
      }
    }
  } else {
    for (int s = s0 + wave; s < s1; s += 4) {
      const f32x4 wv = *reinterpret_cast<const f32x4 *>(wr + 16 * s);
      const f32x4 v0 = *reinterpret_cast<const f32x4 *>(x0 + 16 * s);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[e], v0[e], acc0, 0, 0, 0);
    }
  }
  red[wave][0][lane] = acc0;
  red[wave][1][lane] = acc1;
  __syncthreads();
  if (threadIdx.x >= 128) return;
  const int t = (int)(threadIdx.x >> 6);                       // MFMA tile of the thread: batch rows b0 + 16 t ..
  const f32x4 sum = ((red[0][t][lane] + red[1][t][lane]) + red[2][t][lane]) + red[3][t][lane];
  const int b = b0 + 16 * t + (lane & 15);
  if (b >= B) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = n0 + kl + r;
    if (n < hidden) part[((size_t)ks * B + b) * hidden + n] = sum[r];
  }
}

// embed[b][n] = relu(bias[n] + part[0][b][n] + part[1][b][n] + ...), slices in ascending order; written to x [B, Kp] = [embed | goal |
// zeros] (the GRU's input row, Kp % 4 == 0) and to `embed` [B, hidden] when that is given; x may be NULL (pnvo_baseline_encode).
// A blind handle has E = 0 and nks = 0: the row is the goal alone.  Thread = one element of the row.
__global__ __launch_bounds__(256) void fc_sum_inputs_kernel(const float *part, int nks, const float *bias, const float *goal, int B, int E,
                                                           int goal_dim, int Kp, float *x, float *embed) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)B * Kp) return;
  const int b = (int)(e / Kp), k = (int)(e % Kp);
  float v = 0.f;
  if (k < E) {
    v = bias[k];
#pragma unroll 8
    for (int s = 0; s < nks; ++s) v += part[((size_t)s * B + b) * E + k];      // (loads in flight together, added in slice order)
    v = fmaxf(v, 0.f);
    if (embed) embed[(size_t)b * E + k] = v;
  } else if (k < E + goal_dim && goal) {
    v = goal[(size_t)b * goal_dim + (k - E)];
  }
  if (x) x[e] = v;
}

}  // namespace

}  // namespace pnvo

using namespace pnvo;

static int ensure_rows(Baseline &p, int B) {
  if (B <= p.cap) return PNVO_OK;
  const pnvo_baseline_config &c = p.cfg;
  if (!blind(c)) {
    PCHK(p.a1.alloc((size_t)B * p.oh[0] * p.ow[0] * 32));
    PCHK(p.a2.alloc((size_t)B * p.oh[1] * p.ow[1] * 64));
    PCHK(p.a3.alloc((size_t)B * p.F));
    PCHK(p.part.alloc((size_t)p.nks * B * c.hidden));
  }
  PCHK(p.x.alloc((size_t)B * p.Kp));
  p.cap = B;
  return PNVO_OK;
}

namespace pnvo {

int baseline_frames_check(const Baseline &p, const char *fn, const void *rgb, int rgb_is_u8, const float *depth, int B) {
  const pnvo_baseline_config &c = p.cfg;
  if ((c.rgb_channels > 0) != (rgb != nullptr) || (c.depth_channels > 0) != (depth != nullptr))
    return pfail(PNVO_ERR_ARG, std::string(fn) + ": rgb / depth do not match the handle's visual types (rgb_channels " +
                                   std::to_string(c.rgb_channels) + ", depth_channels " + std::to_string(c.depth_channels) + ")");
  if ((rgb && !rgb_is_u8 && ((uintptr_t)rgb & 3)) || ((uintptr_t)depth & 3)) return pfail(PNVO_ERR_ARG, std::string(fn) + ": misaligned frames");
  if ((long long)B * c.height * c.width >= (1ll << 31)) return pfail(PNVO_ERR_ARG, std::string(fn) + ": batch too large (B * H * W must stay below 2^31)");
  return PNVO_OK;
}

// frames -> part (the Linear's partial tiles); the caller sums them (fc_sum_inputs_kernel)
int baseline_encoder_launches(const Baseline &p, const void *rgb, int rgb_is_u8, const float *depth, int B, float *o1, float *o2, float *o3,
                              float *part, hipStream_t s) {
  const pnvo_baseline_config &c = p.cfg;
  TileArgs a1{rgb, depth, nullptr, p.cw[0], p.cb[0], o1, B * p.oh[0] * p.ow[0], c.height, c.width, p.oh[0], p.ow[0]};
  if (c.rgb_channels && c.depth_channels)
    PCHK(rgb_is_u8 ? (launch_conv<2, 3, 4, 8, 8, 4, 32, true>(a1, s)) : (launch_conv<1, 3, 4, 8, 8, 4, 32, true>(a1, s)));
  else if (c.rgb_channels)
    PCHK(rgb_is_u8 ? (launch_conv<2, 3, 3, 8, 8, 4, 32, true>(a1, s)) : (launch_conv<1, 3, 3, 8, 8, 4, 32, true>(a1, s)));
  else
    PCHK((launch_conv<1, 0, 1, 8, 8, 4, 32, true>(a1, s)));
  TileArgs a2{nullptr, nullptr, o1, p.cw[1], p.cb[1], o2, B * p.oh[1] * p.ow[1], p.oh[0], p.ow[0], p.oh[1], p.ow[1]};
  PCHK((launch_conv<0, 0, 32, 4, 4, 2, 64, true>(a2, s)));
  TileArgs a3{nullptr, nullptr, o2, p.cw[2], p.cb[2], o3, B * p.oh[2] * p.ow[2], p.oh[1], p.ow[1], p.oh[2], p.ow[2]};
  PCHK((launch_conv<0, 0, 64, 3, 3, 1, 32, false>(a3, s)));
  hipLaunchKernelGGL(fc_splitk_kernel, dim3((unsigned)((c.hidden + 15) / 16), (unsigned)p.nks, (unsigned)((B + FC_ROWS - 1) / FC_ROWS)), dim3(256),
                     0, s, o3, p.fcw, B, p.F, c.hidden, p.F / 16, part);
  PCHK(hipGetLastError());
  return PNVO_OK;
}

hipError_t baseline_sum_inputs(const Baseline &p, const float *part, const float *goal, int B, float *x, float *embed, hipStream_t s) {
  const int Kp = x ? p.Kp : p.E;                 // (encode: one thread per element of the embedding)
  hipLaunchKernelGGL(fc_sum_inputs_kernel, dim3((unsigned)(((long)B * Kp + 255) / 256)), dim3(256), 0, s, part, p.nks, p.fcb, goal, B, p.E,
                     p.cfg.goal_dim, Kp, x, embed);
  return hipGetLastError();
}

}  // namespace pnvo

extern "C" {

int pnvo_baseline_create(const pnvo_baseline_config *cfg, int device, pnvo_baseline_handle *out) {
  if (!cfg || !out) return pfail(PNVO_ERR_ARG, "null argument");
  if ((cfg->rgb_channels != 0 && cfg->rgb_channels != 3) || (cfg->depth_channels != 0 && cfg->depth_channels != 1))
    return pfail(PNVO_ERR_ARG, "unsupported baseline policy visual input: rgb_channels " + std::to_string(cfg->rgb_channels) +
                                   " (0 or 3), depth_channels " + std::to_string(cfg->depth_channels) + " (0 or 1)");
  // 36 -> 8 -> 3 -> 1: the smallest frame that leaves conv3 an output pixel (simple_cnn.py:102-127)
  if (!blind(*cfg) && (cfg->width < 36 || cfg->height < 36))
    return pfail(PNVO_ERR_ARG, "unsupported baseline policy observation size " + std::to_string(cfg->width) + "x" + std::to_string(cfg->height) +
                                   " (width and height must be >= 36)");
  if (cfg->hidden <= 0 || cfg->hidden % 8 != 0)
    return pfail(PNVO_ERR_ARG, "unsupported baseline policy hidden_size " + std::to_string(cfg->hidden) + " (must be a positive multiple of 8)");
  if (cfg->n_actions < 1 || cfg->n_actions > 32)
    return pfail(PNVO_ERR_ARG, "unsupported baseline policy action_space.n " + std::to_string(cfg->n_actions) + " (1 to 32)");
  if (cfg->goal_dim < 1 || cfg->goal_dim > 8)
    return pfail(PNVO_ERR_ARG, "unsupported baseline policy goal size " + std::to_string(cfg->goal_dim) + " (1 to 8)");
  pnvo_baseline_s *h = new pnvo_baseline_s();
  Baseline &p = h->p;
  p.cfg = *cfg;
  p.device = device;
  p.C = cfg->rgb_channels + cfg->depth_channels;
  if (!blind(*cfg)) {
    const int k[3] = {8, 4, 3}, st[3] = {4, 2, 1};
    int hh = cfg->height, ww = cfg->width;
    for (int l = 0; l < 3; ++l) {
      hh = (hh - k[l]) / st[l] + 1, ww = (ww - k[l]) / st[l] + 1;      // floor: the remainder rows / columns are dropped
      p.oh[l] = hh, p.ow[l] = ww;
    }
    p.F = 32 * p.oh[2] * p.ow[2];
    p.E = cfg->hidden;
    p.nks = (p.F / 16 + FC_STEPS_PER_WG - 1) / FC_STEPS_PER_WG;
  }
  p.Kp = (p.E + cfg->goal_dim + 3) / 4 * 4;
  *out = h;
  return PNVO_OK;
}

int pnvo_baseline_load_weights(pnvo_baseline_handle h, const float *blob, size_t n_floats, const pnvo_tensor_desc *toc, int ntoc) {
  if (!h || !blob || !toc || ntoc < 0) return pfail(PNVO_ERR_ARG, "null argument");
  Baseline &p = h->p;
  const pnvo_baseline_config &c = p.cfg;
  if (p.attached)
    return pfail(PNVO_ERR_STATE, "pnvo_baseline_load_weights after pnvo_baseline_train_attach: the parameters live in the caller's flat buffer "
                                 "(write them there and call pnvo_baseline_train_refresh)");
  PCHK(hipSetDevice(p.device));
  int rc = PNVO_OK;
  // every tensor is found and checked before the first upload
  auto find = [&](const std::string &name, std::vector<int64_t> shape) -> const float * {
    PolicyParam e{name, std::move(shape), nullptr, false};
    const pnvo_tensor_desc *d = policy_find(toc, ntoc, e, n_floats, &rc);
    return d ? blob + d->offset : nullptr;
  };
  const int64_t Hd = c.hidden, A = c.n_actions, K = p.E + c.goal_dim;
  const std::string cnn = "net.visual_encoder.cnn.", rnn = "net.state_encoder.rnn.";
  const int64_t kk[3] = {8, 4, 3}, ci[3] = {p.C, 32, 64}, co[3] = {32, 64, 32};
  const float *cw[3] = {nullptr, nullptr, nullptr}, *cb[3] = {nullptr, nullptr, nullptr}, *fw = nullptr, *fb = nullptr;
  if (!blind(c)) {
    for (int l = 0; l < 3; ++l) {
      const std::string pre = cnn + std::to_string(2 * l);
      if (!(cw[l] = find(pre + ".weight", {co[l], ci[l], kk[l], kk[l]})) || !(cb[l] = find(pre + ".bias", {co[l]}))) return rc;
    }
    if (!(fw = find(cnn + "6.weight", {Hd, (int64_t)p.F})) || !(fb = find(cnn + "6.bias", {Hd}))) return rc;
  }
  const float *wih = find(rnn + "weight_ih_l0", {3 * Hd, K}), *whh = find(rnn + "weight_hh_l0", {3 * Hd, Hd});
  const float *bih = find(rnn + "bias_ih_l0", {3 * Hd}), *bhh = find(rnn + "bias_hh_l0", {3 * Hd});
  const float *aw = find("action_distribution.linear.weight", {A, Hd}), *ab = find("action_distribution.linear.bias", {A});
  const float *vw = find("critic.fc.weight", {1, Hd}), *vb = find("critic.fc.bias", {1});
  if (!wih || !whh || !bih || !bhh || !aw || !ab || !vw || !vb) return rc;
  // the tensors kept in torch's layout: one owned copy each, in a fixed order (a reload rewrites the same allocations in place)
  size_t n_own = 0;
  p.owned.resize(11);
  auto own = [&](const float **slot, const float *src, size_t n) -> int {
    DevBuf<float> &b = p.owned[n_own++];
    PCHK(b.upload(src, n));
    *slot = b;
    return PNVO_OK;
  };
  std::vector<float> t;
  if (!blind(c)) {
    for (int l = 0; l < 3; ++l) {                 // OIHW -> [ky][kx][c][o]
      const int64_t taps = kk[l] * kk[l];
      t.assign((size_t)(taps * ci[l] * co[l]), 0.f);
      for (int64_t o = 0; o < co[l]; ++o)
        for (int64_t ch = 0; ch < ci[l]; ++ch)
          for (int64_t tp = 0; tp < taps; ++tp) t[(size_t)((tp * ci[l] + ch) * co[l] + o)] = cw[l][(o * ci[l] + ch) * taps + tp];
      PCHK(p.cw[l].upload(t.data(), t.size()));
      if ((rc = own(&p.cb[l], cb[l], (size_t)co[l])) != PNVO_OK) return rc;
    }
    const int64_t P = p.oh[2] * p.ow[2];          // column c * P + pix (NCHW flatten) -> pix * 32 + c (the map conv3 writes)
    t.assign((size_t)(Hd * p.F), 0.f);
    for (int64_t n = 0; n < Hd; ++n)
      for (int64_t ch = 0; ch < 32; ++ch)
        for (int64_t px = 0; px < P; ++px) t[(size_t)(n * p.F + px * 32 + ch)] = fw[n * p.F + ch * P + px];
    PCHK(p.fcw.upload(t.data(), t.size()));
    if ((rc = own(&p.fcb, fb, (size_t)Hd)) != PNVO_OK) return rc;
  }
  t.assign((size_t)(3 * Hd * p.Kp), 0.f);         // [3 Hd][K] -> pitch Kp, zero columns behind the goal
  for (int64_t n = 0; n < 3 * Hd; ++n) std::memcpy(&t[(size_t)(n * p.Kp)], wih + n * K, sizeof(float) * (size_t)K);
  PCHK(p.w_ih.upload(t.data(), t.size()));
  if ((rc = own(&p.w_hh, whh, (size_t)(3 * Hd * Hd))) != PNVO_OK || (rc = own(&p.b_ih, bih, (size_t)(3 * Hd))) != PNVO_OK ||
      (rc = own(&p.b_hh, bhh, (size_t)(3 * Hd))) != PNVO_OK || (rc = own(&p.act_w, aw, (size_t)(A * Hd))) != PNVO_OK ||
      (rc = own(&p.act_b, ab, (size_t)A)) != PNVO_OK || (rc = own(&p.cr_w, vw, (size_t)Hd)) != PNVO_OK || (rc = own(&p.cr_b, vb, 1)) != PNVO_OK)
    return rc;
  p.loaded = true;
  return PNVO_OK;
}

int pnvo_baseline_encode(pnvo_baseline_handle h, const void *rgb, int rgb_is_u8, const float *depth, int B, float *embed, void *stream) {
  if (!h) return pfail(PNVO_ERR_ARG, "null handle");
  Baseline &p = h->p;
  if (blind(p.cfg)) return pfail(PNVO_ERR_STATE, "pnvo_baseline_encode: a blind policy has no visual encoder");
  if (!p.loaded) return pfail(PNVO_ERR_STATE, "pnvo_baseline_encode before pnvo_baseline_load_weights");
  if (B <= 0 || !embed) return pfail(PNVO_ERR_ARG, "null argument / bad batch");
  int rc = baseline_frames_check(p, "pnvo_baseline_encode", rgb, rgb_is_u8, depth, B);
  if (rc != PNVO_OK) return rc;
  PCHK(hipSetDevice(p.device));
  if ((rc = ensure_rows(p, B)) != PNVO_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = baseline_encoder_launches(p, rgb, rgb_is_u8, depth, B, p.a1, p.a2, p.a3, p.part, s)) != PNVO_OK) return rc;
  PCHK(baseline_sum_inputs(p, p.part, nullptr, B, nullptr, embed, s));
  return PNVO_OK;
}

int pnvo_baseline_act(pnvo_baseline_handle h, const void *rgb, int rgb_is_u8, const float *depth, const float *goal, const float *masks,
                      const float *hidden_in, int B, float *hidden_out, float *features, float *logits, float *value, void *stream) {
  if (!h) return pfail(PNVO_ERR_ARG, "null handle");
  Baseline &p = h->p;
  const pnvo_baseline_config &c = p.cfg;
  if (!p.loaded) return pfail(PNVO_ERR_STATE, "pnvo_baseline_act before pnvo_baseline_load_weights");
  if (B <= 0 || !goal || !masks || !hidden_in || !hidden_out) return pfail(PNVO_ERR_ARG, "null argument / bad batch");
  int rc = baseline_frames_check(p, "pnvo_baseline_act", rgb, rgb_is_u8, depth, B);
  if (rc != PNVO_OK) return rc;
  if (((uintptr_t)hidden_in & 15) || ((uintptr_t)hidden_out & 15))
    return pfail(PNVO_ERR_ARG, "pnvo_baseline_act: hidden_in / hidden_out must be 16-byte aligned");
  if (hidden_states_overlap(hidden_in, hidden_out, (size_t)B * c.hidden))
    return pfail(PNVO_ERR_ARG, "pnvo_baseline_act: hidden_in and hidden_out overlap (the GRU kernel writes the new state while other "
                               "workgroups still read the old one)");
  PCHK(hipSetDevice(p.device));
  if ((rc = ensure_rows(p, B)) != PNVO_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (!blind(c) && (rc = baseline_encoder_launches(p, rgb, rgb_is_u8, depth, B, p.a1, p.a2, p.a3, p.part, s)) != PNVO_OK) return rc;
  PCHK(baseline_sum_inputs(p, p.part, goal, B, p.x, nullptr, s));
  PCHK(launch_gru_layer(p.x, p.Kp, p.w_ih, p.b_ih, hidden_in, p.w_hh, p.b_hh, masks, B, c.hidden, hidden_out, s));
  if (features) PCHK(hipMemcpyAsync(features, hidden_out, (size_t)B * c.hidden * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (logits || value) PCHK(launch_policy_heads(hidden_out, p.act_w, p.act_b, p.cr_w, p.cr_b, B, c.hidden, c.n_actions, logits, value, s));
  return PNVO_OK;
}

int pnvo_baseline_destroy(pnvo_baseline_handle h) {
  if (!h) return PNVO_OK;
  (void)hipSetDevice(h->p.device);
  pnvo_baseline_train_free(h->p);
  delete h;
  return PNVO_OK;
}

}  // extern "C"
