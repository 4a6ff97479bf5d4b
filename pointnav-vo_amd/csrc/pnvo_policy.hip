// pnvo_policy.hip — the navigation policy's per-step forward, gfx950 only.
//
// PointNavResNetPolicy.act (reference: pointnav_vo/rl/policies/policy.py:29-46, resnet_policy.py:26-58,177-282):
//   depth [B,H,W,1] -> avg_pool2d(2) -> GroupNorm-ResNet18 (baseplanes 32) -> compression conv + GN(1) + ReLU
//   -> Flatten + Linear + ReLU (visual_fc)                              | the VO path's kernels, via a pnvo handle
//   x = [visual (hidden) | tgt_embeding([rho, cos(-phi), sin(-phi)]) (32) | prev_action_embedding (32)]
//   -> 2-layer LSTM, or GRU (cfg.rnn_type), with the hidden state masked at episode starts (model_utils/rnns/rnn_state_encoder.py:63-79)
//   -> action logits (CategoricalNet, utils/misc_utils.py:67-78) and value (CriticHead, policy.py:66-74).
// The visual encoder is the SAME kernel set as the VO model: a pnvo handle configured with (W/2, H/2), one depth
// modality of 2 channels [pooled depth | 0] and no whitening (normalize_visual_inputs is False for the depth-only policy,
// ddppo_trainer.py:118-121).  The recurrent part is tiny and weight-bandwidth-bound at B = number of environments
// (9.4 MB of LSTM weights per step), so its Linears are wave-per-output-row dot products on the vector ALU, not MFMA.
// Policies whose visual types name rgb, or that normalise their input (pnvo_policy_config.rgb_channels / no_depth / normalize), enter
// through pnvo_policy_act_rgbd / pnvo_policy_encode_rgbd: policy_input_kernel (rgb / 255, torch.cat([rgb, depth]), the pool, the zero
// channels and — in training mode — the batch moments of RunningMeanAndVar in ONE pass over the frames) in front of a handle configured
// with one float modality of 2C channels on the float32 stem, whose whitening pair policy_whiten_kernel writes from the module's buffers.
// pnvo_policy_encode is net.visual_encoder called on its own (the encoder handle stopped behind the compression conv, then
// feature_pack_kernel -> [B, C, fh, fw]); pnvo_policy_act_features is the step fed with that tensor (vfc_rows_kernel / the GEMM of
// policy_train.hip in place of the encoder).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pnvo.h"
#include "pnvo_internal.h"
#include "pnvo_model.h"
#include "pnvo_policy_state.h"

namespace pnvo {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// F.avg_pool2d(x, 2) of a 1-channel NHWC frame (floor: odd trailing row / column dropped) -> [N,H/2,W/2,2] with
// channel 1 = 0 (the encoder's stem consumes 2-channel pieces).
__global__ __launch_bounds__(256) void avgpool2_kernel(const float *d, int N, int H, int W, float *out) {
  const int Ho = H / 2, Wo = W / 2;
  const long total = (long)N * Ho * Wo;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int x = (int)(e % Wo);
  const int y = (int)((e / Wo) % Ho);
  const long n = e / ((long)Wo * Ho);
  const float *p = d + (n * H + 2 * y) * W + 2 * x;
  const float s = ((p[0] + p[1]) + p[W]) + p[W + 1];
  out[2 * e] = s * 0.25f;
  out[2 * e + 1] = 0.f;
}

// ---------------------------------------------------------------------------------------------------------------- the input stage
// ResNetEncoder.forward up to the backbone (resnet_policy.py:150-170) for the rgb / rgb-d / normalised handles, in one pass over the
// frames: rgb / 255, torch.cat([rgb, depth]), F.avg_pool2d(x, 2) (floor: an odd trailing row / column is dropped) -> [N,H/2,W/2,2C],
// channels [rgb, depth | C zeros]: ONE float modality of the encoder handle, whose reference order (first halves, then second halves)
// is then the reference's channel order followed by zero-weight channels.  With `train` the launch also leaves, per workgroup, the
// sums of (x - center) and (x - center)^2 per channel over its pooled pixels — the power-3 quantities of pnvo_input_moments that
// pnvo_rmv_merge consumes — so RunningMeanAndVar's update (running_mean_and_var.py:24-42) costs no second pass over the frames.
//
// Bandwidth-bound: a thread owns FOUR consecutive pooled pixels of a row, i.e. two input rows of 8 pixels — 24 bytes of uint8 rgb per
// row, fetched as the 6 or 7 aligned dwords that cover them and shifted into place (a row starts at any byte: W * 3 need not be a
// multiple of 4), or 24 floats of float32 rgb / 8 floats of depth, fetched as the aligned 16-byte chunks that cover them and selected
// by the start's offset.  An aligned chunk is only loaded when it holds at least one element the thread needs, so every load stays
// inside the 16-byte block of a valid element.  uint8 converts to float exactly: both kinds of rgb give the same bits.
// Sums: per thread in pixel order, a fixed xor tree over the wave, the four waves in order -> part[row][workgroup] (doubles); no atomics.
template <int NF>
__device__ __forceinline__ void load_row(const float *p, int nvalid, float (&out)[NF]) {
  constexpr int NC = (NF + 3 + 3) / 4;
  const uintptr_t a = (uintptr_t)p;
  const unsigned m = (unsigned)(a >> 2) & 3u;
  const f32x4 *q = reinterpret_cast<const f32x4 *>(a - 4 * m);
  const float *end = p + nvalid;
  float t[NC * 4];
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const f32x4 c = reinterpret_cast<const float *>(q + i) < end ? q[i] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) t[4 * i + e] = c[e];
  }
#pragma unroll
  for (int j = 0; j < NF; ++j) out[j] = m == 0 ? t[j] : (m == 1 ? t[j + 1] : (m == 2 ? t[j + 2] : t[j + 3]));
}
template <int NF>
__device__ __forceinline__ void load_row(const unsigned char *p, int nvalid, float (&out)[NF]) {
  static_assert(NF % 4 == 0, "whole dwords");
  constexpr int NW = NF / 4 + 1;
  const uintptr_t a = (uintptr_t)p;
  const unsigned m = (unsigned)a & 3u;
  const unsigned *q = reinterpret_cast<const unsigned *>(a - m);
  const unsigned char *end = p + nvalid;
  unsigned w[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) w[i] = reinterpret_cast<const unsigned char *>(q + i) < end ? q[i] : 0u;
#pragma unroll
  for (int i = 0; i < NF / 4; ++i) {
    const unsigned v = (unsigned)(((((unsigned long long)w[i + 1]) << 32) | (unsigned long long)w[i]) >> (8 * m));
#pragma unroll
    for (int e = 0; e < 4; ++e) out[4 * i + e] = (float)((v >> (8 * e)) & 0xffu);
  }
}

constexpr int INPUT_MAX_BLOCKS = 2048;      // workgroups of a launch = rows of `part` per moment

template <int CR, bool HAS_D, typename RGB_T>
__global__ __launch_bounds__(256) void policy_input_kernel(const RGB_T *rgb, const float *depth, int N, int H, int W, const float *center,
                                                         int train, float *out, double *part) {
  constexpr int C = CR + (HAS_D ? 1 : 0), C2 = 2 * C;
  const int Ho = H / 2, Wo = W / 2, Gw = (Wo + 3) / 4;
  const long groups = (long)N * Ho * Gw;
  float ctr[C];
  double s1[C], s2[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    ctr[c] = (train && center != nullptr) ? center[c] : 0.f;
    s1[c] = 0.0;
    s2[c] = 0.0;
  }
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
    const int xq = (int)(g % Gw);
    const int y = (int)((g / Gw) % Ho);
    const long n = g / ((long)Gw * Ho);
    const int npx = min(4, Wo - 4 * xq);
    float v[4][C];
    if constexpr (CR > 0) {
      float r0[8 * CR], r1[8 * CR];
      const RGB_T *p0 = rgb + ((n * H + 2 * y) * W + 8 * xq) * CR;
      load_row(p0, 2 * CR * npx, r0);
      load_row(p0 + (long)W * CR, 2 * CR * npx, r1);
#pragma unroll
      for (int px = 0; px < 4; ++px)
#pragma unroll
        for (int c = 0; c < CR; ++c)
          v[px][c] = (((r0[2 * CR * px + c] / 255.0f + r0[2 * CR * px + CR + c] / 255.0f) + r1[2 * CR * px + c] / 255.0f) +
                      r1[2 * CR * px + CR + c] / 255.0f) * 0.25f;
    }
    if constexpr (HAS_D) {
      float d0[8], d1[8];
      const float *p0 = depth + (n * H + 2 * y) * W + 8 * xq;
      load_row(p0, 2 * npx, d0);
      load_row(p0 + W, 2 * npx, d1);
#pragma unroll
      for (int px = 0; px < 4; ++px) v[px][CR] = (((d0[2 * px] + d0[2 * px + 1]) + d1[2 * px]) + d1[2 * px + 1]) * 0.25f;
    }
    float *o = out + ((n * Ho + y) * Wo + 4 * xq) * C2;
#pragma unroll
    for (int px = 0; px < 4; ++px) {
      if (px >= npx) break;
      float e[C2];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        e[c] = v[px][c];
        e[C + c] = 0.f;
      }
      if constexpr (C2 % 4 == 0) {                         // a pixel is 32 bytes: 16-byte stores
#pragma unroll
        for (int k = 0; k < C2; k += 4) *reinterpret_cast<f32x4 *>(o + px * C2 + k) = f32x4{e[k], e[k + 1], e[k + 2], e[k + 3]};
      } else {                                             // 8 or 24 bytes: 8-byte stores
#pragma unroll
        for (int k = 0; k < C2; k += 2) *reinterpret_cast<f32x2 *>(o + px * C2 + k) = f32x2{e[k], e[k + 1]};
      }
      if (train) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const double d = (double)(v[px][c] - ctr[c]);
          s1[c] += d;
          s2[c] += d * d;
        }
      }
    }
  }
  if (!train) return;                                      // (uniform)
  __shared__ double red[2 * C][4];
  const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int k = 0; k < 2 * C; ++k) {
    double s = k < C ? s1[k % C] : s2[k % C];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) red[k][wave] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * C)
    part[(long)threadIdx.x * gridDim.x + blockIdx.x] = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
}

// The moments from the pooled tensor [npix, 2C] instead (the two-launch form pnvo_policy_input_stage mode 2 measures the fused one
// against): thread = pixels npix-strided, the same partial layout.
template <int C>
__global__ __launch_bounds__(256) void pooled_moments_kernel(const float *pooled, long npix, const float *center, double *part) {
  float ctr[C];
  double s1[C], s2[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    ctr[c] = center != nullptr ? center[c] : 0.f;
    s1[c] = 0.0;
    s2[c] = 0.0;
  }
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < npix; e += (long)gridDim.x * 256) {
    float x[C];
    if constexpr (C % 2 == 0) {
#pragma unroll
      for (int c = 0; c < C; c += 2) {
        const f32x2 t = *reinterpret_cast<const f32x2 *>(pooled + e * 2 * C + c);
        x[c] = t[0];
        x[c + 1] = t[1];
      }
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) x[c] = pooled[e * 2 * C + c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const double d = (double)(x[c] - ctr[c]);
      s1[c] += d;
      s2[c] += d * d;
    }
  }
  __shared__ double red[2 * C][4];
  const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int k = 0; k < 2 * C; ++k) {
    double s = k < C ? s1[k % C] : s2[k % C];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) red[k][wave] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * C)
    part[(long)threadIdx.x * gridDim.x + blockIdx.x] = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
}

// one wave per row of `part` (channel c's first moment, then its second): the workgroups' sums in a fixed order -> m12[row] = sum / npix
// (float64: the first batches are centred on a running mean of zero, and e2 - e1^2 of a narrow channel does not survive float32)
__global__ __launch_bounds__(64) void input_moments_final_kernel(const double *part, int nb, double npix, double *m12) {
  const int row = blockIdx.x;
  double s = 0.0;
  for (int k = threadIdx.x; k < nb; k += 64) s += part[(long)row * nb + k];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  if (threadIdx.x == 0) m12[row] = s / npix;
}

// The data-parallel input stage (pnvo_policy_set_stats_hook).  input_moments_final_kernel with npix = 1 leaves the un-normalised sums
// in sums[0 .. 2C); this launch adds the call's frame count behind them, so that ONE all-reduce carries both ...
__global__ __launch_bounds__(64) void stats_count_kernel(double frames, double *count) {
  if (threadIdx.x == 0) *count = frames;
}
// ... and this one turns the reduced sums into the batch moments m12[row] = sums[row] / (frames * pixels per frame), the division
// input_moments_final_kernel makes on one rank (the product of two integers is exact in float64: one rank gives the same bits).
__global__ __launch_bounds__(64) void stats_moments_kernel(const double *sums, int C, double frame_pix, double *m12) {
  const int row = threadIdx.x;
  if (row < 2 * C) m12[row] = sums[row] / (sums[2 * C] * frame_pix);
}

// RunningMeanAndVar's buffers [C] -> the encoder handle's 2C channels (mean 0 / variance 1 on the zero channels: what its train-mode
// forward takes) and the float32 stem's whitening pair (x - mean) / sqrt(max(var, 1e-2)) = x * sc + sh over its CPL channel slots
// (running_mean_and_var.py:62-63; the arithmetic of whiten_table_kernel).  The handle's one modality keeps its channels in place:
// stem channel c is reference channel c.
__global__ __launch_bounds__(64) void policy_whiten_kernel(const float *mean, const float *var, int C, int CPL, float *mean_pad, float *var_pad,
                                                         float *sc, float *sh) {
  const int c = threadIdx.x;
  if (c >= CPL) return;
  const float mu = c < C ? mean[c] : 0.f, vr = c < C ? var[c] : 1.f;
  float a = 0.f, b = 0.f;
  if (c < 2 * C) {
    mean_pad[c] = mu;
    var_pad[c] = vr;
    const double sd = sqrt(fmax((double)vr, 1e-2));
    a = (float)(1.0 / sd);
    b = (float)(-(double)mu / sd);
  }
  sc[c] = a;
  sh[c] = b;
}

// LSTM input x [B, hidden + 64]: visual | Linear(3 -> 32)(rho, cos(-phi), sin(-phi)) | Embedding((a + 1) * mask).  The update step
// (B = the T*N rows of a rollout) keeps the gathered embedding row (rows) and (rho, cos(-phi), sin(-phi)) (g3) per row for its backward;
// both are nullptr on the act path.
__global__ __launch_bounds__(256) void policy_inputs_kernel(const float *visual, const float *goal, const int64_t *prev,
                                                          const float *masks, const float *tgt_w, const float *tgt_b,
                                                          const float *emb, int n_emb, int B, int hidden, float *x, int *rows,
                                                          float *g3) {
  const int K = hidden + 64;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)B * K) return;
  const int b = (int)(e / K), k = (int)(e % K);
  float v;
  if (k < hidden) {
    v = visual[(long)b * hidden + k];
  } else if (k < hidden + 32) {
    const int j = k - hidden;
    const float rho = goal[2 * b], phi = goal[2 * b + 1];
    const float g0 = rho, g1 = cosf(-phi), g2 = sinf(-phi);
    v = __builtin_fmaf(tgt_w[3 * j + 2], g2, __builtin_fmaf(tgt_w[3 * j + 1], g1, tgt_w[3 * j] * g0)) + tgt_b[j];
    if (j == 0 && g3 != nullptr) {
      g3[3 * b] = g0;
      g3[3 * b + 1] = g1;
      g3[3 * b + 2] = g2;
    }
  } else {
    const int j = k - hidden - 32;
    long row = (long)(((float)prev[b] + 1.0f) * masks[b]);     // ((prev_actions.float() + 1) * masks).long()
    if (row < 0) row = 0;
    if (row >= n_emb) row = n_emb - 1;
    v = emb[row * 32 + j];
    if (j == 0 && rows != nullptr) rows[b] = (int)row;
  }
  x[e] = v;
}

// One LSTM layer in one launch (round 6; it was two linear_rows launches + lstm_cell): workgroup = hidden unit j, wave = gate (i, f, g, o),
// gate[b] = (h_prev[b] . W_hh[n] * mask[b] + b_hh[n]) + (x[b] . W_ih[n] + b_ih[n]) with n = gate * Hd + j — one wave per gate row, all rows b, W in torch's
// [N][K] layout, K % 4 == 0; torch.nn.LSTM gate order, c_prev masked like h_prev — then the cell for (b, j) by the first lanes.
__global__ __launch_bounds__(256) void lstm_layer_kernel(const float *x, int K, const float *w_ih, const float *b_ih, const float *h_prev,
                                                       const float *w_hh, const float *b_hh, const float *c_prev, const float *masks,
                                                       int B, int Hd, float *h_out, float *c_out) {
  __shared__ float sg[4][64];
  const int lane = threadIdx.x & 63, gate = (int)(threadIdx.x >> 6), j = blockIdx.x;
  const int n = gate * Hd + j;
  const f32x4 *wi = reinterpret_cast<const f32x4 *>(w_ih + (long)n * K), *wh = reinterpret_cast<const f32x4 *>(w_hh + (long)n * Hd);
  const int K4 = K >> 2, H4 = Hd >> 2;
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int nb = min(64, B - b0);
    for (int bb = 0; bb < nb; ++bb) {
      const int b = b0 + bb;
      const f32x4 *xr = reinterpret_cast<const f32x4 *>(x + (long)b * K), *hr = reinterpret_cast<const f32x4 *>(h_prev + (long)b * Hd);
      float s = 0.f, u = 0.f;
      for (int k = lane; k < K4; k += 64) {
        const f32x4 w = wi[k], v = xr[k];
        s = __builtin_fmaf(w[0], v[0], s);
        s = __builtin_fmaf(w[1], v[1], s);
        s = __builtin_fmaf(w[2], v[2], s);
        s = __builtin_fmaf(w[3], v[3], s);
      }
      for (int k = lane; k < H4; k += 64) {
        const f32x4 w = wh[k], v = hr[k];
        u = __builtin_fmaf(w[0], v[0], u);
        u = __builtin_fmaf(w[1], v[1], u);
        u = __builtin_fmaf(w[2], v[2], u);
        u = __builtin_fmaf(w[3], v[3], u);
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        s += __shfl_xor(s, o);
        u += __shfl_xor(u, o);
      }
      if (lane == 0) sg[gate][bb] = (u * masks[b] + b_hh[n]) + (s + b_ih[n]);
    }
    __syncthreads();
    if ((int)threadIdx.x < nb) {
      const int b = b0 + (int)threadIdx.x;
      const long e = (long)b * Hd + j;
      const float i_ = 1.f / (1.f + expf(-sg[0][threadIdx.x]));
      const float f_ = 1.f / (1.f + expf(-sg[1][threadIdx.x]));
      const float g_ = tanhf(sg[2][threadIdx.x]);
      const float o_ = 1.f / (1.f + expf(-sg[3][threadIdx.x]));
      const float c = f_ * (c_prev[e] * masks[b]) + i_ * g_;
      c_out[e] = c;
      h_out[e] = o_ * tanhf(c);
    }
    __syncthreads();
  }
}

// One GRU layer in one launch, in lstm_layer_kernel's shape: workgroup = hidden unit j, wave = gate (r, z, n; torch.nn.GRU's order),
// W in torch's [3H][K] layout.  With hm = h_prev * mask:
//   r = sigmoid((hm . W_hr + b_hr) + (x . W_ir + b_ir)),  z likewise,  q = hm . W_hn + b_hn,  n = tanh((x . W_in + b_in) + r * q),
//   h' = (1 - z) * n + z * hm.
// b_hn sits inside the product with r, so the n-wave keeps its input sum and its recurrent sum apart (sg[2] / sq) until r is known.
__global__ __launch_bounds__(192) void gru_layer_kernel(const float *x, int K, const float *w_ih, const float *b_ih, const float *h_prev,
                                                      const float *w_hh, const float *b_hh, const float *masks, int B, int Hd,
                                                      float *h_out) {
  __shared__ float sg[3][64], sq[64];
  const int lane = threadIdx.x & 63, gate = (int)(threadIdx.x >> 6), j = blockIdx.x;
  const int n = gate * Hd + j;
  const f32x4 *wi = reinterpret_cast<const f32x4 *>(w_ih + (long)n * K), *wh = reinterpret_cast<const f32x4 *>(w_hh + (long)n * Hd);
  const int K4 = K >> 2, H4 = Hd >> 2;
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int nb = min(64, B - b0);
    for (int bb = 0; bb < nb; ++bb) {
      const int b = b0 + bb;
      const f32x4 *xr = reinterpret_cast<const f32x4 *>(x + (long)b * K), *hr = reinterpret_cast<const f32x4 *>(h_prev + (long)b * Hd);
      float s = 0.f, u = 0.f;
      for (int k = lane; k < K4; k += 64) {
        const f32x4 w = wi[k], v = xr[k];
        s = __builtin_fmaf(w[0], v[0], s);
        s = __builtin_fmaf(w[1], v[1], s);
        s = __builtin_fmaf(w[2], v[2], s);
        s = __builtin_fmaf(w[3], v[3], s);
      }
      for (int k = lane; k < H4; k += 64) {
        const f32x4 w = wh[k], v = hr[k];
        u = __builtin_fmaf(w[0], v[0], u);
        u = __builtin_fmaf(w[1], v[1], u);
        u = __builtin_fmaf(w[2], v[2], u);
        u = __builtin_fmaf(w[3], v[3], u);
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        s += __shfl_xor(s, o);
        u += __shfl_xor(u, o);
      }
      if (lane == 0) {
        const float rec = u * masks[b] + b_hh[n], in = s + b_ih[n];
        if (gate == 2) {
          sg[2][bb] = in;
          sq[bb] = rec;
        } else {
          sg[gate][bb] = rec + in;
        }
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < nb) {
      const int b = b0 + (int)threadIdx.x;
      const long e = (long)b * Hd + j;
      const float r_ = 1.f / (1.f + expf(-sg[0][threadIdx.x]));
      const float z_ = 1.f / (1.f + expf(-sg[1][threadIdx.x]));
      const float n_ = tanhf(sg[2][threadIdx.x] + r_ * sq[threadIdx.x]);
      {                                                    // two rounded products and their sum, spelled out: gru_step_kernel of the
#pragma clang fp contract(off)                             // update step (policy_train.hip) forms h the same way, bit for bit
        h_out[e] = (1.f - z_) * n_ + z_ * (h_prev[e] * masks[b]);
      }
    }
    __syncthreads();
  }
}

// action logits and value in one launch: rows 0 .. n_actions - 1 of the actor, then the critic's single row (one wave per output row)
__global__ __launch_bounds__(256) void policy_heads_kernel(const float *x, const float *act_w, const float *act_b, const float *cr_w,
                                                         const float *cr_b, int B, int K, int n_actions, float *logits, float *value) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (n > n_actions) return;
  const bool critic = n == n_actions;
  if ((critic ? value : logits) == nullptr) return;
  const f32x4 *wr = reinterpret_cast<const f32x4 *>(critic ? cr_w : act_w + (long)n * K);
  const float bias = critic ? cr_b[0] : act_b[n];
  const int K4 = K >> 2;
  for (int b = 0; b < B; ++b) {
    const f32x4 *xr = reinterpret_cast<const f32x4 *>(x + (long)b * K);
    float s = 0.f;
    for (int k = lane; k < K4; k += 64) {
      const f32x4 w = wr[k], v = xr[k];
      s = __builtin_fmaf(w[0], v[0], s);
      s = __builtin_fmaf(w[1], v[1], s);
      s = __builtin_fmaf(w[2], v[2], s);
      s = __builtin_fmaf(w[3], v[3], s);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) {
      if (critic) value[b] = s + bias;
      else logits[(long)b * n_actions + n] = s + bias;
    }
  }
}

// The visual encoder's output as the reference hands it on (ResNetEncoder.forward, resnet_policy.py:157-175): the compression conv's raw
// NHWC map [B, P = fh * fw, cp] (channels padded to cp, a multiple of 32) with its per-sample GroupNorm(1, C) scale / shift [B, cp]
// -> relu(x * scale + shift) as [B, C, fh, fw], the padding channels dropped.  Thread = one element of the raw map.
__global__ __launch_bounds__(256) void feature_pack_kernel(const float *raw, const float *sc, const float *sh, int B, int P, int C, int cp,
                                                         float *out) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)B * P * cp) return;
  const int c = (int)(e % cp);
  if (c >= C) return;
  const long bp = e / cp;
  const int pix = (int)(bp % P);
  const long b = bp / P;
  out[(b * C + c) * P + pix] = fmaxf(__builtin_fmaf(raw[e], sc[b * cp + c], sh[b * cp + c]), 0.f);
}

// visual_fc from features for the batches of act (fc_rows.hip's shape): out[b][n] = relu(x[b] . W[n] + bias[n]), W in torch's [hidden][F]
// layout.  Workgroup = four hidden units x one chunk of up to four samples (blockIdx.y), wave = hidden unit: the chunk's feature rows are
// staged in LDS once, the wave streams its weight row once and keeps four sums.  F % 4 may be anything, so a row starts at any float:
// the lanes below `head` take the elements in front of the row's first 16-byte boundary, the body runs on aligned float4 loads, the
// lanes of the tail take what is left (< 4).  The features are read from LDS by index, whatever their alignment in memory.
// float32 FMA chains and a fixed lane tree: the same bits every time.
__global__ __launch_bounds__(256) void vfc_rows_kernel(const float *x, const float *w, const float *bias, int B, int F, int hidden, float *out) {
  extern __shared__ float xs[];                            // [nb][F]
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  const int b0 = blockIdx.y * 4, nb = min(4, B - b0);
  const float *xb = x + (long)b0 * F;
  for (int i = threadIdx.x; i < nb * F; i += 256) xs[i] = xb[i];
  __syncthreads();
  if (n >= hidden) return;
  const float *wp = w + (long)n * F;
  const int head = min(F, (int)((4 - (((uintptr_t)wp >> 2) & 3)) & 3));
  const int nv = (F - head) >> 2;
  const float *xu[4];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < 4; ++u) xu[u] = xs + min(u, nb - 1) * F;   // (past the chunk's end: the last sample again, result unused)
  if (lane < head) {
    const float w0 = wp[lane];
#pragma unroll
    for (int u = 0; u < 4; ++u) s[u] = w0 * xu[u][lane];
  }
  const f32x4 *wv = reinterpret_cast<const f32x4 *>(wp + head);
  for (int v = lane; v < nv; v += 64) {
    const f32x4 w4 = wv[v];
    const int k = head + 4 * v;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) s[u] = __builtin_fmaf(w4[e], xu[u][k + e], s[u]);
  }
  const int kt = head + 4 * nv + lane;
  if (kt < F) {
    const float w0 = wp[kt];
#pragma unroll
    for (int u = 0; u < 4; ++u) s[u] = __builtin_fmaf(w0, xu[u][kt], s[u]);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
    for (int u = 0; u < 4; ++u) s[u] += __shfl_xor(s[u], o);
  if (lane < nb) {
    const float sv = lane == 0 ? s[0] : (lane == 1 ? s[1] : (lane == 2 ? s[2] : s[3]));
    out[(long)(b0 + lane) * hidden + n] = fmaxf(sv + bias[n], 0.f);
  }
}

template <int CR, bool HAS_D>
hipError_t launch_policy_input_t(const void *rgb, int rgb_is_u8, const float *depth, int N, int H, int W, const float *center, int train,
                                 float *out, double *part, int nb, hipStream_t s) {
  if (rgb_is_u8)
    hipLaunchKernelGGL((policy_input_kernel<CR, HAS_D, unsigned char>), dim3((unsigned)nb), dim3(256), 0, s, (const unsigned char *)rgb, depth, N,
                       H, W, center, train, out, part);
  else
    hipLaunchKernelGGL((policy_input_kernel<CR, HAS_D, float>), dim3((unsigned)nb), dim3(256), 0, s, (const float *)rgb, depth, N, H, W, center,
                       train, out, part);
  return hipGetLastError();
}

// workgroups of the input stage for N frames: one thread per group of four pooled pixels, grid-strided above INPUT_MAX_BLOCKS
int input_blocks(const pnvo_policy_config &c, int N) {
  const long groups = (long)N * (c.height / 2) * ((c.width / 2 + 3) / 4);
  return (int)std::min<long>((groups + 255) / 256, INPUT_MAX_BLOCKS);
}

hipError_t launch_policy_input(const pnvo_policy_config &c, const void *rgb, int rgb_is_u8, const float *depth, int N, const float *center,
                               int train, float *out, double *part, hipStream_t s) {
  const int nb = input_blocks(c, N);
  if (c.rgb_channels == 3 && !c.no_depth) return launch_policy_input_t<3, true>(rgb, rgb_is_u8, depth, N, c.height, c.width, center, train, out, part, nb, s);
  if (c.rgb_channels == 3) return launch_policy_input_t<3, false>(rgb, rgb_is_u8, nullptr, N, c.height, c.width, center, train, out, part, nb, s);
  return launch_policy_input_t<0, true>(nullptr, 0, depth, N, c.height, c.width, center, train, out, part, nb, s);
}

hipError_t launch_pooled_moments(int C, const float *pooled, long npix, const float *center, double *part, int nb, hipStream_t s) {
  if (C == 4) hipLaunchKernelGGL((pooled_moments_kernel<4>), dim3((unsigned)nb), dim3(256), 0, s, pooled, npix, center, part);
  else if (C == 3) hipLaunchKernelGGL((pooled_moments_kernel<3>), dim3((unsigned)nb), dim3(256), 0, s, pooled, npix, center, part);
  else hipLaunchKernelGGL((pooled_moments_kernel<1>), dim3((unsigned)nb), dim3(256), 0, s, pooled, npix, center, part);
  return hipGetLastError();
}

int ensure_moments(Policy &p) {
  if (!p.in_part) PCHK(p.in_part.alloc((size_t)8 * INPUT_MAX_BLOCKS));
  if (!p.m12) PCHK(p.m12.alloc(8));
  return PNVO_OK;
}

int ensure_pooled(Policy &p, int B) {
  if (B <= p.cap_pooled) return PNVO_OK;
  p.pooled.reset();                                        // the old workspace goes first
  p.cap_pooled = 0;
  PCHK(p.pooled.alloc(policy_pooled_floats(p.cfg, B)));
  p.cap_pooled = B;
  return PNVO_OK;
}

}  // namespace

// gru_layer_kernel / policy_heads_kernel for the baseline policy's handle (simple_cnn.hip): the same launches policy_act_tail makes
hipError_t launch_gru_layer(const float *x, int K, const float *w_ih, const float *b_ih, const float *h_prev, const float *w_hh,
                            const float *b_hh, const float *masks, int B, int Hd, float *h_out, hipStream_t s) {
  hipLaunchKernelGGL(gru_layer_kernel, dim3((unsigned)Hd), dim3(192), 0, s, x, K, w_ih, b_ih, h_prev, w_hh, b_hh, masks, B, Hd, h_out);
  return hipGetLastError();
}

hipError_t launch_policy_heads(const float *feat, const float *act_w, const float *act_b, const float *cr_w, const float *cr_b, int B, int Hd,
                               int n_actions, float *logits, float *value, hipStream_t s) {
  hipLaunchKernelGGL(policy_heads_kernel, dim3((unsigned)((n_actions + 1 + 3) / 4)), dim3(256), 0, s, feat, act_w, act_b, cr_w, cr_b, B, Hd,
                     n_actions, logits, value);
  return hipGetLastError();
}

}  // namespace pnvo

using namespace pnvo;

void pnvo::policy_features_shape(const Policy &p, int64_t shape[3]) {
  shape[0] = p.enc->comp_c;
  shape[1] = p.enc->fh;
  shape[2] = p.enc->fw;
}

int pnvo::launch_visual_fc(const Policy &p, const float *feat, int rows, float *out, hipStream_t s) {
  const int F = (int)policy_feature_floats(p), Hd = p.cfg.hidden;
  if (rows > VFC_ROWS_MAX) {
    PCHK(launch_visual_fc_gemm(feat, p.vfc_w, p.vfc_b, rows, F, Hd, out, s));
    return PNVO_OK;
  }
  const size_t lds = (size_t)4 * F * sizeof(float);
  if (lds > 65536) return pfail(PNVO_ERR_ARG, "visual_fc row kernel: " + std::to_string(F) + " feature floats per sample do not fit its LDS stage");
  hipLaunchKernelGGL(vfc_rows_kernel, dim3((unsigned)((Hd + 3) / 4), (unsigned)((rows + 3) / 4)), dim3(256), lds, s, feat, p.vfc_w, p.vfc_b, rows,
                     F, Hd, out);
  PCHK(hipGetLastError());
  return PNVO_OK;
}

hipError_t pnvo::launch_policy_inputs(const Policy &p, const float *visual, const float *goal, const int64_t *prev, const float *masks,
                                      int rows, float *x, int *rows_out, float *g3, hipStream_t s) {
  const int Hd = p.cfg.hidden;
  hipLaunchKernelGGL(policy_inputs_kernel, dim3((unsigned)(((long)rows * (Hd + 64) + 255) / 256)), dim3(256), 0, s, visual, goal, prev,
                     masks, p.tgt_w, p.tgt_b, p.emb, p.cfg.n_actions + 1, rows, Hd, x, rows_out, g3);
  return hipGetLastError();
}

int pnvo::policy_obs_check(const Policy &p, const PolicyObs &o, const char *fn) {
  const pnvo_policy_config &c = p.cfg;
  const std::string f(fn);
  if ((c.rgb_channels > 0) != (o.rgb != nullptr))
    return pfail(PNVO_ERR_ARG, f + ": rgb " + (o.rgb ? "given to a policy without rgb among its visual types" : "missing"));
  if ((c.no_depth == 0) != (o.depth != nullptr))
    return pfail(PNVO_ERR_ARG, f + ": depth " + (o.depth ? "given to a policy without depth among its visual types" : "missing"));
  if (c.normalize ? (!o.mean || !o.var || !o.count) : (o.mean || o.var || o.count || o.training))
    return pfail(PNVO_ERR_ARG, f + (c.normalize ? ": the policy normalises its visual inputs: run_mean, run_var and run_count are required"
                                                : ": the policy does not normalise its visual inputs: no statistics, training = 0"));
  if ((o.rgb && !o.rgb_is_u8 && ((uintptr_t)o.rgb & 3)) || ((uintptr_t)o.depth & 3))
    return pfail(PNVO_ERR_ARG, f + ": float32 frames must be 4-byte aligned");
  return PNVO_OK;
}

int pnvo::policy_input_stage(Policy &p, const PolicyObs &o, int B, float *pooled, hipStream_t s) {
  const pnvo_policy_config &c = p.cfg;
  const int C = policy_channels(c);
  const bool train = c.normalize && o.training;
  int rc = PNVO_OK;
  if (train && (rc = ensure_moments(p)) != PNVO_OK) return rc;
  if (c.normalize && !p.mean_pad) {
    PCHK(p.mean_pad.alloc(8));
    PCHK(p.var_pad.alloc(8));
  }
  PCHK(launch_policy_input(c, o.rgb, o.rgb_is_u8, o.depth, B, o.mean, train ? 1 : 0, pooled, p.in_part, s));
  if (train && p.stats_hook) {
    // one round over the ranks: sums about the (rank-identical) running mean and the frame count, reduced in place by the caller's
    // hook on this stream; the moments and the merge then read the reduced values on the device
    double *S = p.stats_sums;
    hipLaunchKernelGGL(input_moments_final_kernel, dim3((unsigned)(2 * C)), dim3(64), 0, s, p.in_part, input_blocks(c, B), 1.0, S);
    hipLaunchKernelGGL(stats_count_kernel, dim3(1), dim3(64), 0, s, (double)B, S + 2 * C);
    PCHK(hipGetLastError());
    p.stats_hook(p.stats_user, S, 2 * C + 1, (void *)s);
    hipLaunchKernelGGL(stats_moments_kernel, dim3(1), dim3(64), 0, s, S, C, (double)(c.height / 2) * (c.width / 2), p.m12);
    PCHK(hipGetLastError());
    PCHK(launch_rmv_merge_dev(p.m12, C, S + 2 * C, o.mean, o.var, o.count, s));
  } else if (train) {
    const double npix = (double)B * (c.height / 2) * (c.width / 2);
    hipLaunchKernelGGL(input_moments_final_kernel, dim3((unsigned)(2 * C)), dim3(64), 0, s, p.in_part, input_blocks(c, B), npix, p.m12);
    PCHK(hipGetLastError());
    // RunningMeanAndVar.forward's training branch on the module's own buffers (running_mean_and_var.py:41-60): pnvo_rmv_merge's
    // kernel, fed the float64 moments
    PCHK(launch_rmv_merge(p.m12, C, B, o.mean, o.var, o.count, s));
  }
  if (c.normalize) {
    hipLaunchKernelGGL(policy_whiten_kernel, dim3(1), dim3(64), 0, s, o.mean, o.var, C, p.enc->CPL, p.mean_pad, p.var_pad, p.enc->stem_sc,
                       p.enc->stem_sh);
    PCHK(hipGetLastError());
  }
  return PNVO_OK;
}

const pnvo_tensor_desc *pnvo::policy_find(const pnvo_tensor_desc *toc, int ntoc, const PolicyParam &e, size_t n_floats, int *rc) {
  for (int k = 0; k < ntoc; ++k) {
    if (e.name != toc[k].name) continue;
    const pnvo_tensor_desc &d = toc[k];
    bool ok = d.ndim == (int)e.shape.size();
    for (int i = 0; ok && i < d.ndim; ++i) ok = d.shape[i] == e.shape[i];
    if (!ok || d.offset + numel(e.shape) > n_floats) {
      *rc = pfail(PNVO_ERR_WEIGHTS, "policy tensor '" + e.name + "' has the wrong shape");
      return nullptr;
    }
    return &d;
  }
  *rc = pfail(PNVO_ERR_WEIGHTS, "policy state_dict is missing tensor '" + e.name + "'");
  return nullptr;
}

int pnvo::policy_encoder_table(const Policy &p, const pnvo_tensor_desc *toc, int ntoc, size_t n_floats, std::vector<EncoderEntry> *out) {
  const std::string pre = "net.visual_encoder.";
  out->clear();
  for (int k = 0; k < ntoc; ++k) {
    const std::string nm = toc[k].name;
    if (toc[k].ndim < 0 || toc[k].ndim > 4) return pfail(PNVO_ERR_WEIGHTS, "tensor '" + nm + "' has a bad rank");
    const std::vector<int64_t> shape(toc[k].shape, toc[k].shape + toc[k].ndim);
    if (toc[k].offset + numel(shape) > n_floats) return pfail(PNVO_ERR_WEIGHTS, "tensor '" + nm + "' exceeds the buffer");
    if (nm == pre + "backbone.conv1.0.weight") {          // [C0,C,7,7] -> [C0,2C,7,7], the second half of the input channels = 0
      const int64_t C = policy_channels(p.cfg);
      if (shape != std::vector<int64_t>{p.cfg.baseplanes, C, 7, 7})
        return pfail(PNVO_ERR_WEIGHTS, "policy stem must take " + std::to_string(C) + " input channel" + (C == 1 ? " (depth)" : "s"));
      out->push_back({"visual_encoder.backbone.conv1.0.weight", {shape[0], 2 * C, 7, 7}, EncoderEntry::STEM, k});
    } else if (nm.compare(0, pre.size(), pre) == 0) {
      // (RunningMeanAndVar's buffers are no parameters: the handle's whitening pair is written from them on the device at every call)
      if (nm.compare(pre.size(), 21, "running_mean_and_var.") == 0) continue;
      out->push_back({"visual_encoder." + nm.substr(pre.size()), shape, EncoderEntry::VIEW, k});
    } else if (nm == "net.visual_fc.1.weight" || nm == "net.visual_fc.1.bias") {
      out->push_back({"visual_fc.2." + nm.substr(nm.rfind('.') + 1), shape, EncoderEntry::VIEW, k});
    }
  }
  out->push_back({"output_head.1.weight", {1, p.cfg.hidden}, EncoderEntry::ZEROS, -1});
  out->push_back({"output_head.1.bias", {1}, EncoderEntry::ZEROS, -1});
  return PNVO_OK;
}

std::vector<pnvo_tensor_desc> pnvo::encoder_toc(const std::vector<EncoderEntry> &entries, const std::vector<size_t> &offsets) {
  std::vector<pnvo_tensor_desc> toc(entries.size());
  for (size_t i = 0; i < entries.size(); ++i) {
    std::memset(&toc[i], 0, sizeof(toc[i]));
    toc[i].name = entries[i].name.c_str();
    toc[i].offset = offsets[i];
    toc[i].ndim = (int)entries[i].shape.size();
    for (size_t d = 0; d < entries[i].shape.size(); ++d) toc[i].shape[d] = entries[i].shape[d];
  }
  return toc;
}

// a handle with rgb / normalisation reached through an entry point that takes depth alone
static int refuse_plain_entry(const Policy &p, const char *fn) {
  if (policy_is_plain(p.cfg)) return PNVO_OK;
  return pfail(PNVO_ERR_STATE, std::string(fn) + ": this policy takes rgb and / or RunningMeanAndVar statistics (rgb_channels, no_depth, normalize): "
                                   "call " + fn + "_rgbd");
}

// p.pooled [B, ...] -> features_out [B,C,fh,fw] (NCHW): the encoder up to the compression block, channel padding dropped
static int policy_encode_pooled(Policy &p, int B, float *features_out, hipStream_t s) {
  const int rc = pnvo_forward_compression(p.enc, p.pooled, B, s);
  if (rc != PNVO_OK) return pfail(rc, std::string("policy visual encoder: ") + pnvo_last_error(p.enc));
  const pnvo_handle m = p.enc;
  const int P = m->fh * m->fw;
  const long total = (long)B * P * m->comp_cp;
  hipLaunchKernelGGL(feature_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, m->comp_raw, m->ssC[0], m->ssC[1], B, P,
                     m->comp_c, m->comp_cp, features_out);
  PCHK(hipGetLastError());
  return PNVO_OK;
}

// the shared body of pnvo_policy_act (depth given), pnvo_policy_act_rgbd (obs given) and pnvo_policy_act_features (vfeat given)
static int policy_act_impl(pnvo_policy_handle h, const char *fn, const float *depth, const PolicyObs *obs, const float *vfeat, const float *goal,
                           const int64_t *prev_actions, const float *masks, const float *hidden_in, int B, float *hidden_out, float *features,
                           float *logits, float *value, void *stream) {
  if (!h) return pfail(PNVO_ERR_ARG, "null handle");
  Policy &p = h->p;
  if (!p.loaded) return pfail(PNVO_ERR_STATE, std::string(fn) + " before pnvo_policy_load_weights");
  if (B <= 0 || (!depth && !obs && !vfeat) || !goal || !prev_actions || !masks || !hidden_in || !hidden_out)
    return pfail(PNVO_ERR_ARG, "null argument / bad batch");
  int rc = PNVO_OK;
  if (obs && (rc = policy_obs_check(p, *obs, fn)) != PNVO_OK) return rc;
  const pnvo_policy_config &c = p.cfg;
  const int Hd = c.hidden, K0 = Hd + 64;
  const bool gru = is_gru(c);
  if (hidden_states_overlap(hidden_in, hidden_out, rnn_state_floats(c, B)))
    return pfail(PNVO_ERR_ARG, std::string("hidden_out overlaps hidden_in (each holds ") + (gru ? "" : "2 * ") +
                                   "rnn_layers * B * hidden floats): pass separate buffers");
  PCHK(hipSetDevice(p.device));
  hipStream_t s = (hipStream_t)stream;
  if (B > p.cap) {
    for (DevBuf<float> *b : {&p.visual, &p.x}) b->reset();   // the old workspace goes first
    p.cap = 0;
    PCHK(p.visual.alloc((size_t)B * Hd));
    PCHK(p.x.alloc((size_t)B * K0));
    p.cap = B;
  }
  if (depth || obs) {
    if ((rc = ensure_pooled(p, B)) != PNVO_OK) return rc;
    if ((rc = obs ? policy_input_stage(p, *obs, B, p.pooled, s) : pnvo_avgpool2(depth, B, c.height, c.width, p.pooled, stream)) != PNVO_OK)
      return rc;
    if (p.attached && !policy_resnet18(c)) {
      // a frozen non-resnet18 encoder is not attached to the update step: its handle's copy of visual_fc went stale with the first
      // optimiser step.  The encoder's output goes through the policy's own visual_fc (the flat buffer), as on the visual_features path.
      if (B > p.cap_feat) {
        p.feat.reset();
        p.cap_feat = 0;
        PCHK(p.feat.alloc((size_t)B * policy_feature_floats(p)));
        p.cap_feat = B;
      }
      if ((rc = policy_encode_pooled(p, B, p.feat, s)) != PNVO_OK || (rc = launch_visual_fc(p, p.feat, B, p.visual, s)) != PNVO_OK) return rc;
    } else {
      rc = pnvo_forward_features(p.enc, nullptr, p.pooled, nullptr, nullptr, nullptr, B, p.visual, stream);
      if (rc != PNVO_OK) return pfail(rc, std::string("policy visual encoder: ") + pnvo_last_error(p.enc));
    }
  } else if ((rc = launch_visual_fc(p, vfeat, B, p.visual, s)) != PNVO_OK) {
    return rc;
  }
  PCHK(launch_policy_inputs(p, p.visual, goal, prev_actions, masks, B, p.x, nullptr, nullptr, s));
  return policy_act_tail(p, masks, hidden_in, B, hidden_out, features, logits, value, s);
}

int pnvo::policy_act_tail(Policy &p, const float *masks, const float *hidden_in, int B, float *hidden_out, float *features, float *logits,
                          float *value, hipStream_t s) {
  const pnvo_policy_config &c = p.cfg;
  const int Hd = c.hidden, L = c.rnn_layers, K0 = Hd + 64;
  const bool gru = is_gru(c);
  // hidden_in / hidden_out: LSTM [2L, B, Hd] = (h_0 .. h_{L-1}, c_0 .. c_{L-1}), GRU [L, B, Hd] = (h_0 .. h_{L-1})  (rnn_state_encoder.py:43-61)
  const float *xin = p.x;
  int K = K0;
  if (gru) {
    for (int l = 0; l < L; ++l) {
      float *h_new = hidden_out + (size_t)l * B * Hd;
      hipLaunchKernelGGL(gru_layer_kernel, dim3((unsigned)Hd), dim3(192), 0, s, xin, K, p.w_ih[l], p.b_ih[l], hidden_in + (size_t)l * B * Hd,
                         p.w_hh[l], p.b_hh[l], masks, B, Hd, h_new);
      xin = h_new;
      K = Hd;
    }
  } else {
    for (int l = 0; l < L; ++l) {
      const float *h_prev = hidden_in + (size_t)l * B * Hd, *c_prev = hidden_in + (size_t)(L + l) * B * Hd;
      float *h_new = hidden_out + (size_t)l * B * Hd, *c_new = hidden_out + (size_t)(L + l) * B * Hd;
      hipLaunchKernelGGL(lstm_layer_kernel, dim3((unsigned)Hd), dim3(256), 0, s, xin, K, p.w_ih[l], p.b_ih[l], h_prev, p.w_hh[l], p.b_hh[l],
                         c_prev, masks, B, Hd, h_new, c_new);
      xin = h_new;
      K = Hd;
    }
  }
  const float *feat = hidden_out + (size_t)(L - 1) * B * Hd;
  if (features) PCHK(hipMemcpyAsync(features, feat, (size_t)B * Hd * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (logits || value)
    hipLaunchKernelGGL(policy_heads_kernel, dim3((unsigned)((c.n_actions + 1 + 3) / 4)), dim3(256), 0, s, feat, p.act_w, p.act_b, p.cr_w,
                       p.cr_b, B, Hd, c.n_actions, logits, value);
  PCHK(hipGetLastError());
  return PNVO_OK;
}

extern "C" {

int pnvo_avgpool2(const float *depth, int N, int H, int W, float *out, void *stream) {
  if (!depth || !out || N < 0 || H < 2 || W < 2) return pfail(PNVO_ERR_ARG, "bad argument");
  if (N == 0) return PNVO_OK;
  const long total = (long)N * (H / 2) * (W / 2);
  hipLaunchKernelGGL(avgpool2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, depth, N, H, W,
                     out);
  PCHK(hipGetLastError());
  return PNVO_OK;
}

int pnvo_policy_create(const pnvo_policy_config *cfg, int device, pnvo_policy_handle *out) {
  if (!cfg || !out) return pfail(PNVO_ERR_ARG, "null argument");
  if (cfg->width < 64 || cfg->height < 64)
    return pfail(PNVO_ERR_ARG, "unsupported policy observation size " + std::to_string(cfg->width) + "x" + std::to_string(cfg->height) +
                                   " (width and height must be >= 64)");
  // the visual encoder's visual_fc takes hidden sizes in multiples of 8 (pnvo_create); the recurrent weights' rows are read as float4
  if (cfg->hidden <= 0 || cfg->hidden % 8 != 0)
    return pfail(PNVO_ERR_ARG, "unsupported policy hidden_size " + std::to_string(cfg->hidden) + " (must be a positive multiple of 8)");
  if (cfg->rnn_layers < 1 || cfg->rnn_layers > 4)
    return pfail(PNVO_ERR_ARG, "unsupported policy num_recurrent_layers " + std::to_string(cfg->rnn_layers) + " (1 to 4)");
  if (cfg->n_actions < 1 || cfg->n_actions > 32)
    return pfail(PNVO_ERR_ARG, "unsupported policy action_space.n " + std::to_string(cfg->n_actions) + " (1 to 32)");
  if (cfg->rnn_type != PNVO_RNN_LSTM && cfg->rnn_type != PNVO_RNN_GRU)
    return pfail(PNVO_ERR_ARG, "unsupported policy rnn_type " + std::to_string(cfg->rnn_type) + " (0 = LSTM, 1 = GRU)");
  // (read behind rnn_type: callers built against the eight-field struct are served or refused by the checks above)
  if ((cfg->rgb_channels != 0 && cfg->rgb_channels != 3) || (cfg->no_depth != 0 && cfg->no_depth != 1) ||
      (cfg->normalize != 0 && cfg->normalize != 1) || (cfg->no_depth && cfg->rgb_channels == 0))
    return pfail(PNVO_ERR_ARG, "unsupported policy visual input: rgb_channels " + std::to_string(cfg->rgb_channels) + " (0 or 3), no_depth " +
                                   std::to_string(cfg->no_depth) + " (0, or 1 with rgb), normalize " + std::to_string(cfg->normalize) + " (0 or 1)");
  // (read behind normalize: zero keeps resnet18; pnvo_create checks the combination)
  if (cfg->backbone_depth != 0 && cfg->backbone_depth != 18 && cfg->backbone_depth != 50 && cfg->backbone_depth != 101)
    return pfail(PNVO_ERR_ARG, "unsupported policy backbone_depth " + std::to_string(cfg->backbone_depth) + " (0 / 18, 50 or 101)");
  pnvo_policy_s *h = new pnvo_policy_s();
  h->p.cfg = *cfg;
  h->p.device = device;
  pnvo_config ec;
  std::memset(&ec, 0, sizeof(ec));
  ec.width = cfg->width / 2;             // after F.avg_pool2d(x, 2)  (resnet_policy.py:168)
  ec.height = cfg->height / 2;
  ec.n_depth = 2 * policy_channels(*cfg);   // [pooled depth | 0], or [rgb / 255, depth | zeros] / [rgb / 255 | zeros] (policy_input_kernel)
  ec.baseplanes = cfg->baseplanes;
  ec.hidden = cfg->hidden;
  ec.out_dim = 1;                        // unused head (the policy stops at the hidden vector)
  ec.normalize = cfg->normalize;         // the whitening rides on the stem's scale / shift pair (policy_whiten_kernel)
  ec.n_acts = 4;
  ec.flat_size = cfg->flat_size;
  ec.max_batch = 16;
  ec.backbone_depth = cfg->backbone_depth;
  ec.resnext = cfg->resnext;
  ec.se = cfg->se;
  int rc = pnvo_create(&ec, device, &h->p.enc);
  if (rc != PNVO_OK) {
    delete h;
    return rc;
  }
  if (!policy_is_plain(*cfg)) {
    // Pooled rgb is no integer 0..255 and the statistics move on the device: these handles run the float32 stem, which takes any
    // float input and reads its whitening pair from a device table, at every batch size on the per-layer kernels; the stem's weight
    // gradient stays on the float32 kernel that reads the same table.
    const char *opts[3][2] = {{"stem", "dense"}, {"small_net", "off"}, {"wgrad_stem", "fp32"}};
    for (auto &o : opts)
      if ((rc = pnvo_set_option(h->p.enc, o[0], o[1])) != PNVO_OK) {
        rc = pfail(rc, std::string("policy visual encoder: ") + pnvo_last_error(h->p.enc));
        pnvo_destroy(h->p.enc);
        delete h;
        return rc;
      }
  }
  for (auto *v : {&h->p.w_ih, &h->p.w_hh, &h->p.b_ih, &h->p.b_hh}) v->assign(cfg->rnn_layers, nullptr);   // policy_params()'s slots
  *out = h;
  return PNVO_OK;
}

int pnvo_policy_load_weights(pnvo_policy_handle h, const float *blob, size_t n_floats, const pnvo_tensor_desc *toc,
                             int ntoc) {
  if (!h || !blob || !toc) return pfail(PNVO_ERR_ARG, "null argument");
  Policy &p = h->p;
  if (p.attached)
    return pfail(PNVO_ERR_STATE, "pnvo_policy_load_weights after pnvo_policy_train_attach: the parameters live in the caller's flat buffer "
                                 "(write them there and call pnvo_policy_train_refresh)");
  PCHK(hipSetDevice(p.device));
  int rc = PNVO_OK;
  // ---- visual encoder + visual_fc: the encoder handle's table, materialised into a blob of its own
  {
    std::vector<EncoderEntry> ent;
    if ((rc = policy_encoder_table(p, toc, ntoc, n_floats, &ent)) != PNVO_OK) return rc;
    std::vector<float> eblob;
    std::vector<size_t> offs;
    for (const EncoderEntry &e : ent) {
      offs.push_back(eblob.size());
      const size_t cnt = numel(e.shape);
      if (e.src == EncoderEntry::VIEW) {
        eblob.insert(eblob.end(), blob + toc[e.k].offset, blob + toc[e.k].offset + cnt);
      } else {
        eblob.insert(eblob.end(), cnt, 0.f);
        if (e.src == EncoderEntry::STEM) {               // [C0,C,7,7] -> channels 0 .. C-1 of [C0,2C,7,7]
          const size_t row = (size_t)policy_channels(p.cfg) * 49;
          for (int64_t o = 0; o < e.shape[0]; ++o)
            std::memcpy(&eblob[offs.back() + (size_t)o * 2 * row], blob + toc[e.k].offset + o * row, sizeof(float) * row);
        }
      }
    }
    if (p.cfg.normalize) {
      // the handle wants its statistics at load: mean 0 / variance 1 over its 2C channels, stand-ins until the first call's
      // policy_whiten_kernel writes the whitening pair from the module's buffers
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
  }
  // ---- recurrent part and heads (kept in torch's layouts)
  const std::vector<PolicyParam> tab = policy_params(p);
  p.owned.resize(tab.size());
  for (size_t i = 0; i < tab.size(); ++i) {
    const pnvo_tensor_desc *d = policy_find(toc, ntoc, tab[i], n_floats, &rc);
    if (!d) return rc;
    PCHK(p.owned[i].alloc(numel(tab[i].shape)));
    PCHK(hipMemcpy(p.owned[i], blob + d->offset, numel(tab[i].shape) * sizeof(float), hipMemcpyHostToDevice));
    *tab[i].slot = p.owned[i];
  }
  p.loaded = true;
  return PNVO_OK;
}

int pnvo_policy_act(pnvo_policy_handle h, const float *depth, const float *goal, const int64_t *prev_actions,
                    const float *masks, const float *hidden_in, int B, float *hidden_out, float *features, float *logits,
                    float *value, void *stream) {
  if (!depth) return pfail(PNVO_ERR_ARG, "null argument / bad batch");
  if (h && refuse_plain_entry(h->p, "pnvo_policy_act") != PNVO_OK) return PNVO_ERR_STATE;
  return policy_act_impl(h, "pnvo_policy_act", depth, nullptr, nullptr, goal, prev_actions, masks, hidden_in, B, hidden_out, features, logits, value,
                         stream);
}

int pnvo_policy_act_features(pnvo_policy_handle h, const float *visual_features, const float *goal, const int64_t *prev_actions,
                             const float *masks, const float *hidden_in, int B, float *hidden_out, float *features, float *logits,
                             float *value, void *stream) {
  if (!visual_features) return pfail(PNVO_ERR_ARG, "null argument / bad batch");
  return policy_act_impl(h, "pnvo_policy_act_features", nullptr, nullptr, visual_features, goal, prev_actions, masks, hidden_in, B, hidden_out,
                         features, logits, value, stream);
}

int pnvo_policy_features_shape(pnvo_policy_handle h, int64_t shape[3]) {
  if (!h || !shape) return pfail(PNVO_ERR_ARG, "null argument");
  policy_features_shape(h->p, shape);
  return PNVO_OK;
}

static int policy_encode_impl(pnvo_policy_handle h, const char *fn, const float *depth, const PolicyObs *obs, int B, float *features_out,
                              void *stream) {
  if (!h) return pfail(PNVO_ERR_ARG, "null handle");
  Policy &p = h->p;
  if (!p.loaded) return pfail(PNVO_ERR_STATE, std::string(fn) + " before pnvo_policy_load_weights");
  if (B <= 0 || (!depth && !obs) || !features_out) return pfail(PNVO_ERR_ARG, "null argument / bad batch");
  int rc = PNVO_OK;
  if (obs && (rc = policy_obs_check(p, *obs, fn)) != PNVO_OK) return rc;
  const pnvo_policy_config &c = p.cfg;
  PCHK(hipSetDevice(p.device));
  if ((rc = ensure_pooled(p, B)) != PNVO_OK) return rc;
  if ((rc = obs ? policy_input_stage(p, *obs, B, p.pooled, (hipStream_t)stream) : pnvo_avgpool2(depth, B, c.height, c.width, p.pooled, stream)) !=
      PNVO_OK)
    return rc;
  return policy_encode_pooled(p, B, features_out, (hipStream_t)stream);
}

int pnvo_policy_encode(pnvo_policy_handle h, const float *depth, int B, float *features_out, void *stream) {
  if (h && refuse_plain_entry(h->p, "pnvo_policy_encode") != PNVO_OK) return PNVO_ERR_STATE;
  if (!depth) return pfail(PNVO_ERR_ARG, "null argument / bad batch");
  return policy_encode_impl(h, "pnvo_policy_encode", depth, nullptr, B, features_out, stream);
}

// rgb, the statistics and `training` of a *_rgbd call on a depth-only, un-normalised handle: nothing to take
static bool plain_rgbd_call(const void *rgb, const float *mean, const float *var, const float *count, int training) {
  return rgb == nullptr && mean == nullptr && var == nullptr && count == nullptr && training == 0;
}

int pnvo_policy_act_rgbd(pnvo_policy_handle h, const void *rgb, int rgb_is_u8, const float *depth, float *run_mean, float *run_var,
                         float *run_count, int training, const float *goal, const int64_t *prev_actions, const float *masks,
                         const float *hidden_in, int B, float *hidden_out, float *features, float *logits, float *value, void *stream) {
  if (!h) return pfail(PNVO_ERR_ARG, "null handle");
  if (policy_is_plain(h->p.cfg) && plain_rgbd_call(rgb, run_mean, run_var, run_count, training))
    return pnvo_policy_act(h, depth, goal, prev_actions, masks, hidden_in, B, hidden_out, features, logits, value, stream);
  PolicyObs o;
  o.rgb = rgb, o.rgb_is_u8 = rgb_is_u8, o.depth = depth, o.mean = run_mean, o.var = run_var, o.count = run_count, o.training = training;
  return policy_act_impl(h, "pnvo_policy_act_rgbd", nullptr, &o, nullptr, goal, prev_actions, masks, hidden_in, B, hidden_out, features, logits,
                         value, stream);
}

int pnvo_policy_encode_rgbd(pnvo_policy_handle h, const void *rgb, int rgb_is_u8, const float *depth, float *run_mean, float *run_var,
                            float *run_count, int training, int B, float *features_out, void *stream) {
  if (!h) return pfail(PNVO_ERR_ARG, "null handle");
  if (policy_is_plain(h->p.cfg) && plain_rgbd_call(rgb, run_mean, run_var, run_count, training))
    return pnvo_policy_encode(h, depth, B, features_out, stream);
  PolicyObs o;
  o.rgb = rgb, o.rgb_is_u8 = rgb_is_u8, o.depth = depth, o.mean = run_mean, o.var = run_var, o.count = run_count, o.training = training;
  return policy_encode_impl(h, "pnvo_policy_encode_rgbd", nullptr, &o, B, features_out, stream);
}

int pnvo_policy_input_stage(pnvo_policy_handle h, const void *rgb, int rgb_is_u8, const float *depth, const float *center, int mode, int B,
                            float *pooled_out, double *m12_out, void *stream) {
  if (!h) return pfail(PNVO_ERR_ARG, "null handle");
  Policy &p = h->p;
  const pnvo_policy_config &c = p.cfg;
  if (policy_is_plain(c)) return pfail(PNVO_ERR_STATE, "pnvo_policy_input_stage: the depth-only, un-normalised policy pools with pnvo_avgpool2");
  if (B <= 0 || mode < 0 || mode > 2 || !pooled_out || (mode && !m12_out) || ((uintptr_t)pooled_out & 15) || ((uintptr_t)m12_out & 7))
    return pfail(PNVO_ERR_ARG, "null argument / bad batch / bad mode / pooled_out not 16-byte aligned");
  PolicyObs o;
  o.rgb = rgb, o.rgb_is_u8 = rgb_is_u8, o.depth = depth;
  if ((c.rgb_channels > 0) != (rgb != nullptr) || (c.no_depth == 0) != (depth != nullptr) || (rgb && !rgb_is_u8 && ((uintptr_t)rgb & 3)) ||
      ((uintptr_t)depth & 3))
    return pfail(PNVO_ERR_ARG, "pnvo_policy_input_stage: frames do not match the policy's visual types");
  PCHK(hipSetDevice(p.device));
  hipStream_t s = (hipStream_t)stream;
  int rc = PNVO_OK;
  if (mode && (rc = ensure_moments(p)) != PNVO_OK) return rc;
  const int C = policy_channels(c), nb = input_blocks(c, B);
  const long npix = (long)B * (c.height / 2) * (c.width / 2);
  PCHK(launch_policy_input(c, rgb, rgb_is_u8, depth, B, center, mode == 1, pooled_out, p.in_part, s));
  if (mode == 2) PCHK(launch_pooled_moments(C, pooled_out, npix, center, p.in_part, nb, s));
  if (mode) {
    hipLaunchKernelGGL(input_moments_final_kernel, dim3((unsigned)(2 * C)), dim3(64), 0, s, p.in_part, nb, (double)npix, m12_out);
    PCHK(hipGetLastError());
  }
  return PNVO_OK;
}

int pnvo_policy_set_stats_hook(pnvo_policy_handle h, pnvo_stats_reduce_fn fn, void *user, double *sums) {
  if (!h) return pfail(PNVO_ERR_ARG, "null handle");
  Policy &p = h->p;
  if (fn && !p.cfg.normalize) return pfail(PNVO_ERR_STATE, "pnvo_policy_set_stats_hook: the policy does not normalise its visual inputs");
  if (fn && (!sums || ((uintptr_t)sums & 7))) return pfail(PNVO_ERR_ARG, "pnvo_policy_set_stats_hook: sums must be an 8-byte aligned device buffer");
  p.stats_hook = fn;
  p.stats_user = fn ? user : nullptr;
  p.stats_sums = fn ? sums : nullptr;
  return PNVO_OK;
}

int pnvo_policy_destroy(pnvo_policy_handle h) {
  if (!h) return PNVO_OK;
  Policy &p = h->p;
  (void)hipSetDevice(p.device);
  pnvo_policy_train_free(p);
  if (p.enc) pnvo_destroy(p.enc);
  delete h;
  return PNVO_OK;
}

}  // extern "C"
