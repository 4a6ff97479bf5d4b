// simple_cnn_train.hip — one PPO minibatch update of the baseline navigation policy (pnvo_baseline_train_* / _evaluate / _ppo_loss /
// _backward / _clip_grad_norm), gfx950 only, float32.  The reference's plain PPOTrainer (rl/ppo/ppo_trainer.py:79-98) does nothing else
// with this policy: PPO(actor_critic=PointNavBaselinePolicy(...)) and agent.update(rollouts).
//
//   evaluate : the retained frames [T*N] -> conv_tile_kernel x 3, fc_splitk_kernel, fc_sum_inputs_kernel of simple_cnn.hip on M = T*N rows
//              (every chain there is independent of the batch size and the row's position: the embedding has the bits act gives)
//              -> G_x = X . W_ih^T + b_ih                                gru_gx_kernel: the summation order of the act path's GRU kernel
//              -> the GRU's T steps, the heads                            core_recurrent_forward (G_x given), core_heads
//   ppo_loss, clip_grad_norm, timing : forwards to the core (ppo_core.hip's PpoCore, pnvo_ppo_core.h: the retained rollout, the recurrent
//              and head kernels, the loss, the clipping — shared with the ResNet policy's update step; this file keeps the SimpleCNN side)
//   backward : core_backward (heads, BPTT, dW_ih / dW_hh and the bias gradients, dX on torch's [3H][K] weight)
//              -> d embed = the first `hidden` columns of dX under the ReLU mask                     relu_mask_cols_kernel
//              -> Linear: db6 = colsum, dW6 = d^T . a3 and dA3 = d . W6 on gemm_f32_kernel.  conv3 writes NHWC, the flat gradient wants the
//                 NCHW flatten's column order: the ACTIVATION is un-permuted (a3 -> [M][32][P], batched_transpose_kernel: 2 * M * F * 4 bytes)
//                 and dW6 is written once, in torch's order, by the GEMM's own epilogue — the 51 MB gradient is never re-laid.  dA3 reads
//                 the handle's column-permuted weight, so it comes out NHWC as conv3's backward reads it.
//              -> conv3, conv2: conv_dgrad_kernel (gather form: one thread-owned output per INPUT pixel, the stride's S x S parity classes
//                 each with (KH / S) x (KW / S) taps, the ReLU mask of the layer below in the epilogue, exact zeros where the floor in the
//                 map size dropped a row or column) and, all three convs, conv_wgrad_kernel + conv_wgrad_reduce_kernel (the pixel range in
//                 slices, one partial [K][COUT] per slice, added in ascending slice order, stored OIHW; the bias gradient rides along).
//                 conv1's weight gradient reads the sensor frames through the forward's own loader (/ 255, channel concatenation).
// Parameters stay in torch's layouts in the caller's flat buffer and gradients land there in torch's layouts; the handle's kernel-layout
// operands ([K][COUT] conv weights, the column-permuted Linear weight, weight_ih_l0 at the padded pitch) are rebuilt from the flat buffer
// on the device by pnvo_baseline_train_refresh.  float32 operands throughout (no normalisation behind any layer absorbs a rounding);
// no atomics: two runs of the same update give the same bits.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pnvo.h"
#include "pnvo_internal.h"
#include "pnvo_model.h"
#include "pnvo_baseline_state.h"
#include "pnvo_policy_state.h"
#include "pnvo_ppo_core.h"

namespace pnvo {

struct BaselineTrain {
  PpoCore core;                       // flat buffers, retained rollout, the recurrent layer's and the heads' scratch
  // flat offsets: conv weights (OIHW) and biases, the Linear (columns in the NCHW flatten's order), the recurrent tensors, the heads
  struct Offsets {
    size_t cw[3] = {0, 0, 0}, cb[3] = {0, 0, 0}, fcw = 0, fcb = 0, wih = 0, whh = 0, bih = 0, bhh = 0, aw = 0, ab = 0, vw = 0, vb = 0;
  } o;
  int rgb_is_u8 = 0;                  // of the last evaluate
  // workspace, sized for core.capM rows: the frames in the dtype given, the forward's activations, the encoder's gradients
  DevBuf<uint8_t> rgb;
  DevBuf<float> depth, a1, a2, a3, part, x, dX;
  DevBuf<float> a3t, d3, d2, d1;      // conv3's map in the NCHW flatten's order; dA3, dA2, dA1 (NHWC)
  DevBuf<float> wpart, bpart;         // weight / bias gradient partials of one conv [slices][K][COUT], [slices][COUT]
};

namespace {

constexpr int WG_BM = 16;             // pixels per tile of the weight-gradient kernel
constexpr int WG_TARGET = 768;        // workgroups a weight gradient is split into (three per CU)

// ------------------------------------------------------------------------------------------------------------ re-lay (refresh)
// OIHW -> [k = (ky * KW + kx) * CIN + c][o]
__global__ __launch_bounds__(256) void relay_conv_w_kernel(const float *src, int CIN, int COUT, int taps, float *dst) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= taps * CIN * COUT) return;
  const int k = e / COUT, o = e % COUT, tap = k / CIN, c = k % CIN;
  dst[e] = src[(o * CIN + c) * taps + tap];
}

// dst[z] [C][R] = src[z] [R][C]^T for nb matrices back to back (whole 128-byte lines on both sides).  The Linear's weight rows,
// [32][P] -> [P][32] (refresh), and conv3's map rows, [P][32] -> [32][P] (backward).
__global__ __launch_bounds__(256) void batched_transpose_kernel(const float *src, int R, int C, long nb, float *dst) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = (int)(threadIdx.x >> 5);
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  for (long z = blockIdx.z; z < nb; z += gridDim.z) {
    const float *s = src + z * R * C;
    float *d = dst + z * R * C;
    for (int i = ty; i < 32; i += 8)
      if (r0 + i < R && c0 + tx < C) tile[i][tx] = s[(long)(r0 + i) * C + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
      if (c0 + i < C && r0 + tx < R) d[(long)(c0 + i) * R + r0 + tx] = tile[tx][i];
    __syncthreads();
  }
}

// [R][K] -> pitch Kp, zero columns behind K
__global__ __launch_bounds__(256) void pad_rows_kernel(const float *src, int R, int K, int Kp, float *dst) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= R * Kp) return;
  const int r = e / Kp, k = e % Kp;
  dst[e] = k < K ? src[r * K + k] : 0.f;
}

// ------------------------------------------------------------------------------------------------------------ G_x of the rollout
// g[m][n] = x[m] . w_ih[n] + b_ih[n] for the 3 Hd gate rows n into the [M, 4 Hd] gate workspace, each sum in the order the act path's
// GRU kernel takes it (lane-strided float4 chains folded across the wave): the rollout forward has the bits of T act calls.
// Workgroup = gate row n, wave = every fourth row m.
__global__ __launch_bounds__(256) void gru_gx_kernel(const float *x, int Kp, const float *w_ih, const float *b_ih, int M, int Hd, float *g) {
  const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6), n = blockIdx.x;
  const f32x4 *wi = reinterpret_cast<const f32x4 *>(w_ih + (long)n * Kp);
  const int K4 = Kp >> 2;
  const float bias = b_ih[n];
  for (int m = wave; m < M; m += 4) {
    const f32x4 *xr = reinterpret_cast<const f32x4 *>(x + (long)m * Kp);
    float s = 0.f;
    for (int k = lane; k < K4; k += 64) {
      const f32x4 w = wi[k], v = xr[k];
      s = __builtin_fmaf(w[0], v[0], s);
      s = __builtin_fmaf(w[1], v[1], s);
      s = __builtin_fmaf(w[2], v[2], s);
      s = __builtin_fmaf(w[3], v[3], s);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) g[(long)m * 4 * Hd + n] = s + bias;
  }
}

// ReLU's backward on the first E columns of d [M, ldd] in place: zero where the layer's output y [M, ldy] is not positive
__global__ __launch_bounds__(256) void relu_mask_cols_kernel(const float *y, int ldy, int M, int E, int ldd, float *d) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)M * E) return;
  const long m = e / E, k = e % E;
  if (!(y[m * ldy + k] > 0.f)) d[m * ldd + k] = 0.f;
}

// ------------------------------------------------------------------------------------------------------------ conv weight gradient
// part[slice][k][o] = sum over the slice's output pixels of in(pixel, k) * dy[pixel][o], k = (ky, kx, c) as the forward's [K][COUT]
// operand: workgroup = one 64-wide chunk of k x one slice of `slice` pixels (a multiple of 16), tiles of 16 pixels through LDS with
// the forward's loader, thread = KC / KG values of k x 4 output channels, pixels in ascending order.  The workgroups of chunk 0 also sum
// dy's columns over their slice (the bias gradient).  Pixels past the end of the range enter with dy = 0.
struct WgradArgs {
  TileArgs t;                         // the forward's view of the layer (out / wt / bias unused)
  const float *dy;                    // [M][COUT]
  float *part, *bpart;                // [slices][K][COUT], [slices][COUT]
  int slice;
};

template <int SRC, int NRGB, int CIN, int KH, int KW, int S, int COUT>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradArgs w) {
  constexpr int BM = WG_BM, TNG = COUT / 4, KG = 256 / TNG, KI = KC / KG, K = KH * KW * CIN;
  static_assert(K % KC == 0 && KC % KG == 0, "whole chunks");
  __shared__ __attribute__((aligned(16))) float As[BM * LDA];
  __shared__ __attribute__((aligned(16))) float Ds[BM * COUT];
  __shared__ unsigned pix[BM];
  const int tid = threadIdx.x, tn = tid % TNG, tk = tid / TNG;
  const int k0 = blockIdx.x * KC, sl = blockIdx.y;
  const int p0 = sl * w.slice, p1 = min(w.t.M, p0 + w.slice);
  float acc[KI][4];
#pragma unroll
  for (int i = 0; i < KI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  float bsum = 0.f;
  for (int m0 = p0; m0 < p1; m0 += BM) {
    __syncthreads();                               // the previous tile has been read
    tile_pixels<S>(w.t, m0, BM, tid, 256, pix);
    for (int g = tid; g < BM * TNG; g += 256) {
      const int m = g / TNG, q = g % TNG;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (m0 + m < p1) v = *reinterpret_cast<const f32x4 *>(w.dy + (size_t)(m0 + m) * COUT + 4 * q);
      *reinterpret_cast<f32x4 *>(&Ds[m * COUT + 4 * q]) = v;
    }
    __syncthreads();
    tile_load_a<SRC, NRGB, CIN, KW>(w.t, pix, k0, BM, tid, 256, As);
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < BM; ++i) {
      const f32x4 d = *reinterpret_cast<const f32x4 *>(&Ds[i * COUT + 4 * tn]);
#pragma unroll
      for (int ii = 0; ii < KI; ++ii) {
        const float a = As[i * LDA + tk + KG * ii];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[ii][j] = __builtin_fmaf(a, d[j], acc[ii][j]);
      }
    }
    if (blockIdx.x == 0 && tid < COUT)
      for (int i = 0; i < BM; ++i) bsum += Ds[i * COUT + tid];
  }
#pragma unroll
  for (int ii = 0; ii < KI; ++ii) {
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = acc[ii][j];
    *reinterpret_cast<f32x4 *>(w.part + ((size_t)sl * K + k0 + tk + KG * ii) * COUT + 4 * tn) = v;
  }
  if (blockIdx.x == 0 && tid < COUT) w.bpart[(size_t)sl * COUT + tid] = bsum;
}

// the slices in ascending order -> the flat gradient: weight OIHW, bias [COUT].  Thread = one element.
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const float *part, const float *bpart, int ns, int K, int CIN, int COUT,
                                                              float *gw, float *gb) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < K * COUT) {
    float s = 0.f;
    for (int sl = 0; sl < ns; ++sl) s += part[(size_t)sl * K * COUT + e];
    const int k = e / COUT, o = e % COUT, tap = k / CIN, c = k % CIN;
    gw[(o * CIN + c) * (K / CIN) + tap] = s;
  } else if (e < K * COUT + COUT) {
    const int o = e - K * COUT;
    float s = 0.f;
    for (int sl = 0; sl < ns; ++sl) s += bpart[(size_t)sl * COUT + o];
    gb[o] = s;
  }
}

// ------------------------------------------------------------------------------------------------------------ conv data gradient
// dx[b][iy][ix][c] = (act > 0) * sum over (ky, kx, o) with iy = oy * S + ky, ix = ox * S + kx of dy[b][oy][ox][o] * w[(ky, kx, c)][o],
// gathered: a thread owns 4 channels of TM input pixels, nothing is scattered.  An input pixel of parity class (iy % S, ix % S) =
// (cy, cx) meets the taps ky = cy + S a, kx = cx + S b only, (KH / S) x (KW / S) of them, at the output pixel (iy / S - a, ix / S - b);
// blockIdx.y = class, so the taps are uniform over a workgroup.  One tap = one LDS chunk: the tile's dy rows [BM][COUT] (zeros where
// the output pixel does not exist) and the tap's weights transposed to [o][c].  One fmaf chain per output over (tap, o) ascending.
// Input rows / columns behind the last window (dropped by the floor in the map size) find no output pixel and get exactly 0.
struct DgradArgs {
  const float *dy;                    // [B][OH][OW][COUT]
  const float *wt;                    // [KH*KW*CIN][COUT]
  const float *act;                   // [B][H][W][CIN]: the layer's input (a ReLU's output)
  float *dx;                          // [B][H][W][CIN]
  int B, H, W, OH, OW;
};

template <int CIN, int KH, int KW, int S, int COUT, int TM>
__global__ __launch_bounds__(4 * CIN) void conv_dgrad_kernel(DgradArgs a) {
  constexpr int BM = 16 * TM, TNG = CIN / 4, NT = 16 * TNG, TH = KH / S, TW = KW / S, LDD = COUT + 4;
  static_assert(KH % S == 0 && KW % S == 0, "every parity class has the same number of taps");
  __shared__ __attribute__((aligned(16))) float As[BM * LDD];
  __shared__ __attribute__((aligned(16))) float Bs[COUT * CIN];
  __shared__ int pb[BM], py[BM], px[BM];           // batch index (-1 past the end), iy / S, ix / S of the tile's pixels
  const int tid = threadIdx.x, tn = tid % TNG, tm = tid / TNG;
  const int cy = (int)blockIdx.y / S, cx = (int)blockIdx.y % S;
  const int Hc = (a.H - cy + S - 1) / S, Wc = (a.W - cx + S - 1) / S;
  const long Mc = (long)a.B * Hc * Wc;
  const long m0 = (long)blockIdx.x * BM;
  if (m0 >= Mc) return;                            // (uniform: the grid is sized for class (0, 0), the largest)
  for (int i = tid; i < BM; i += NT) {
    const long m = m0 + i;
    const int b = (int)(m / ((long)Hc * Wc)), r = (int)(m - (long)b * Hc * Wc);
    pb[i] = m < Mc ? b : -1;
    py[i] = r / Wc;
    px[i] = r % Wc;
  }
  float acc[TM][4];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int t = 0; t < TH * TW; ++t) {
    const int ta = t / TW, tb = t % TW, tap = (cy + S * ta) * KW + cx + S * tb;
    __syncthreads();                               // the previous tap has been read (first pass: pb / py / px are written)
    for (int g = tid; g < BM * (COUT / 4); g += NT) {
      const int m = g / (COUT / 4), q = g % (COUT / 4);
      const int oy = py[m] - ta, ox = px[m] - tb;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (pb[m] >= 0 && oy >= 0 && oy < a.OH && ox >= 0 && ox < a.OW)
        v = *reinterpret_cast<const f32x4 *>(a.dy + (((size_t)pb[m] * a.OH + oy) * a.OW + ox) * COUT + 4 * q);
      *reinterpret_cast<f32x4 *>(&As[m * LDD + 4 * q]) = v;
    }
    for (int g = tid; g < COUT * CIN; g += NT) {
      const int o = g / CIN, c = g % CIN;
      Bs[g] = a.wt[((size_t)tap * CIN + c) * COUT + o];
    }
    __syncthreads();
#pragma unroll 2
    for (int o = 0; o < COUT; o += 4) {
      f32x4 av[TM];
#pragma unroll
      for (int i = 0; i < TM; ++i) av[i] = *reinterpret_cast<const f32x4 *>(&As[(tm + 16 * i) * LDD + o]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f32x4 bv = *reinterpret_cast<const f32x4 *>(&Bs[(o + e) * CIN + 4 * tn]);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(av[i][e], bv[j], acc[i][j]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int l = tm + 16 * i;
    if (pb[l] < 0) continue;
    const size_t idx = (((size_t)pb[l] * a.H + py[l] * S + cy) * a.W + px[l] * S + cx) * CIN + 4 * tn;
    const f32x4 y = *reinterpret_cast<const f32x4 *>(a.act + idx);
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = y[j] > 0.f ? acc[i][j] : 0.f;
    *reinterpret_cast<f32x4 *>(a.dx + idx) = v;
  }
}

// the tile by the number of input pixels, as launch_conv picks the forward's
template <int CIN, int KH, int KW, int S, int COUT>
hipError_t launch_dgrad(const DgradArgs &a, hipStream_t s) {
  const long mc = (long)a.B * ((a.H + S - 1) / S) * ((a.W + S - 1) / S);      // class (0, 0)
  const dim3 nt(4 * CIN);
  if (mc >= 64 * 1024)
    hipLaunchKernelGGL((conv_dgrad_kernel<CIN, KH, KW, S, COUT, 4>), dim3((unsigned)((mc + 63) / 64), S * S), nt, 0, s, a);
  else if (mc >= 32 * 512)
    hipLaunchKernelGGL((conv_dgrad_kernel<CIN, KH, KW, S, COUT, 2>), dim3((unsigned)((mc + 31) / 32), S * S), nt, 0, s, a);
  else
    hipLaunchKernelGGL((conv_dgrad_kernel<CIN, KH, KW, S, COUT, 1>), dim3((unsigned)((mc + 15) / 16), S * S), nt, 0, s, a);
  return hipGetLastError();
}

// pixels per slice (a multiple of the tile) and the number of slices of a weight gradient over `pixels` output pixels in `chunks` k chunks
void wgrad_slices(long pixels, int chunks, int *slice, int *ns) {
  const long want = std::max(1, WG_TARGET / chunks);
  long sl = (pixels + want - 1) / want;
  sl = std::max<long>(WG_BM, (sl + WG_BM - 1) / WG_BM * WG_BM);
  *slice = (int)sl;
  *ns = (int)((pixels + sl - 1) / sl);
}

template <int SRC, int NRGB, int CIN, int KH, int KW, int S, int COUT>
int launch_wgrad(BaselineTrain *t, const TileArgs &ta, const float *dy, float *gw, float *gb, hipStream_t s) {
  constexpr int K = KH * KW * CIN;
  int slice = 0, ns = 0;
  wgrad_slices(ta.M, K / KC, &slice, &ns);
  if (t->wpart.size() < (size_t)ns * K * COUT || t->bpart.size() < (size_t)ns * COUT)
    return pfail(PNVO_ERR_STATE, "weight-gradient scratch is smaller than the layer needs");      // (reserve_wgrad sizes it for all three)
  WgradArgs w{ta, dy, t->wpart, t->bpart, slice};
  hipLaunchKernelGGL((conv_wgrad_kernel<SRC, NRGB, CIN, KH, KW, S, COUT>), dim3(K / KC, (unsigned)ns), dim3(256), 0, s, w);
  hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3((unsigned)((K * COUT + COUT + 255) / 256)), dim3(256), 0, s, t->wpart, t->bpart, ns, K, CIN,
                     COUT, gw, gb);
  PCHK(hipGetLastError());
  return PNVO_OK;
}

// the partials of the largest of the three weight gradients over M rows, before anything of the backward is launched (a regrow
// between two layers would free memory an enqueued kernel still writes)
int reserve_wgrad(const Baseline &p, BaselineTrain *t, int M) {
  const int K[3] = {64 * p.C, 512, 576}, co[3] = {32, 64, 32};
  size_t w = 0, b = 0;
  for (int l = 0; l < 3; ++l) {
    int slice = 0, ns = 0;
    wgrad_slices((long)M * p.oh[l] * p.ow[l], K[l] / KC, &slice, &ns);
    w = std::max(w, (size_t)ns * K[l] * co[l]);
    b = std::max(b, (size_t)ns * co[l]);
  }
  PCHK(t->wpart.reserve(w));
  PCHK(t->bpart.reserve(b));
  return PNVO_OK;
}

hipError_t launch_batched_transpose(const float *src, int R, int C, long nb, float *dst, hipStream_t s) {
  hipLaunchKernelGGL(batched_transpose_kernel, dim3((unsigned)((C + 31) / 32), (unsigned)((R + 31) / 32), (unsigned)std::min<long>(nb, 4096)),
                     dim3(256), 0, s, src, R, C, nb, dst);
  return hipGetLastError();
}


// the handle's kernel-layout operands from the flat parameter buffer
int relay_operands(Baseline &p, BaselineTrain *t, hipStream_t s) {
  const pnvo_baseline_config &c = p.cfg;
  const int Hd = c.hidden, K = p.E + c.goal_dim;
  if (!blind(c)) {
    const int kk[3] = {8, 4, 3}, ci[3] = {p.C, 32, 64}, co[3] = {32, 64, 32};
    for (int l = 0; l < 3; ++l) {
      const int taps = kk[l] * kk[l], nel = taps * ci[l] * co[l];
      hipLaunchKernelGGL(relay_conv_w_kernel, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, s, t->core.params + t->o.cw[l], ci[l], co[l], taps,
                         (float *)p.cw[l]);
    }
    PCHK(launch_batched_transpose(t->core.params + t->o.fcw, 32, p.oh[2] * p.ow[2], Hd, p.fcw, s));
  }
  hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)((3 * Hd * p.Kp + 255) / 256)), dim3(256), 0, s, t->core.params + t->o.wih, 3 * Hd, K, p.Kp,
                     (float *)p.w_ih);
  PCHK(hipGetLastError());
  return PNVO_OK;
}

// the GRU layer as the core reads it: torch's weight_ih_l0 [3H][K] in the flat buffer, the input rows x [M][K] at pitch Kp
RnnLayer baseline_layer(const Baseline &p, const BaselineTrain *t) {
  return {t->core.params + t->o.wih, p.w_hh, p.b_ih, p.b_hh, p.E + p.cfg.goal_dim, p.Kp};
}
Heads baseline_heads(const Baseline &p) { return {p.act_w, p.act_b, p.cr_w, p.cr_b}; }

void free_ws(BaselineTrain *t) {
  for (DevBuf<float> *b : {&t->depth, &t->a1, &t->a2, &t->a3, &t->part, &t->x, &t->dX, &t->a3t, &t->d3, &t->d2, &t->d1}) b->reset();
  t->rgb.reset();
  core_release(&t->core);
}

int ensure_ws(Baseline &p, BaselineTrain *t, int M, int N) {
  if (M > t->core.capM) {
    free_ws(t);                                    // the old workspace goes first; a failed regrow leaves core.capM = 0
    const pnvo_baseline_config &c = p.cfg;
    const size_t Hd = (size_t)c.hidden, m = (size_t)M, K = (size_t)(p.E + c.goal_dim);
    if (!blind(c)) {
      const size_t px = (size_t)c.height * c.width;
      if (c.rgb_channels) PCHK(t->rgb.alloc(m * px * 3 * sizeof(float)));      // (either dtype fits)
      if (c.depth_channels) PCHK(t->depth.alloc(m * px));
      const size_t n1 = m * p.oh[0] * p.ow[0] * 32, n2 = m * p.oh[1] * p.ow[1] * 64, n3 = m * p.F;
      PCHK(t->a1.alloc(n1));
      PCHK(t->a2.alloc(n2));
      PCHK(t->a3.alloc(n3));
      PCHK(t->part.alloc((size_t)p.nks * m * Hd));
      PCHK(t->d1.alloc(n1));
      PCHK(t->d2.alloc(n2));
      PCHK(t->d3.alloc(n3));
      PCHK(t->a3t.alloc(n3));
    }
    PCHK(t->x.alloc(m * p.Kp));
    PCHK(t->dX.alloc(m * K));
  }
  return core_reserve(&t->core, M, N);
}

}  // namespace

void pnvo_baseline_train_free(Baseline &p) {
  delete p.train;
  p.train = nullptr;
}

}  // namespace pnvo

using namespace pnvo;

#define TRAIN_OR_FAIL(h)                                                                        \
  if (!(h) || !(h)->p.train) return pfail(PNVO_ERR_STATE, "pnvo_baseline_train_attach first")

extern "C" {

int pnvo_baseline_train_attach(pnvo_baseline_handle h, float *params, float *grads, size_t n_floats, const pnvo_tensor_desc *toc, int ntoc) {
  if (!h || !params || !grads || !toc || ntoc < 0) return pfail(PNVO_ERR_ARG, "null argument");
  Baseline &p = h->p;
  if (!p.loaded) return pfail(PNVO_ERR_STATE, "pnvo_baseline_train_attach before pnvo_baseline_load_weights");
  if (((uintptr_t)params & 15) != 0 || ((uintptr_t)grads & 15) != 0) return pfail(PNVO_ERR_ARG, "flat parameter / gradient buffer is not 16-byte aligned");
  PCHK(hipSetDevice(p.device));
  const pnvo_baseline_config &c = p.cfg;
  const int64_t Hd = c.hidden, A = c.n_actions, K = p.E + c.goal_dim;
  int rc = PNVO_OK;
  BaselineTrain::Offsets o;            // collected here: nothing of the handle changes before every entry has been checked
  // rows the kernels read as 16-byte vectors must start at a multiple of 4 floats
  auto find = [&](const std::string &name, std::vector<int64_t> shape, bool f4, size_t *off) -> bool {
    PolicyParam e{name, std::move(shape), nullptr, f4};
    const pnvo_tensor_desc *d = policy_find(toc, ntoc, e, n_floats, &rc);
    if (!d) return false;
    if (f4 && d->offset % 4 != 0) {
      rc = pfail(PNVO_ERR_ARG, "parameter '" + name + "' starts at float " + std::to_string(d->offset) + ", not a multiple of 4 (its rows are read as float4)");
      return false;
    }
    *off = (size_t)d->offset;
    return true;
  };
  const std::string cnn = "net.visual_encoder.cnn.", rnn = "net.state_encoder.rnn.";
  if (!blind(c)) {
    const int64_t kk[3] = {8, 4, 3}, ci[3] = {p.C, 32, 64}, co[3] = {32, 64, 32};
    for (int l = 0; l < 3; ++l) {
      const std::string pre = cnn + std::to_string(2 * l);
      if (!find(pre + ".weight", {co[l], ci[l], kk[l], kk[l]}, false, &o.cw[l]) || !find(pre + ".bias", {co[l]}, true, &o.cb[l])) return rc;
    }
    if (!find(cnn + "6.weight", {Hd, (int64_t)p.F}, true, &o.fcw) || !find(cnn + "6.bias", {Hd}, false, &o.fcb)) return rc;
  }
  if (!find(rnn + "weight_ih_l0", {3 * Hd, K}, false, &o.wih) || !find(rnn + "weight_hh_l0", {3 * Hd, Hd}, true, &o.whh) ||
      !find(rnn + "bias_ih_l0", {3 * Hd}, false, &o.bih) || !find(rnn + "bias_hh_l0", {3 * Hd}, false, &o.bhh) ||
      !find("action_distribution.linear.weight", {A, Hd}, true, &o.aw) || !find("action_distribution.linear.bias", {A}, false, &o.ab) ||
      !find("critic.fc.weight", {1, Hd}, true, &o.vw) || !find("critic.fc.bias", {1}, false, &o.vb))
    return rc;
  size_t n_named = 0;
  for (int k = 0; k < ntoc; ++k) {
    if (toc[k].ndim < 0 || toc[k].ndim > 4) return pfail(PNVO_ERR_ARG, "parameter table entry " + std::to_string(k) + " has a bad rank");
    const size_t end = (size_t)toc[k].offset + numel(std::vector<int64_t>(toc[k].shape, toc[k].shape + toc[k].ndim));
    if (end > n_floats) return pfail(PNVO_ERR_ARG, "parameter table entry " + std::to_string(k) + " ends behind the flat buffer");
    n_named = std::max(n_named, end);
  }
  pnvo_baseline_train_free(p);
  BaselineTrain *t = new BaselineTrain();
  p.train = t;
  t->o = o;
  rc = [&]() -> int {
    const int rc1 = core_init(&t->core, "pnvo_baseline", p.device, params, grads, n_floats, n_named, c.hidden, 1, c.n_actions, true);
    if (rc1 != PNVO_OK) return rc1;
    const int rc2 = relay_operands(p, t, nullptr);
    if (rc2 != PNVO_OK) return rc2;
    PCHK(hipDeviceSynchronize());
    return PNVO_OK;
  }();
  if (rc != PNVO_OK) {                  // no half-built train step is left behind
    pnvo_baseline_train_free(p);
    return rc;
  }
  // the tensors in torch's layout are read from the flat buffer from now on (pnvo_baseline_act / _encode included): no second copy
  p.owned.clear();
  p.attached = true;
  if (!blind(c)) {
    for (int l = 0; l < 3; ++l) p.cb[l] = params + o.cb[l];
    p.fcb = params + o.fcb;
  }
  p.w_hh = params + o.whh, p.b_ih = params + o.bih, p.b_hh = params + o.bhh;
  p.act_w = params + o.aw, p.act_b = params + o.ab, p.cr_w = params + o.vw, p.cr_b = params + o.vb;
  return PNVO_OK;
}

int pnvo_baseline_train_refresh(pnvo_baseline_handle h, void *stream) {
  TRAIN_OR_FAIL(h);
  PCHK(hipSetDevice(h->p.device));
  return relay_operands(h->p, h->p.train, (hipStream_t)stream);
}

int pnvo_baseline_evaluate(pnvo_baseline_handle h, const void *rgb, int rgb_is_u8, const float *depth, const float *goal, const float *masks,
                           const float *hidden_in, int T, int N, const int64_t *actions, float *hidden_out, float *value, float *logp,
                           float *entropy, void *stream) {
  TRAIN_OR_FAIL(h);
  Baseline &p = h->p;
  BaselineTrain *t = p.train;
  const pnvo_baseline_config &c = p.cfg;
  const int Hd = c.hidden;
  int rc = core_check_rollout("pnvo_baseline_evaluate", T, N, {goal, masks, actions}, hidden_in, hidden_out, (size_t)N * Hd, "N * hidden");
  if (rc != PNVO_OK) return rc;
  const int M = T * N;
  if ((rc = baseline_frames_check(p, "pnvo_baseline_evaluate", rgb, rgb_is_u8, depth, M)) != PNVO_OK) return rc;
  PCHK(hipSetDevice(p.device));
  hipStream_t s = (hipStream_t)stream;
  if ((rc = ensure_ws(p, t, M, N)) != PNVO_OK) return rc;
  t->rgb_is_u8 = rgb_is_u8;
  if ((rc = core_keep(&t->core, T, N, masks, actions, hidden_in, s)) != PNVO_OK) return rc;
  const size_t px = (size_t)M * c.height * c.width;
  if (rgb) PCHK(hipMemcpyAsync(t->rgb, rgb, px * 3 * (rgb_is_u8 ? 1 : sizeof(float)), hipMemcpyDeviceToDevice, s));
  if (depth) PCHK(hipMemcpyAsync(t->depth, depth, px * sizeof(float), hipMemcpyDeviceToDevice, s));
  PCHK(core_mark(&t->core, 0, s));
  if (!blind(c) && (rc = baseline_encoder_launches(p, rgb ? (const void *)t->rgb : nullptr, rgb_is_u8, depth ? (const float *)t->depth : nullptr, M,
                                                   t->a1, t->a2, t->a3, t->part, s)) != PNVO_OK)
    return rc;
  PCHK(baseline_sum_inputs(p, t->part, goal, M, t->x, nullptr, s));
  PCHK(core_mark(&t->core, 1, s));
  hipLaunchKernelGGL(gru_gx_kernel, dim3((unsigned)(3 * Hd)), dim3(256), 0, s, t->x, p.Kp, p.w_ih, p.b_ih, M, Hd, t->core.gates[0]);
  PCHK(hipGetLastError());
  const RnnLayer layer = baseline_layer(p, t);
  if ((rc = core_recurrent_forward(&t->core, &layer, t->x, true, hidden_out, s)) != PNVO_OK) return rc;
  return core_heads(&t->core, baseline_heads(p), value, logp, entropy, s);
}

int pnvo_baseline_ppo_loss(pnvo_baseline_handle h, const float *actions_logp_old, const float *adv, const float *value_preds,
                           const float *returns, float clip, float value_coef, float entropy_coef, int use_clipped_value_loss, float *out3,
                           void *stream) {
  TRAIN_OR_FAIL(h);
  return core_ppo_loss(&h->p.train->core, actions_logp_old, adv, value_preds, returns, clip, value_coef, entropy_coef, use_clipped_value_loss,
                       out3, (hipStream_t)stream);
}

int pnvo_baseline_backward(pnvo_baseline_handle h, int train_encoder, void *stream) {
  TRAIN_OR_FAIL(h);
  Baseline &p = h->p;
  BaselineTrain *t = p.train;
  int rc = core_backward_ready(&t->core);
  if (rc != PNVO_OK) return rc;
  PCHK(hipSetDevice(p.device));
  hipStream_t s = (hipStream_t)stream;
  const pnvo_baseline_config &c = p.cfg;
  const int Hd = c.hidden, M = t->core.M, K = p.E + c.goal_dim, Kp = p.Kp;
  const bool encoder = !blind(c) && train_encoder != 0;
  float *G = t->core.grads;
  auto g = [&](size_t off) { return G + off; };
  if (encoder && (rc = reserve_wgrad(p, t, M)) != PNVO_OK) return rc;
  PCHK(core_mark(&t->core, 5, s));
  // overwrite semantics; a frozen encoder's range stays zero.  The Linear's weight gradient, 51 MB at the reference's frame, is written
  // in full by its GEMM: it is left out of the clear
  if (encoder) {
    const size_t lo = t->o.fcw, hi = t->o.fcw + (size_t)Hd * p.F;
    if (lo > 0) PCHK(hipMemsetAsync(G, 0, lo * sizeof(float), s));
    if (t->core.n > hi) PCHK(hipMemsetAsync(G + hi, 0, (t->core.n - hi) * sizeof(float), s));
  } else {
    PCHK(hipMemsetAsync(G, 0, t->core.n * sizeof(float), s));
  }
  // blind, or net.visual_encoder frozen: no dX, and the encoder's range stays at the clear's zeros
  const RnnLayer layer = baseline_layer(p, t);
  if ((rc = core_backward(&t->core, &layer, baseline_heads(p), t->x, encoder ? (float *)t->dX : nullptr, s)) != PNVO_OK) return rc;
  if (!encoder) {
    PCHK(core_mark(&t->core, 6, s));
    PCHK(core_mark(&t->core, 7, s));
    return PNVO_OK;
  }
  // d embed = the first `hidden` columns of dX under the Linear's ReLU
  hipLaunchKernelGGL(relu_mask_cols_kernel, dim3((unsigned)(((long)M * Hd + 255) / 256)), dim3(256), 0, s, t->x, Kp, M, Hd, K, t->dX);
  PCHK(hipGetLastError());
  PCHK(core_mark(&t->core, 6, s));
  // the Linear: db6, dW6 = d^T . a3 (a3 un-permuted to the NCHW flatten's order, the gradient written in torch's layout), dA3 = d . W6
  const int P3 = p.oh[2] * p.ow[2], F = p.F;
  PCHK(launch_colsum(t->dX, M, Hd, K, g(t->o.fcb), s));
  PCHK(launch_batched_transpose(t->a3, P3, 32, M, t->a3t, s));
  GemmArgs dw6{t->dX, t->a3t, nullptr, nullptr, g(t->o.fcw), Hd, F, M, 1, (long)K, (long)F, 1, (long)F};
  PCHK(launch_gemm_f32(dw6, false, false, s));
  GemmArgs da3{t->dX, p.fcw, nullptr, nullptr, t->d3, M, F, Hd, (long)K, 1, (long)F, 1, (long)F};
  PCHK(launch_gemm_f32(da3, true, false, s));
  // conv3 (3x3, stride 1, 64 -> 32; no ReLU behind it)
  TileArgs t3{nullptr, nullptr, t->a2, nullptr, nullptr, nullptr, M * P3, p.oh[1], p.ow[1], p.oh[2], p.ow[2]};
  if ((rc = launch_wgrad<0, 0, 64, 3, 3, 1, 32>(t, t3, t->d3, g(t->o.cw[2]), g(t->o.cb[2]), s)) != PNVO_OK) return rc;
  DgradArgs g3{t->d3, p.cw[2], t->a2, t->d2, M, p.oh[1], p.ow[1], p.oh[2], p.ow[2]};
  PCHK((launch_dgrad<64, 3, 3, 1, 32>(g3, s)));
  // conv2 (4x4, stride 2, 32 -> 64)
  TileArgs t2{nullptr, nullptr, t->a1, nullptr, nullptr, nullptr, M * p.oh[1] * p.ow[1], p.oh[0], p.ow[0], p.oh[1], p.ow[1]};
  if ((rc = launch_wgrad<0, 0, 32, 4, 4, 2, 64>(t, t2, t->d2, g(t->o.cw[1]), g(t->o.cb[1]), s)) != PNVO_OK) return rc;
  DgradArgs g2{t->d2, p.cw[1], t->a1, t->d1, M, p.oh[0], p.ow[0], p.oh[1], p.ow[1]};
  PCHK((launch_dgrad<32, 4, 4, 2, 64>(g2, s)));
  // conv1 (8x8, stride 4, frames -> 32): the weight gradient alone, through the forward's frame loader
  const void *rgb = c.rgb_channels ? (const void *)t->rgb : nullptr;
  TileArgs t1{rgb, c.depth_channels ? (const float *)t->depth : nullptr, nullptr, nullptr, nullptr, nullptr, M * p.oh[0] * p.ow[0], c.height, c.width,
              p.oh[0], p.ow[0]};
  float *gw1 = g(t->o.cw[0]), *gb1 = g(t->o.cb[0]);
  if (c.rgb_channels && c.depth_channels)
    rc = t->rgb_is_u8 ? launch_wgrad<2, 3, 4, 8, 8, 4, 32>(t, t1, t->d1, gw1, gb1, s) : launch_wgrad<1, 3, 4, 8, 8, 4, 32>(t, t1, t->d1, gw1, gb1, s);
  else if (c.rgb_channels)
    rc = t->rgb_is_u8 ? launch_wgrad<2, 3, 3, 8, 8, 4, 32>(t, t1, t->d1, gw1, gb1, s) : launch_wgrad<1, 3, 3, 8, 8, 4, 32>(t, t1, t->d1, gw1, gb1, s);
  else
    rc = launch_wgrad<1, 0, 1, 8, 8, 4, 32>(t, t1, t->d1, gw1, gb1, s);
  if (rc != PNVO_OK) return rc;
  PCHK(core_mark(&t->core, 7, s));
  return PNVO_OK;
}

int pnvo_baseline_clip_grad_norm(pnvo_baseline_handle h, float max_norm, float *norm_out, void *stream) {
  TRAIN_OR_FAIL(h);
  if (!(max_norm > 0.f)) return pfail(PNVO_ERR_ARG, "max_grad_norm " + std::to_string(max_norm) + " must be > 0");
  return core_clip_grad_norm(&h->p.train->core, 1.f, max_norm, norm_out, (hipStream_t)stream);
}

int pnvo_baseline_train_timing(pnvo_baseline_handle h, int mode) {
  TRAIN_OR_FAIL(h);
  return core_timing(&h->p.train->core, mode);
}

int pnvo_baseline_train_timing_read(pnvo_baseline_handle h, double ms[5]) {
  if (!h || !h->p.train || !ms) return pfail(PNVO_ERR_STATE, "pnvo_baseline_train_attach first");
  return core_timing_read(&h->p.train->core, ms);
}

}  // extern "C"
