// conv_group.hip — the grouped 3x3 convolution of the ResNeXt blocks (resnet.py:58-69 with groups = cardinality: the first block of
// each stage, resnet.py:198-210) on the float32-input matrix cores, exact float32 arithmetic (v_mfma_f32_16x16x4_f32: a k-ordered
// fmaf chain).
//
// Contract of the convs behind pnvo_run_conv: NHWC input with the producer's per-sample relu(x * scale + shift) applied while the
// operand is fetched, raw NHWC output, per-(sample, slot, channel) partial (sum, sum of squares) in the slots launch_gn_finalize
// reads, every reduction in a fixed order (no atomics).  Stride 1 or 2, pad 1, any map size.
//
// Geometry.  cg = channels per group (4, 8, 16 or 32; C a multiple of 32).  The channel axis is cut into slabs of S = max(cg, 16)
// channels: the outputs of a slab read the inputs of the same slab only (groups never straddle a slab).  One wave owns
// (sample, 32 output pixels, slab): two 16-pixel tiles x S/16 tiles of 16 output channels, 2 or 4 independent accumulators (the
// 16x16x4 form needs two to issue back to back).  The weight operand is packed on the host per (slab, tap, 4-channel step, output
// tile) as the 64 lane values of the MFMA's A operand — W[o = lane & 15][k = lane >> 4], zero where input channel and output channel
// belong to different groups (cg < 16: 16 / cg groups share an output tile) — so a wave reads 256 contiguous bytes per MFMA and the
// same lines serve every pixel tile of the launch out of L2.  The B operand is the activation, X[k = lane >> 4][pixel = lane & 15],
// fetched from global memory per (tap, step): the maps are 24 x 43 and smaller, L2-resident, and the launch is latency-bound long
// before it is bandwidth-bound.  D has the output channel on (lane >> 4, register) and the pixel on lane & 15:
// one float4 store per accumulator, and the statistics are a 16-lane butterfly over the pixels.
#include "pnvo_internal.h"

namespace pnvo {

typedef float gc_f32x4 __attribute__((ext_vector_type(4)));

int conv_group_slots(int P) { return (P + 31) / 32; }

bool conv_group_supported(int C, int cg, int ks, int stride, int pad) {
  return ks == 3 && pad == 1 && (stride == 1 || stride == 2) && C > 0 && C % 32 == 0 && (cg == 4 || cg == 8 || cg == 16 || cg == 32);
}

size_t conv_group_packed_floats(int C, int cg) {
  const int S = cg > 16 ? cg : 16;
  return (size_t)(C / S) * 9 * (S / 4) * (S / 16) * 64;
}

// w: [C][cg][3][3] (torch's grouped OIHW) -> out[slab][tap][j][nt][lane]
void pack_conv_group_weight(const float *w, int C, int cg, float *out) {
  const int S = cg > 16 ? cg : 16, J = S / 4, NT = S / 16;
  for (int sl = 0; sl < C / S; ++sl)
    for (int tap = 0; tap < 9; ++tap)
      for (int j = 0; j < J; ++j)
        for (int nt = 0; nt < NT; ++nt)
          for (int lane = 0; lane < 64; ++lane) {
            const int o = sl * S + nt * 16 + (lane & 15), ci = sl * S + 4 * j + (lane >> 4);
            const int g = o / cg, cl = ci - g * cg;
            out[((((size_t)sl * 9 + tap) * J + j) * NT + nt) * 64 + lane] =
                (cl >= 0 && cl < cg) ? w[((size_t)o * cg + cl) * 9 + tap] : 0.f;
          }
}

// S: slab width (16 or 32)
template <int S>
__global__ __launch_bounds__(256) void conv_group_kernel(const ConvGroupArgs a) {
  constexpr int J = S / 4, NT = S / 16;
  const int lane = threadIdx.x & 63;
  const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nslab = a.C / S;
  const long nwork = (long)a.B * a.slots * nslab;
  if (wid >= nwork) return;                        // (wave-uniform)
  const int sl = (int)(wid % nslab);
  const long r = wid / nslab;
  const int slot = (int)(r % a.slots), n = (int)(r / a.slots);
  const int P = a.Ho * a.Wo;
  const int kq = lane >> 4, px = lane & 15;
  const int cbase = sl * S;

  // the producer's GroupNorm scale / shift of this lane's J input channels
  float sc[J], sh[J];
  const bool norm = a.in_scale != nullptr;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int c = cbase + 4 * j + kq;
    sc[j] = norm ? a.in_scale[(long)n * a.C + c] : 1.f;
    sh[j] = norm ? a.in_shift[(long)n * a.C + c] : 0.f;
  }
  int oh[2], ow[2];
  bool pv[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int p = slot * 32 + t * 16 + px;
    pv[t] = p < P;
    const int pc = pv[t] ? p : 0;
    oh[t] = pc / a.Wo;
    ow[t] = pc % a.Wo;
  }
  gc_f32x4 acc[2][NT];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[t][nt] = gc_f32x4{0.f, 0.f, 0.f, 0.f};

  const float *wp = a.wpk + (size_t)sl * 9 * J * NT * 64 + lane;
  const float *xn = a.x + (long)n * a.H * a.W * a.C + cbase + kq;
  for (int tap = 0; tap < 9; ++tap) {
    const int kh = tap / 3, kw = tap % 3;
    const float *xp[2];
    bool v[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int ih = oh[t] * a.stride - 1 + kh, iw = ow[t] * a.stride - 1 + kw;
      v[t] = pv[t] && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
      xp[t] = xn + ((long)(v[t] ? ih : 0) * a.W + (v[t] ? iw : 0)) * a.C;
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
      float b[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float xv = 0.f;
        if (v[t]) {
          xv = xp[t][4 * j];
          if (norm) xv = fmaxf(__builtin_fmaf(xv, sc[j], sh[j]), 0.f);
        }
        b[t] = xv;
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const float w = wp[((size_t)(tap * J + j) * NT + nt) * 64];
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[t][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, b[t], acc[t][nt], 0, 0, 0);
      }
    }
  }

  // epilogue: raw output (channel 4 * kq + i of output tile nt, pixel px of pixel tile t) and the slot's per-channel partial sums:
  // tile 0 + tile 1 per lane, then a butterfly over the 16 pixel lanes — the same order on every run
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int c0 = cbase + nt * 16 + 4 * kq;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int p = slot * 32 + t * 16 + px;
      if (p < P) *reinterpret_cast<gc_f32x4 *>(a.y + ((long)n * P + p) * a.C + c0) = acc[t][nt];
    }
    if (a.stats != nullptr) {
      float s1[4], s2[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float u = acc[0][nt][i], w = acc[1][nt][i];   // (pixels past the map hold exact zeros: every operand was masked)
        s1[i] = u + w;
        s2[i] = __builtin_fmaf(u, u, w * w);
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          s1[i] += __shfl_xor(s1[i], o);
          s2[i] += __shfl_xor(s2[i], o);
        }
      if (px == 0) {
        float *dst = a.stats + (((long)n * a.slots + slot) * a.C + c0) * 2;
        *reinterpret_cast<gc_f32x4 *>(dst) = gc_f32x4{s1[0], s2[0], s1[1], s2[1]};
        *reinterpret_cast<gc_f32x4 *>(dst + 4) = gc_f32x4{s1[2], s2[2], s1[3], s2[3]};
      }
    }
  }
}

hipError_t launch_conv_group(const ConvGroupArgs &a, hipStream_t s) {
  if (!conv_group_supported(a.C, a.cg, 3, a.stride, 1) || a.slots != conv_group_slots(a.Ho * a.Wo) || a.B <= 0) return hipErrorInvalidValue;
  const int S = a.cg > 16 ? a.cg : 16;
  const long nwork = (long)a.B * a.slots * (a.C / S);
  const unsigned blocks = (unsigned)((nwork + 3) / 4);
  if (S == 16)
    hipLaunchKernelGGL(conv_group_kernel<16>, dim3(blocks), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(conv_group_kernel<32>, dim3(blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace pnvo
