// se_gate.hip — the squeeze-and-excite gate of the SE blocks (resnet.py:71-140) in one launch per block.
//
// The block's last GroupNorm output is never materialised: the conv left its raw output x [B,P,C] and the per-sample scale / shift
// pair of its GroupNorm.  One workgroup per sample
//   squeezes   z[c] = scale[c] * mean_p x[p][c] + shift[c]          (the mean of the normalised map, by linearity),
//   excites    g = sigmoid(W2 . relu(W1 . z + b1) + b2),            W1 [R,C], W2 [C,R], R = C / 16,
//   and writes the GATED pair (g * scale, g * shift): residual_kernel then computes relu(g * GN(x) + identity) as it stands.
// Every sum runs in a fixed order: the pixel slices of a channel are added slice by slice, the dot products of the first linear
// layer by a wave butterfly, those of the second sequentially.  P is 6 .. ~1000 and C 128 .. 1024: a sample's map is 24 - 520 KB
// read once, and the launch is latency-bound.
#include "pnvo_internal.h"

namespace pnvo {

typedef float se_f32x4 __attribute__((ext_vector_type(4)));

constexpr int SE_MAX_C = 2048, SE_MAX_R = 128;

bool se_gate_supported(int C, int R) { return C > 0 && C % 4 == 0 && C <= SE_MAX_C && R > 0 && R <= SE_MAX_R; }

__global__ __launch_bounds__(256) void se_gate_kernel(const SeGateArgs a) {
  __shared__ float part[SE_MAX_C];    // [slices][C] partial sums when C <= 1024, else [C]
  __shared__ float z[SE_MAX_C];
  __shared__ float hid[SE_MAX_R];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int C = a.C, Q = C / 4;
  const float *x = a.x + (long)n * a.P * C;
  const float *sc = a.scale + (long)n * C, *sh = a.shift + (long)n * C;
  // squeeze: thread (slice, quad) sums pixels slice, slice + nsl, ... of four channels
  const int nsl = Q >= 256 ? 1 : 256 / Q;           // (nsl * C <= 1024 floats of `part`; threads behind nsl * Q stay idle)
  const int slice = Q >= 256 ? 0 : tid / Q;
  if (slice < nsl)
    for (int q = Q >= 256 ? tid : tid % Q; q < Q; q += 256) {
      se_f32x4 s = {0.f, 0.f, 0.f, 0.f};
      for (long p = slice; p < a.P; p += nsl) s += *reinterpret_cast<const se_f32x4 *>(x + p * C + 4 * q);
      *reinterpret_cast<se_f32x4 *>(&part[slice * C + 4 * q]) = s;
    }
  __syncthreads();
  const float inv_p = 1.f / (float)a.P;
  for (int c = tid; c < C; c += 256) {
    float s = 0.f;
    for (int k = 0; k < nsl; ++k) s += part[k * C + c];
    z[c] = __builtin_fmaf(sc[c], s * inv_p, sh[c]);
  }
  __syncthreads();
  // excite 1: one wave per hidden unit, lanes over the channels
  const int wave = tid >> 6, lane = tid & 63;
  for (int r = wave; r < a.R; r += 4) {
    const float *w = a.w1 + (long)r * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s = __builtin_fmaf(w[c], z[c], s);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) hid[r] = fmaxf(s + a.b1[r], 0.f);
  }
  __syncthreads();
  // excite 2 + sigmoid, and the gated pair
  for (int c = tid; c < C; c += 256) {
    const float *w = a.w2 + (long)c * a.R;
    float s = a.b2[c];
    for (int r = 0; r < a.R; ++r) s = __builtin_fmaf(w[r], hid[r], s);
    const float g = 1.f / (1.f + expf(-s));
    a.out_scale[(long)n * C + c] = g * sc[c];
    a.out_shift[(long)n * C + c] = g * sh[c];
  }
}

hipError_t launch_se_gate(const SeGateArgs &a, hipStream_t s) {
  if (!se_gate_supported(a.C, a.R) || a.B <= 0 || a.P <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(se_gate_kernel, dim3((unsigned)a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace pnvo
