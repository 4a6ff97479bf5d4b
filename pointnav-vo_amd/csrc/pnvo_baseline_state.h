// pnvo_baseline_state.h — the baseline navigation policy's handle and what its per-step forward (simple_cnn.hip) shares with its PPO
// update step (simple_cnn_train.hip): the conv tile's arguments and loader (the backward reads the same operands the same way), and the
// launches of the forward on caller-named buffers.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/pnvo.h"
#include "pnvo_model.h"
#include "pnvo_policy_state.h"

namespace pnvo {

struct BaselineTrain;                // simple_cnn_train.hip: the flat buffers, saved activations and scratch of the update step

struct Baseline {
  pnvo_baseline_config cfg;
  int device = 0;
  bool loaded = false;
  int C = 0;                         // input channels: rgb, then depth
  int oh[3] = {0, 0, 0}, ow[3] = {0, 0, 0};   // the three conv maps
  int F = 0;                         // 32 * oh[2] * ow[2]
  int E = 0;                         // embedding width in front of the goal: hidden, or 0 when blind
  int Kp = 0;                        // the GRU input row's pitch: E + goal_dim rounded up to a multiple of 4
  int nks = 0;                       // K slices of the Linear
  // kernel-layout operands, owned: conv weights [K][COUT], the Linear [hidden][F] with its columns in NHWC order, weight_ih_l0 at pitch Kp
  DevBuf<float> cw[3], fcw, w_ih;
  // tensors whose layout is torch's: views of the copies in `owned`, or — once a train step is attached — of the caller's flat buffer
  const float *cb[3] = {nullptr, nullptr, nullptr}, *fcb = nullptr;
  const float *w_hh = nullptr, *b_ih = nullptr, *b_hh = nullptr, *act_w = nullptr, *act_b = nullptr, *cr_w = nullptr, *cr_b = nullptr;
  std::vector<DevBuf<float>> owned;  // pnvo_baseline_load_weights' copies; empty once a train step is attached
  bool attached = false;             // pnvo_baseline_train_attach: the parameters live in the caller's flat buffer
  BaselineTrain *train = nullptr;
  // workspace, grown on demand
  int cap = 0;
  DevBuf<float> a1, a2, a3, part, x;
};

inline bool blind(const pnvo_baseline_config &c) { return c.rgb_channels + c.depth_channels == 0; }

// simple_cnn.hip
// the frames fit the handle (else PNVO_ERR_ARG, nothing launched)
int baseline_frames_check(const Baseline &p, const char *fn, const void *rgb, int rgb_is_u8, const float *depth, int B);
// frames -> a1, a2, a3 (the three maps, NHWC) -> part (the Linear's partial tiles [nks][B][hidden])
int baseline_encoder_launches(const Baseline &p, const void *rgb, int rgb_is_u8, const float *depth, int B, float *a1, float *a2, float *a3,
                              float *part, hipStream_t s);
// partial tiles + bias + ReLU -> x [B, Kp] = [embed | goal | zeros] and / or embed [B, hidden]
hipError_t baseline_sum_inputs(const Baseline &p, const float *part, const float *goal, int B, float *x, float *embed, hipStream_t s);
// simple_cnn_train.hip
void pnvo_baseline_train_free(Baseline &p);

// ---- the conv tile (conv_tile_kernel and the weight-gradient kernel of the update step)
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int KC = 64;         // k per LDS chunk
constexpr int LDA = KC + 4;    // row pitch of the activation tile: consecutive pixel rows start four banks apart

struct TileArgs {
  const void *rgb;             // conv1: [B,H,W,3] uint8 or float32
  const float *depth;          // conv1: [B,H,W,1]
  const float *in;             // conv2 / conv3: [B,H,W,CIN]
  const float *wt;             // [KH*KW*CIN][COUT]: k = (ky * KW + kx) * CIN + c
  const float *bias;           // [COUT]
  float *out;                  // [B,OH,OW,COUT]
  int M, H, W, OH, OW;         // M = B * OH * OW output pixels
};

#ifdef __HIPCC__
// pix[i] = (b * H + oy * S) * W + ox * S of the tile's BM output pixels m0 .. (past the end: the last pixel again)
template <int S>
__device__ __forceinline__ void tile_pixels(const TileArgs &a, int m0, int BM, int tid, int NT, unsigned *pix) {
  for (int i = tid; i < BM; i += NT) {
    const int m = min(m0 + i, a.M - 1);
    const int P = a.OH * a.OW, b = m / P, r = m - b * P, oy = r / a.OW, ox = r - oy * a.OW;
    pix[i] = ((unsigned)b * a.H + oy * S) * a.W + ox * S;
  }
}

// As[m * LDA + kk] = the conv's input at pixel pix[m], k = k0 + kk, for BM pixels and one 64-wide chunk of k.
// SRC 0: NHWC float activations (CIN % 4 == 0: float4 loads of four channels of one tap); 1 / 2: the sensor frames with float32 /
// uint8 rgb, CIN = NRGB + (depth ? 1 : 0) channels in the reference's torch.cat order, element loads (a pixel's taps of one kernel row
// are contiguous in memory); rgb is divided by 255 here.
template <int SRC, int NRGB, int CIN, int KW>
__device__ __forceinline__ void tile_load_a(const TileArgs &a, const unsigned *pix, int k0, int BM, int tid, int NT, float *As) {
  if constexpr (SRC == 0) {
    for (int g = tid; g < BM * (KC / 4); g += NT) {
      const int m = g / (KC / 4), q = g % (KC / 4), k = k0 + 4 * q, tap = k / CIN, c = k % CIN;
      const unsigned toff = (unsigned)(tap / KW) * a.W + tap % KW;
      *reinterpret_cast<f32x4 *>(&As[m * LDA + 4 * q]) = *reinterpret_cast<const f32x4 *>(a.in + (size_t)(pix[m] + toff) * CIN + c);
    }
  } else if constexpr (CIN == 4) {             // rgb-d: one tap of one pixel = (r, g, b) / 255 and the depth, stored as one float4
    for (int g = tid; g < BM * (KC / 4); g += NT) {
      const int m = g / (KC / 4), q = g % (KC / 4), tap = k0 / 4 + q;
      const size_t p = (size_t)pix[m] + (unsigned)(tap / KW) * a.W + tap % KW;
      f32x4 v;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        v[c] = (SRC == 2 ? (float)static_cast<const uint8_t *>(a.rgb)[p * 3 + c] : static_cast<const float *>(a.rgb)[p * 3 + c]) / 255.0f;
      v[3] = a.depth[p];
      *reinterpret_cast<f32x4 *>(&As[m * LDA + 4 * q]) = v;
    }
  } else {
    for (int g = tid; g < BM * KC; g += NT) {
      const int m = g / KC, kk = g % KC, k = k0 + kk, tap = k / CIN, c = k % CIN;
      const size_t p = (size_t)pix[m] + (unsigned)(tap / KW) * a.W + tap % KW;
      float v;
      if (c < NRGB)
        v = (SRC == 2 ? (float)static_cast<const uint8_t *>(a.rgb)[p * 3 + c] : static_cast<const float *>(a.rgb)[p * 3 + c]) / 255.0f;
      else
        v = a.depth[p];
      As[m * LDA + kk] = v;
    }
  }
}
#endif

}  // namespace pnvo

extern "C" {
struct pnvo_baseline_s {
  pnvo::Baseline p;
};
}
