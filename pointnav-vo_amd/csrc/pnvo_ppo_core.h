// pnvo_ppo_core.h — the part of one PPO minibatch update that both navigation policies run (ppo_core.hip): everything between "the
// recurrent core's input rows exist" and "the gradient at those rows exists".  PolicyTrain (policy_train.hip) and BaselineTrain
// (simple_cnn_train.hip) each embed one PpoCore and keep only their own encoder's side of the step.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <vector>

#include "dev_buf.h"

namespace pnvo {

// C[m][n] = sum_k A(m,k) B(k,n) (+ bias0[n] + bias1[n]) on the exact-float32 matrix instruction; both operands addressed by two strides
struct GemmArgs {
  const float *A, *B, *bias0, *bias1;
  float *C;
  int M, N, K;
  long a_sm, a_sk, b_sk, b_sn, ldc;
  int relu = 0;                       // epilogue: max(., 0) behind the bias
};
// akc / bkc: k is the contiguous index of A / B in memory (else m / n): picks the staging order that reads whole lines
hipError_t launch_gemm_f32(const GemmArgs &g, bool akc, bool bkc, hipStream_t s);
hipError_t launch_transpose(const float *src, int R, int C, float *dst, hipStream_t s);       // dst [C][R] = src [R][C]^T

// One recurrent layer as the update step reads it: torch's tensors in the caller's flat parameter buffer (each gradient sits at the
// same offset of the flat gradient buffer), and the layer's input rows [M][K] at pitch ldx.
struct RnnLayer {
  const float *w_ih, *w_hh, *b_ih, *b_hh;       // [G*H][K], [G*H][H], [G*H], [G*H];  G = 3 (GRU: r, z, n) or 4 (LSTM: i, f, g, o)
  int K, ldx;
};
struct Heads {
  const float *act_w, *act_b, *cr_w, *cr_b;     // in the flat parameter buffer
};

struct PpoCore {
  const char *abi = "";               // "pnvo_policy" / "pnvo_baseline": names the entry points in the refusals
  int device = 0;
  float *params = nullptr, *grads = nullptr;   // the caller's flat buffers (not owned)
  size_t n = 0, n_named = 0;          // floats handed over / floats covered by the parameter table
  int Hd = 0, L = 0, A = 0;           // hidden size, recurrent layers, actions
  bool gru = false;
  // the last evaluate
  int T = 0, N = 0, M = 0;
  bool have_loss = false;
  // workspace, sized for capM rows: what the backward reads of the rollout, the heads' outputs, the gradients' scratch
  int capM = 0;
  DevBuf<float> masks, hid0;
  DevBuf<int64_t> actions;
  std::vector<DevBuf<float>> gates, c, y, hm;      // per layer: [M, 4H] gate rows, c[t] (LSTM only), y = h[t], hm = h[t-1] * mask[t]
  DevBuf<float> logits, value, logp, ent, dlogits, dvalue;
  DevBuf<float> dY, dG, dH, whhT;     // dH: d h[t] per row (LSTM: d c[t])
  DevBuf<float> dGh;                  // GRU only: the recurrent side's gate gradients [M, 3H] (dG holds the input side's)
  DevBuf<double> sq_part;             // clip_grad_norm partial sums
  // core_timing: events at the phase boundaries of evaluate / ppo_loss / backward (tools/bench_ppo_update.py)
  bool timing = false;
  hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  ~PpoCore();
};

// the gradient of a tensor of the flat parameter buffer
inline float *grad_of(const PpoCore &c, const float *p) { return c.grads + (p - c.params); }
// floats of hidden_in / hidden_out for N environments: h per layer, and c behind them for an LSTM
inline size_t core_state_floats(const PpoCore &c, int N) { return (size_t)(c.gru ? 1 : 2) * c.L * N * c.Hd; }

// Every function returns PNVO_OK or fails through pnvo_fail (the message names the entry point through `abi` / `fn`).
int core_init(PpoCore *c, const char *abi, int device, float *params, float *grads, size_t n, size_t n_named, int Hd, int L, int A, bool gru);
// The rollout's shape, null pointers (`ptrs` and the two states), the states' 16-byte alignment and their overlap; `state_desc` says
// what each state holds ("N * hidden").  Nothing is launched.
int core_check_rollout(const char *fn, int T, int N, std::initializer_list<const void *> ptrs, const float *hidden_in,
                       const float *hidden_out, size_t state_floats, const char *state_desc);
// The workspace for M = T * N rows.  A regrow frees the old one first (core_release: the embedding struct frees its own buffers with it
// and allocates them BEFORE this call), and a failed regrow leaves capM = 0.
int core_reserve(PpoCore *c, int M, int N);
void core_release(PpoCore *c);
// records T / N and keeps what the backward reads later (the caller's tensors may be gone by then)
int core_keep(PpoCore *c, int T, int N, const float *masks, const int64_t *actions, const float *hidden_in, hipStream_t s);
// Per layer: G_x = X . W_ih^T + bias over all M rows, then T step launches.  x0: layer 0's rows (layers[0].K columns at pitch ldx).
// gx0_done: the caller has filled blocks 0 .. 2 of gates[0] with layer 0's G_x itself.
int core_recurrent_forward(PpoCore *c, const RnnLayer *layers, const float *x0, bool gx0_done, float *hidden_out, hipStream_t s);
// logits / value / log pi(a) / entropy per row from the top layer's rows; value, logp [M] and entropy [1] are optional outputs.  Mark 2.
int core_heads(PpoCore *c, const Heads &h, float *value, float *logp, float *entropy, hipStream_t s);
int core_ppo_loss(PpoCore *c, const float *actions_logp_old, const float *adv, const float *value_preds, const float *returns, float clip,
                  float value_coef, float entropy_coef, int use_clipped_value_loss, float *out3, hipStream_t s);
// "<abi>_backward before <abi>_evaluate + <abi>_ppo_loss" unless both have run
int core_backward_ready(const PpoCore *c);
// Heads, then per layer from the top: BPTT, dW_ih, dW_hh, the bias gradients, dX (into dY for the layer below, into dX0 [M][K] for
// layer 0; dX0 == nullptr: not taken).  Gradients land in the flat gradient buffer, which the caller has cleared as it sees fit.
int core_backward(PpoCore *c, const RnnLayer *layers, const Heads &h, const float *x0, float *dX0, hipStream_t s);
// nn.utils.clip_grad_norm_ over the n_named floats of scale * grads (max_norm <= 0: scale only)
int core_clip_grad_norm(PpoCore *c, float scale, float max_norm, float *norm_out, hipStream_t s);
int core_timing(PpoCore *c, int mode);
int core_timing_read(PpoCore *c, double ms[5]);
// phase boundary k of the update step (only while timing is on)
inline hipError_t core_mark(PpoCore *c, int k, hipStream_t s) { return c->timing ? hipEventRecord(c->ev[k], s) : hipSuccess; }

}  // namespace pnvo
