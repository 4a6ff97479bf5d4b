// pnvo_policy_state.h — the navigation policy's handle, its parameter table and the small host helpers shared by its per-step forward
// (pnvo_policy.hip) and its PPO update step (policy_train.hip).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/pnvo.h"
#include "pnvo_model.h"

namespace pnvo {

struct PolicyTrain;                  // policy_train.hip: the flat buffers, saved activations and scratch of the update step

struct Policy {
  pnvo_policy_config cfg;
  int device = 0;
  pnvo_handle enc = nullptr;
  bool loaded = false;
  // device weights (torch layouts), listed once in policy_params(): views of the copies in `owned`, or — once a train step is
  // attached — of the caller's flat buffer
  float *emb = nullptr, *tgt_w = nullptr, *tgt_b = nullptr;
  std::vector<float *> w_ih, w_hh, b_ih, b_hh;       // one per recurrent layer
  float *act_w = nullptr, *act_b = nullptr, *cr_w = nullptr, *cr_b = nullptr;
  // net.visual_fc.1 in torch's own [hidden, F] layout (rows in the NCHW flatten's order): what the visual_features entry points read.
  // The depth path reads the encoder handle's channel-padded copy of the same two tensors.
  float *vfc_w = nullptr, *vfc_b = nullptr;
  std::vector<DevBuf<float>> owned;  // pnvo_policy_load_weights' copies, in policy_params() order; empty once a train step is attached
  bool attached = false;             // pnvo_policy_train_attach: the parameters live in the caller's flat buffer
  PolicyTrain *train = nullptr;
  // workspace
  int cap = 0, cap_pooled = 0;       // rows `visual` and `x` hold / frames `pooled` holds (only the entry points that take depth grow it)
  DevBuf<float> pooled, visual, x;
  DevBuf<float> feat;                // [cap_feat, F]: the encoder's output on its way to visual_fc (policy_visual_from_frames)
  int cap_feat = 0;
  // the input stage of the rgb / rgb-d / normalised handles (policy_input_stage): per-workgroup partial sums of the moments, the
  // moments [2C] (float64), and the statistics padded to the encoder handle's 2C channels (mean 0, variance 1 on the zero channels)
  DevBuf<double> in_part, m12;
  DevBuf<float> mean_pad, var_pad;
  // pnvo_policy_set_stats_hook: the cross-process reduction of the batch sums (stats_sums: the caller's 2C + 1 doubles, borrowed)
  pnvo_stats_reduce_fn stats_hook = nullptr;
  void *stats_user = nullptr;
  double *stats_sums = nullptr;
};

// ---- the visual input (pnvo_policy_config.rgb_channels / no_depth / normalize).  C channels in the reference's torch.cat order (rgb,
// then depth); the encoder handle takes ONE float modality of 2C channels: the C real ones, then C zero channels with zero weights.
inline int policy_channels(const pnvo_policy_config &c) { return c.rgb_channels + (c.no_depth ? 0 : 1); }
// today's depth-only, un-normalised policy: the 16-bit-matrix-core stem, the persistent small-batch encoder, the depth-only entry points
inline bool policy_is_plain(const pnvo_policy_config &c) { return c.rgb_channels == 0 && c.no_depth == 0 && c.normalize == 0; }
// RL.Policy.backbone other than resnet18 (pnvo_policy_config.backbone_depth / resnext / se): the encoder runs its inference forward only —
// frozen, never attached to the update step, evaluated from frames as encode + the visual_features path
inline bool policy_resnet18(const pnvo_policy_config &c) { return (c.backbone_depth == 0 || c.backbone_depth == 18) && !c.resnext && !c.se; }
inline size_t policy_pooled_floats(const pnvo_policy_config &c, int frames) {
  return (size_t)frames * (c.height / 2) * (c.width / 2) * 2 * policy_channels(c);
}
// One call's visual observations and the module's RunningMeanAndVar buffers (borrowed), as the *_rgbd entry points take them
struct PolicyObs {
  const void *rgb = nullptr;         // [B,H,W,3] uint8 or float32, values 0..255
  int rgb_is_u8 = 0;
  const float *depth = nullptr;      // [B,H,W,1]
  float *mean = nullptr, *var = nullptr, *count = nullptr;
  int training = 0;
};
// pnvo_policy.hip.  policy_obs_check: the pointers fit the handle's configuration (else PNVO_ERR_ARG, nothing launched).
// policy_input_stage: frames -> pooled [B,H/2,W/2,2C] (rgb / 255, avg_pool2d(2), zero channels); with normalize and o.training the
// batch is merged into the buffers; with normalize the padded statistics (Policy::mean_pad / var_pad) and the encoder stem's scale /
// shift pair are rewritten from the buffers.  All on `s`, no host synchronisation.
int policy_obs_check(const Policy &p, const PolicyObs &o, const char *fn);
int policy_input_stage(Policy &p, const PolicyObs &o, int B, float *pooled, hipStream_t s);

// ---- the policy-owned tensors (everything but the visual encoder, which lives in the encoder handle; visual_fc is held twice, here in
// torch's layout for the visual_features path and there channel-padded for the depth path), in state_dict order
struct PolicyParam {
  std::string name;
  std::vector<int64_t> shape;
  float **slot;                      // where Policy keeps the device pointer
  bool rows_as_float4;               // kernels read its rows as 16-byte vectors: the tensor must start at a multiple of 4 floats
};

// torch.nn.GRU keeps three gate blocks (r, z, n) per layer and one state tensor, torch.nn.LSTM four (i, f, g, o) and two (h, c)
inline bool is_gru(const pnvo_policy_config &c) { return c.rnn_type == PNVO_RNN_GRU; }
inline int rnn_gates(const pnvo_policy_config &c) { return is_gru(c) ? 3 : 4; }
// floats of hidden_in / hidden_out for `rows` environments
inline size_t rnn_state_floats(const pnvo_policy_config &c, int rows) {
  return (size_t)(is_gru(c) ? 1 : 2) * c.rnn_layers * rows * c.hidden;
}

// the visual encoder's output [C, fh, fw] (ResNetEncoder.output_shape, resnet_policy.py:113-124) and its flattened size F
void policy_features_shape(const Policy &p, int64_t shape[3]);       // pnvo_policy.hip
inline int64_t policy_feature_floats(const Policy &p) {
  int64_t s[3];
  policy_features_shape(p, s);
  return s[0] * s[1] * s[2];
}

inline std::vector<PolicyParam> policy_params(Policy &p) {
  const int64_t Hd = p.cfg.hidden, A = p.cfg.n_actions, G = rnn_gates(p.cfg);
  std::vector<PolicyParam> t = {{"net.prev_action_embedding.weight", {A + 1, 32}, &p.emb, false},
                                {"net.tgt_embeding.weight", {32, 3}, &p.tgt_w, false},
                                {"net.tgt_embeding.bias", {32}, &p.tgt_b, false}};
  const int64_t F = policy_feature_floats(p);
  t.push_back({"net.visual_fc.1.weight", {Hd, F}, &p.vfc_w, false});       // (F % 4 != 0 on some frame sizes: rows are not 16-byte aligned)
  t.push_back({"net.visual_fc.1.bias", {Hd}, &p.vfc_b, false});
  for (int l = 0; l < p.cfg.rnn_layers; ++l) {
    const std::string r = "net.state_encoder.rnn.", sl = "_l" + std::to_string(l);
    t.push_back({r + "weight_ih" + sl, {G * Hd, l == 0 ? Hd + 64 : Hd}, &p.w_ih[l], true});
    t.push_back({r + "weight_hh" + sl, {G * Hd, Hd}, &p.w_hh[l], true});
    t.push_back({r + "bias_ih" + sl, {G * Hd}, &p.b_ih[l], false});
    t.push_back({r + "bias_hh" + sl, {G * Hd}, &p.b_hh[l], false});
  }
  t.push_back({"action_distribution.linear.weight", {A, Hd}, &p.act_w, true});
  t.push_back({"action_distribution.linear.bias", {A}, &p.act_b, false});
  t.push_back({"critic.fc.weight", {1, Hd}, &p.cr_w, true});
  t.push_back({"critic.fc.bias", {1}, &p.cr_b, false});
  return t;
}

inline size_t numel(const std::vector<int64_t> &shape) {
  size_t n = 1;
  for (int64_t s : shape) n *= (size_t)s;
  return n;
}

// ---- the encoder handle's table, from the caller's: the VO model's names (net.visual_encoder.* -> visual_encoder.*, net.visual_fc.1.*
// -> visual_fc.2.*), the stem widened to the handle's two input channels [C0,2,7,7], and the handle's unused output head
struct EncoderEntry {
  enum Source { VIEW, STEM, ZEROS };  // entry k of the caller's table as it is / that entry [C0,C,7,7] zero-padded to 2C input channels / all zeros
  std::string name;
  std::vector<int64_t> shape;
  Source src;
  int k;
};
// pnvo_policy.hip; also checks the rank and the range (offset + numel <= n_floats) of EVERY entry of the caller's table
int policy_encoder_table(const Policy &p, const pnvo_tensor_desc *toc, int ntoc, size_t n_floats, std::vector<EncoderEntry> *out);
// the descriptors pnvo_load_weights / pnvo_train_attach take, with entry i at offsets[i] (the names point into `entries`)
std::vector<pnvo_tensor_desc> encoder_toc(const std::vector<EncoderEntry> &entries, const std::vector<size_t> &offsets);
// entry `e` of the parameter table in the caller's toc, with its full shape and range checked; nullptr with *rc set otherwise
const pnvo_tensor_desc *policy_find(const pnvo_tensor_desc *toc, int ntoc, const PolicyParam &e, size_t n_floats, int *rc);

void pnvo_policy_train_free(Policy &p);       // policy_train.hip
// pnvo_policy.hip: x [rows, hidden + 64] = visual | tgt_embeding(goal) | prev_action_embedding; rows_out / g3 (optional, the update step's)
// keep the gathered embedding row and (rho, cos(-phi), sin(-phi)) per row
hipError_t launch_policy_inputs(const Policy &p, const float *visual, const float *goal, const int64_t *prev, const float *masks, int rows,
                                float *x, int *rows_out, float *g3, hipStream_t s);
// out [rows, hidden] = relu(feat [rows, F] . vfc_w^T + vfc_b): the row kernel of pnvo_policy.hip up to VFC_ROWS_MAX rows, the float32
// matrix-core GEMM of ppo_core.hip above
constexpr int VFC_ROWS_MAX = 48;
int launch_visual_fc(const Policy &p, const float *feat, int rows, float *out, hipStream_t s);
hipError_t launch_visual_fc_gemm(const float *feat, const float *w, const float *b, int rows, int F, int hidden, float *out, hipStream_t s);   // policy_train.hip
// the recurrent layers and the heads of one act step on x [B, hidden + 64] (pnvo_policy.hip)
int policy_act_tail(Policy &p, const float *masks, const float *hidden_in, int B, float *hidden_out, float *features, float *logits,
                    float *value, hipStream_t s);

// one GRU layer (x [B, K], K % 4 == 0, rows 16-byte aligned; w_ih [3 Hd, K]) and the two heads, as policy_act_tail launches them: the
// baseline policy's handle (simple_cnn.hip) runs the same kernels (pnvo_policy.hip)
hipError_t launch_gru_layer(const float *x, int K, const float *w_ih, const float *b_ih, const float *h_prev, const float *w_hh,
                            const float *b_hh, const float *masks, int B, int Hd, float *h_out, hipStream_t s);
hipError_t launch_policy_heads(const float *feat, const float *act_w, const float *act_b, const float *cr_w, const float *cr_b, int B, int Hd,
                               int n_actions, float *logits, float *value, hipStream_t s);

// ---- host helpers of both files
inline int pfail(int code, const std::string &msg) { return pnvo_fail(nullptr, code, msg); }

#define PCHK(expr)                                                                              \
  do {                                                                                          \
    hipError_t e__ = (expr);                                                                    \
    if (e__ != hipSuccess) return pfail(PNVO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
  } while (0)

// The recurrent kernels write h_out / c_out rows while other workgroups still read h_prev / c_prev: the two states must not share memory.
inline bool hidden_states_overlap(const float *in, const float *out, size_t floats) {
  const uintptr_t bytes = (uintptr_t)floats * sizeof(float), a = (uintptr_t)in, b = (uintptr_t)out;
  return a < b + bytes && b < a + bytes;
}

}  // namespace pnvo

extern "C" {
struct pnvo_policy_s {
  pnvo::Policy p;
};
}
