// policy_train.hip — one PPO minibatch update of the navigation policy (rl/ppo/ppo.py:61-139 around Policy.evaluate_actions,
// rl/policies/policy.py:52-63), gfx950 only, float32.
//
//   evaluate : depth [T*N] -> avg_pool2d(2) (or, pnvo_policy_evaluate_rgbd: rgb / depth frames -> the input stage of pnvo_policy.hip, which
//              in training mode merges the T*N rows into RunningMeanAndVar's buffers first) -> the visual encoder's TRAIN-mode forward
//              (pnvo_train_forward: activations kept)
//              -> x = [visual | tgt_embeding | prev_action_embedding]                       policy_inputs_kernel, M = T*N rows
//              -> the recurrent layers (LSTM or GRU), the heads                              core_recurrent_forward, core_heads
//   ppo_loss : core_ppo_loss
//   backward : core_backward (heads, BPTT, the recurrent tensors' gradients, dX of layer 0) -> embeddings (inputs_bwd_kernel)
//              -> d visual into the encoder's backward below its output head.
// What sits between x and dX — the retained rollout, the recurrent and head kernels, the loss, the clipping, the phase timing — is
// ppo_core.hip's (pnvo_ppo_core.h), shared with the baseline policy's update step.  This file keeps what is this policy's: attach /
// refresh / reload, the three evaluate front ends, the embeddings' and the encoder's backward, the gradient-ready ranges.
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
#include "pnvo_ppo_core.h"

namespace pnvo {

struct PolicyTrain {
  PpoCore core;                       // flat buffers (n_named: the parameter table's floats; the rest is the tail below), retained rollout, scratch
  size_t o_stem = 0;                  // the policy's stem weight [C0,C,7,7] (the one tensor read here that is not a Policy slot)
  size_t o_stem2 = 0;                 // tail: the stem weight zero-padded to the encoder handle's 2C input channels [C0,2C,7,7],
  int c0 = 0, stem_row = 49;          //       then the handle's unused output head (hidden weights + 1 bias, zeros); stem_row = C * 49
  // the input side's workspace, sized for core.capM rows
  DevBuf<float> pooled, enc_out, x0, g3, dX0;
  DevBuf<int> rows;
  int cap_pooled = 0;                 // frames `pooled` holds: grown by the evaluate that takes depth only
  // the evaluate that takes visual_features: the feature rows [M, F] (kept: the caller's tensor may be gone by the backward) and
  // visual = relu(visual_fc(features)) [M, hidden]; from_features says which kind of evaluate came last
  DevBuf<float> feat, visual;
  int cap_feat = 0;
  bool from_features = false;
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

std::vector<RnnLayer> policy_layers(const Policy &p) {
  const int Hd = p.cfg.hidden;
  std::vector<RnnLayer> ls;
  for (int l = 0; l < p.cfg.rnn_layers; ++l) {
    const int K = l == 0 ? Hd + 64 : Hd;
    ls.push_back({p.w_ih[l], p.w_hh[l], p.b_ih[l], p.b_hh[l], K, K});
  }
  return ls;
}
Heads policy_heads(const Policy &p) { return {p.act_w, p.act_b, p.cr_w, p.cr_b}; }

// Before a regrow: the old workspace goes first (not old and new side by side), and a failed regrow leaves core.capM = 0.
void free_ws(PolicyTrain *t) {
  for (DevBuf<float> *b : {&t->pooled, &t->feat, &t->visual, &t->enc_out, &t->x0, &t->g3, &t->dX0}) b->reset();
  t->rows.reset();
  t->cap_pooled = t->cap_feat = 0;
  core_release(&t->core);
}

int ensure_ws(Policy &p, PolicyTrain *t, int M, int N) {
  if (M > t->core.capM) {
    free_ws(t);
    const size_t K0 = (size_t)p.cfg.hidden + 64, m = (size_t)M;
    PCHK(t->enc_out.alloc(m));
    PCHK(t->x0.alloc(m * K0));
    PCHK(t->g3.alloc(m * 3));
    PCHK(t->rows.alloc(m));
    PCHK(t->dX0.alloc(m * K0));
  }
  return core_reserve(&t->core, M, N);
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
  const int rc = pnvo_train_attach(p.enc, t->core.params, t->core.grads, t->core.n, etoc.data(), (int)etoc.size());
  if (rc != PNVO_OK) return pfail(rc, std::string("policy visual encoder: ") + pnvo_last_error(p.enc));
  return PNVO_OK;
}

size_t tail_floats(const pnvo_policy_config &c) { return (size_t)c.baseplanes * 98 * policy_channels(c) + (size_t)c.hidden + 1; }

}  // namespace

hipError_t launch_visual_fc_gemm(const float *feat, const float *w, const float *b, int rows, int F, int hidden, float *out, hipStream_t s) {
  GemmArgs g{feat, w, b, nullptr, out, rows, hidden, F, (long)F, 1, 1, (long)F, (long)hidden, 1};
  return launch_gemm_f32(g, true, true, s);
}

void pnvo_policy_train_free(Policy &p) {
  delete p.train;
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
    const int rc1 = core_init(&t->core, "pnvo_policy", p.device, params, grads, n_floats, n_named, c.hidden, c.rnn_layers, c.n_actions, is_gru(c));
    if (rc1 != PNVO_OK) return rc1;
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
                     t->core.params + t->o_stem, t->c0, t->stem_row, t->core.params + t->o_stem2);
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
  int rc = policy_encoder_table(p, toc, ntoc, t->core.n, &ent);
  if (rc != PNVO_OK) return rc;
  PCHK(hipStreamSynchronize((hipStream_t)stream));
  std::vector<float> host(t->core.n_named);
  PCHK(hipMemcpy(host.data(), t->core.params, t->core.n_named * sizeof(float), hipMemcpyDeviceToHost));
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
  if (obs)
    if (int rc0 = policy_obs_check(p, *obs, "pnvo_policy_evaluate_rgbd")) return rc0;
  const pnvo_policy_config &c = p.cfg;
  const void *vis = depth ? (const void *)depth : obs ? (const void *)obs : (const void *)vfeat;
  int rc = core_check_rollout("pnvo_policy_evaluate", T, N, {vis, goal, prev_actions, masks, actions}, hidden_in, hidden_out,
                              rnn_state_floats(c, N), is_gru(c) ? "rnn_layers * N * hidden" : "2 * rnn_layers * N * hidden");
  if (rc != PNVO_OK) return rc;
  const int M = T * N;
  PCHK(hipSetDevice(p.device));
  hipStream_t s = (hipStream_t)stream;
  if ((rc = ensure_ws(p, t, M, N)) != PNVO_OK) return rc;
  if ((rc = (depth || obs) ? ensure_pooled(p, t, M) : ensure_feat(p, t, M)) != PNVO_OK) return rc;
  t->from_features = vfeat != nullptr;
  if ((rc = core_keep(&t->core, T, N, masks, actions, hidden_in, s)) != PNVO_OK) return rc;
  const float *visual = nullptr;
  if (depth || obs) {
    PCHK(core_mark(&t->core, 0, s));
    // the M = T * N rows are ONE batch of RunningMeanAndVar (policy.py:52-63 runs the net once over the minibatch); the train-mode
    // forward takes the statistics over the handle's 2C channels, as the input stage padded them
    if ((rc = obs ? policy_input_stage(p, *obs, M, t->pooled, s) : pnvo_avgpool2(depth, M, c.height, c.width, t->pooled, stream)) != PNVO_OK)
      return rc;
    const bool norm = c.normalize != 0;
    rc = pnvo_train_forward(p.enc, nullptr, t->pooled, nullptr, nullptr, M, norm ? (const float *)p.mean_pad : nullptr,
                            norm ? (const float *)p.var_pad : nullptr, t->enc_out, stream);
    if (rc != PNVO_OK) return pfail(rc, std::string("policy visual encoder: ") + pnvo_last_error(p.enc));
    PCHK(core_mark(&t->core, 1, s));
    visual = pnvo_train_hidden(p.enc);
    if (!visual) return pfail(PNVO_ERR_STATE, "policy visual encoder kept no hidden vector");
  } else {                               // the encoder does not run: visual_fc on the caller's features, kept for dW = d visual^T . features
    PCHK(hipMemcpyAsync(t->feat, vfeat, (size_t)M * policy_feature_floats(p) * sizeof(float), hipMemcpyDeviceToDevice, s));
    PCHK(core_mark(&t->core, 0, s));
    if ((rc = launch_visual_fc(p, t->feat, M, t->visual, s)) != PNVO_OK) return rc;
    PCHK(core_mark(&t->core, 1, s));
    visual = t->visual;
  }
  PCHK(launch_policy_inputs(p, visual, goal, prev_actions, t->core.masks, M, t->x0, t->rows, t->g3, s));
  if ((rc = core_recurrent_forward(&t->core, policy_layers(p).data(), t->x0, false, hidden_out, s)) != PNVO_OK) return rc;
  return core_heads(&t->core, policy_heads(p), value, logp, entropy, s);
}

#define TRAIN_OR_FAIL(h)                                                                      \
  if (!(h) || !(h)->p.train) return pfail(PNVO_ERR_STATE, "pnvo_policy_train_attach first")

extern "C" {

int pnvo_policy_ppo_loss(pnvo_policy_handle h, const float *actions_logp_old, const float *adv, const float *value_preds,
                         const float *returns, float clip, float value_coef, float entropy_coef, int use_clipped_value_loss, float *out3,
                         void *stream) {
  TRAIN_OR_FAIL(h);
  return core_ppo_loss(&h->p.train->core, actions_logp_old, adv, value_preds, returns, clip, value_coef, entropy_coef, use_clipped_value_loss,
                       out3, (hipStream_t)stream);
}

int pnvo_policy_backward(pnvo_policy_handle h, int train_encoder, void *stream) {
  TRAIN_OR_FAIL(h);
  Policy &p = h->p;
  PolicyTrain *t = p.train;
  PpoCore *core = &t->core;
  int rc = core_backward_ready(core);
  if (rc != PNVO_OK) return rc;
  if (train_encoder && !policy_resnet18(p.cfg))
    return pfail(PNVO_ERR_STATE, "pnvo_policy_backward: a non-resnet18 encoder has no backward (RL.DDPPO.train_encoder: False)");
  PCHK(hipSetDevice(p.device));
  hipStream_t s = (hipStream_t)stream;
  const int Hd = p.cfg.hidden, A = p.cfg.n_actions, M = core->M;
  float *G = core->grads;
  PCHK(core_mark(core, 5, s));
  PCHK(hipMemsetAsync(G, 0, core->n * sizeof(float), s));              // overwrite semantics; a frozen encoder's range stays zero
  if ((rc = core_backward(core, policy_layers(p).data(), policy_heads(p), t->x0, t->dX0, s)) != PNVO_OK) return rc;
  // embeddings; d visual -> dY (contiguous [M, hidden]) -> the encoder's backward below its output head
  hipLaunchKernelGGL(inputs_bwd_kernel, dim3((unsigned)(((long)M * Hd + 128 + (long)(A + 1) * 32 + 255) / 256)), dim3(256), 0, s, t->dX0,
                     t->rows, t->g3, M, Hd, A + 1, grad_of(*core, p.tgt_w), grad_of(*core, p.tgt_b), grad_of(*core, p.emb), core->dY);
  PCHK(hipGetLastError());
  PCHK(core_mark(core, 6, s));
  report(t, t->r_early, s);             // embeddings, recurrent tensors, heads: final; they can travel while the encoder's backward runs
  if (t->from_features) {
    // visual_fc alone, whatever train_encoder says: nothing of the encoder ran, and no gradient is taken with respect to the features.
    // d visual (core->dY) through the ReLU, dW = d visual^T . features, db = colsum(d visual); the encoder's range stays at the memset's zeros
    const int F = (int)policy_feature_floats(p);
    hipLaunchKernelGGL(relu_mask_kernel, dim3((unsigned)(((long)M * Hd + 255) / 256)), dim3(256), 0, s, t->visual, (long)M * Hd, core->dY);
    PCHK(hipGetLastError());
    GemmArgs dw{core->dY, t->feat, nullptr, nullptr, grad_of(*core, p.vfc_w), Hd, F, M, 1, (long)Hd, (long)F, 1, (long)F};
    PCHK(launch_gemm_f32(dw, false, false, s));
    PCHK(launch_colsum(core->dY, M, Hd, Hd, grad_of(*core, p.vfc_b), s));
    report(t, t->r_vfc, s);
    PCHK(core_mark(core, 7, s));
    return PNVO_OK;
  }
  t->enc_pass = train_encoder ? 2 : 1;
  rc = pnvo_train_backward_from_hidden(p.enc, core->dY, train_encoder == 0, stream);
  t->enc_pass = 0;
  if (rc != PNVO_OK) return pfail(rc, std::string("policy visual encoder: ") + pnvo_last_error(p.enc));
  if (train_encoder) {
    hipLaunchKernelGGL(stem_unpad_kernel, dim3((unsigned)((t->c0 * t->stem_row + 255) / 256)), dim3(256), 0, s, G + t->o_stem2, t->c0, t->stem_row,
                       G + t->o_stem);
    PCHK(hipGetLastError());
    report(t, {{t->o_stem, t->o_stem + (size_t)t->c0 * t->stem_row}}, s);
  }
  PCHK(core_mark(core, 7, s));
  return PNVO_OK;
}

int pnvo_policy_train_timing(pnvo_policy_handle h, int mode) {
  TRAIN_OR_FAIL(h);
  return core_timing(&h->p.train->core, mode);
}

int pnvo_policy_train_timing_read(pnvo_policy_handle h, double ms[5]) {
  if (!h || !h->p.train || !ms) return pfail(PNVO_ERR_STATE, "pnvo_policy_train_attach first");
  return core_timing_read(&h->p.train->core, ms);
}

int pnvo_policy_clip_grad_norm(pnvo_policy_handle h, float max_norm, float *norm_out, void *stream) {
  TRAIN_OR_FAIL(h);
  if (!(max_norm > 0.f)) return pfail(PNVO_ERR_ARG, "max_grad_norm " + std::to_string(max_norm) + " must be > 0");
  return core_clip_grad_norm(&h->p.train->core, 1.f, max_norm, norm_out, (hipStream_t)stream);
}

int pnvo_policy_clip_grad_norm_scaled(pnvo_policy_handle h, float scale, float max_norm, float *norm_out, void *stream) {
  TRAIN_OR_FAIL(h);
  if (!std::isfinite(scale) || !(scale > 0.f)) return pfail(PNVO_ERR_ARG, "gradient scale " + std::to_string(scale) + " must be finite and > 0");
  if (std::isnan(max_norm)) return pfail(PNVO_ERR_ARG, "max_grad_norm is NaN");
  return core_clip_grad_norm(&h->p.train->core, scale, max_norm > 0.f ? max_norm : 0.f, norm_out, (hipStream_t)stream);
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
