// pnvo_train_api.hip — C ABI of the VO training step (BASELINE config 4): forward in train mode with
// saved activations, backward through the whole network, and the optimiser/loss helpers.  Replaces, for one action
// model, the body of the reference's training iteration
//   optimizer.zero_grad(); out = vo_model(batch_pairs); loss = sum_d mse_d; loss.backward(); optimizer.step()
// (/root/reference/pointnav_vo/vo/engine/vo_cnn_regression_geo_invariance_engine.py:855-901, :586; loss
//  vo_cnn_engine.py:135-198; Adam :122-133).  The flat parameter / gradient buffers are caller-owned device memory in
// the reference's state_dict parameter order, so the data-parallel all-reduce is ONE collective on one buffer.
//
// pnvo_train_attach resolves every parameter name to its flat offset ONCE (TrainLayer, TrainLinear) and builds every table that
// never changes afterwards; the refresh, the forward and the backward only read those records and launch.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <utility>

#include "pnvo_model.h"

using namespace pnvo;

namespace {

struct PackMap {
  float *dst;             // an operand buffer of the handle (not owned)
  DevBuf<int> map;
};

struct ConvSave {
  DevBuf<float> raw;
  DevPair<float> ss;
  DevBuf<float> mu, rstd;
};

// the caller's parameter table by name: a local of pnvo_train_attach (run-time code reads the records below)
struct TocEnt {
  size_t off;
  std::vector<int64_t> shape;
  size_t numel;
};
using Toc = std::map<std::string, TocEnt>;

struct Param {                // a parameter inside the flat buffers
  size_t off = 0, numel = 0;
};
struct Weight : Param {
  std::string t_wgrad;        // its timing entry: "wgrad:<name>"
};

// What pnvo_train_attach bound for conv li of m->convs.
struct TrainLayer {
  Weight w;
  Param gamma, beta;          // the GroupNorm behind it
  int x2_row = -1;            // row of TrainState::x2_scale, or -1 (stem, Bottleneck models)
  std::string t_dgrad;        // timing entry "dgrad:<name>"
  // backward-data operands (none for the stem: no input gradient)
  DevBuf<float> dgrad_w;                       // flipped / transposed weights, re-packed by the gather of every refresh
  std::array<DevBuf<float>, 4> dgrad_wph;      // stride-2 3x3 convs: one sub-kernel per output parity phase (ph*2 + pw)
  DevBuf<unsigned short> dgrad_x[2];           // 3x3 stride-1 convs on conv_x3.hip: [0] two float16 pieces (option train_pieces = 2),
  unsigned long long dgrad_x_gen[2] = {0, 0};  //   [1] three bf16 pieces; built from the flat parameters when m->weights_gen moved
};
struct TrainLinear {
  Weight w;
  Param b;
};

// everything sized for TrainState::capB: saved activations of the last forward and the backward's scratch
struct TrainWs {
  std::vector<ConvSave> cs;
  std::vector<DevBuf<float>> y;     // y[0] = pooled stem output, y[k] = output of residual block k
  DevBuf<unsigned char> pool_idx;
  DevBuf<float> hid;
  DevBuf<float> dYa, dYb, G, dRaw, dA, dStem;
  DevBuf<float> dout8, dh, gh, dz;
  DevBuf<float> gn_part, gn_coef, wg_partial;
  DevBuf<double> mom_part;
  DevBuf<float> zdrop, hdrop, dmask;          // dropped activations of the last forward
  DevBuf<float> egath, efeat, biasB, dfeat;   // action embedding: gathered rows, dropped rows, per-sample bias rows, gradient
  DevBuf<int64_t> iota;
};

struct TrainState {
  float *params = nullptr, *grads = nullptr;   // the caller's flat buffers (not owned)
  size_t n = 0;
  std::vector<TrainLayer> conv;     // index-aligned with m->convs
  TrainLinear fc, head;
  size_t emb_off = 0;               // action_embedding.weight (act_embed models)
  long w1_pitch = 0;                // columns of the hidden layer's weight: flat (+ 32 embedding columns)
  size_t stem_w_off = 0;            // offset of the OIHW stem weight in the flat parameter buffer
  std::vector<PackMap> maps;
  DevBuf<unsigned> dmax;            // per conv: float bits of max |dRaw| of the backward in flight (gn_bwd_apply)
  DevBuf<float> fc_t, head_t;
  DevBuf<int> d_ref_of_new, d_tensor_of_new, d_ciperm;
  DevBuf<GatherSeg> d_segs;         // all re-pack maps as one segment table
  long seg_total = 0;
  int nseg = 0;
  DevBuf<int> d_mxmaps;             // mx stem: [slot_ref 32 | slot_new 32 | xslot 4]
  DevBuf<int> d_ddmaps;             // one-hot stem: [dense_ref 12 | dense_new 12 | dd_ref 2*bins | dd_new 2*bins]
  int dd_nd = 0;
  int capB = 0;
  int lastB = 0;
  TrainWs ws;
  const float *src[4] = {nullptr, nullptr, nullptr, nullptr};   // observation tensors of the last forward
  // ... or, from_frames (pnvo_train_forward_raw on the frame-reading kernels), its sensor frames: src[3] is the top-down pair tensor,
  // src[0..2] are null and the stem's weight gradient reads the frames with the same bin edges
  bool from_frames = false;
  const unsigned char *f_rgb = nullptr;
  const float *f_depth = nullptr;
  float f_edges[12] = {0};
  // ... or, where those kernels do not serve the handle, the pairs materialised from them (kept until the backward has read them)
  DevBuf<float> fpairs[3];
  int fpairs_cap = 0;
  // dropout (pnvo_train_set_dropout): p, seed, forward counter
  float drop_p = 0.f;
  uint64_t drop_seed = 0, drop_step = 0;
  // action-embedding variants: the Linear's 32 embedding columns as per-sample bias rows (train_kernels.hip embed_*)
  const long long *actions = nullptr;   // device [B], set by pnvo_train_set_actions for the next forward/backward
  DevBuf<int> embed_err;                // host-mapped flag: action outside the embedding table
  // gradient-ready hook (pnvo_train_set_grad_hook): the backward reports flat ranges [first, first + count) whose gradients
  // are final while the rest of it is still being enqueued; bucket_first = lower bounds of the ranges, latest layers first
  pnvo_grad_ready_fn hook = nullptr;
  void *hook_user = nullptr;
  std::vector<size_t> bucket_first;     // e.g. {offset of layer4's first parameter, offset of layer2's, 0}
  std::vector<char> bucket_done;        // per backward: which ranges have been reported (the end of the backward reports the rest)
  // two-piece float16 operands of the training forward's convs: per conv weight {scale, 1/scale}, recomputed from the flat
  // parameters by ONE launch per pnvo_train_refresh (conv_x3.hip conv_x2_scale_kernel)
  int x2_rows = 0;
  DevBuf<long> x2_seg;                  // [rows][2]: flat offset, element count
  DevBuf<float> x2_scale;               // [rows][2]
  // GroupNorm bounds behind Layer::in_bound (the range guard of the float16 pieces), tracked while gamma / beta move: one small
  // launch per pnvo_train_refresh writes max_c (|gamma_c| sqrt(N) + |beta_c|) per conv into host-mapped memory; the next training
  // forward chains them into in_bound without a synchronisation (a value may lag one optimiser step: a step moves gamma by <= lr)
  struct GnbSeg { long goff, boff; int c; float rootn; };
  DevBuf<GnbSeg> gnb_seg;               // [convs]
  DevBuf<float> gnb_host;               // host-mapped [3][convs]: the bounds of the last three refreshes (ring); < 0: not computed yet
  hipEvent_t gnb_ev[3] = {nullptr, nullptr, nullptr};   // behind the gn_bound_kernel of each ring entry
  long gnb_refreshes = 0;               // refreshes issued so far: entry (r % 3) holds refresh r
  int gnb_n = 0;
};

TrainState *TS(pnvo_handle m) { return reinterpret_cast<TrainState *>(m->train); }

const std::string T_GN_BWD = "gn_bwd";

// index of l in m->convs, or -1 (m->fc, m->head, a layer of another handle)
long conv_index(pnvo_handle m, const Layer &l) {
  const Layer *first = m->convs.data();
  return std::less_equal<const Layer *>()(first, &l) && std::less<const Layer *>()(&l, first + m->convs.size()) ? &l - first : -1;
}

// ---- pnvo_train_attach: names -> records, re-pack maps, tables ------------------------------------------------------------

// float "index tensor" of a parameter: value = flat offset + 1 (exact in fp32 below 2^24 elements)
std::vector<float> index_tensor(const TocEnt &e) {
  std::vector<float> v(e.numel);
  for (size_t i = 0; i < e.numel; ++i) v[i] = (float)(e.off + i + 1);
  return v;
}

int add_map(pnvo_handle m, TrainState *t, float *dst, const std::vector<float> &packed_idx) {
  std::vector<int> mp(packed_idx.size());
  for (size_t i = 0; i < mp.size(); ++i) mp[i] = (int)packed_idx[i];
  PackMap pm;
  pm.dst = dst;
  HIPCHK(m, pm.map.upload(mp.data(), mp.size()));
  t->maps.push_back(std::move(pm));
  return PNVO_OK;
}

const TocEnt *need(pnvo_handle m, const Toc &toc, const std::string &name, int *rc) {
  auto it = toc.find(name);
  if (it == toc.end()) {
    *rc = pnvo_fail(m, PNVO_ERR_WEIGHTS, "parameter table is missing '" + name + "'");
    return nullptr;
  }
  return &it->second;
}

// OIHW [cout][cin][K][K] -> backward-data weights [cin][cout][K][K], taps flipped
std::vector<float> transpose_flip(const std::vector<float> &w, int cout, int cin, int kh, int kw) {
  std::vector<float> o((size_t)cin * cout * kh * kw);
  for (int co = 0; co < cout; ++co)
    for (int ci = 0; ci < cin; ++ci)
      for (int a = 0; a < kh; ++a)
        for (int b = 0; b < kw; ++b)
          o[(((size_t)ci * cout + co) * kh + a) * kw + b] = w[(((size_t)co * cin + ci) * kh + (kh - 1 - a)) * kw + (kw - 1 - b)];
  return o;
}

// the stem's forward operands: channel order of the fused gather (pnvo_load_weights does the same permutation)
int map_stem_weight(pnvo_handle m, TrainState *t, const std::vector<float> &idx) {
  const Layer &l = m->convs[0];
  const int T = l.k * l.kw;
  int rc = PNVO_OK;
  std::vector<float> wp((size_t)l.cout * m->CP * T, 0.f), pk;
  for (int nc = 0; nc < m->CP; ++nc) {
    const int r = m->stem_ref_of_new[nc];
    if (r < 0) continue;
    for (int o = 0; o < l.cout; ++o)
      std::memcpy(&wp[((size_t)o * m->CP + nc) * T], &idx[((size_t)o * l.cin + r) * T], sizeof(float) * T);
  }
  pnvo_pack_conv_weight_cinp(wp.data(), l.cout, m->CP, m->CP, l.k, l.kw, pk);
  if ((rc = add_map(m, t, l.wpk, pk)) != PNVO_OK) return rc;
  std::vector<float> pk16((size_t)49 * m->CPL * l.cout);
  pack_stem_weight(wp.data(), l.cout, m->CP, m->CPL, pk16.data());
  return add_map(m, t, m->stem_wpk16, pk16);
}

// conv li's forward operand and its backward-data operands: "conv" with CIN' = coutp (gradient channels), COUT' = cin
int map_conv_weight(pnvo_handle m, TrainState *t, size_t li, const std::vector<float> &idx) {
  const Layer &l = m->convs[li];
  TrainLayer &tl = t->conv[li];
  int rc = PNVO_OK;
  std::vector<float> pk;
  pnvo_pack_conv_weight_cinp(idx.data(), l.cout, l.cin, l.cinp, l.k, l.kw, pk);
  if ((rc = add_map(m, t, l.wpk, pk)) != PNVO_OK) return rc;
  const std::vector<float> wt = transpose_flip(idx, l.cout, l.cin, l.k, l.kw);
  pnvo_pack_conv_weight_cinp(wt.data(), l.cin, l.cout, l.coutp, l.k, l.kw, pk);
  HIPCHK(m, tl.dgrad_w.alloc(pk.size()));
  if ((rc = add_map(m, t, tl.dgrad_w, pk)) != PNVO_OK) return rc;
  if (!(l.stride == 2 && l.k == 3 && l.kw == 3 && l.pad == 1)) return PNVO_OK;
  // dX[2i+ph] = sum over the taps whose source row (2i+ph-1+kh)/2 is an integer: kh = 1 (ph = 0) or kh = 0, 2
  // (ph = 1), reading dY rows i, or i and i+1 — a 1- or 2-tap stride-1 conv per parity phase, no masked taps
  for (int ph = 0; ph < 2; ++ph)
    for (int pw = 0; pw < 2; ++pw) {
      const int th[2] = {ph ? 0 : 1, 2}, tw[2] = {pw ? 0 : 1, 2};
      const int nh = ph ? 2 : 1, nw = pw ? 2 : 1;
      std::vector<float> sub((size_t)l.cin * l.cout * nh * nw);
      for (int ci = 0; ci < l.cin; ++ci)
        for (int co = 0; co < l.cout; ++co)
          for (int a = 0; a < nh; ++a)
            for (int b = 0; b < nw; ++b)
              sub[(((size_t)ci * l.cout + co) * nh + a) * nw + b] = wt[(((size_t)ci * l.cout + co) * 3 + th[a]) * 3 + tw[b]];
      pnvo_pack_conv_weight_cinp(sub.data(), l.cin, l.cout, l.coutp, nh, nw, pk);
      DevBuf<float> &dst = tl.dgrad_wph[ph * 2 + pw];
      HIPCHK(m, dst.alloc(pk.size()));
      if ((rc = add_map(m, t, dst, pk)) != PNVO_OK) return rc;
    }
  return PNVO_OK;
}

int bind_convs(pnvo_handle m, TrainState *t, const Toc &toc) {
  int rc = PNVO_OK;
  t->conv.resize(m->convs.size());
  for (size_t li = 0; li < m->convs.size(); ++li) {
    const Layer &l = m->convs[li];
    TrainLayer &tl = t->conv[li];
    const TocEnt *w = need(m, toc, l.name + ".weight", &rc);
    if (!w) return rc;
    tl.w.off = w->off;
    tl.w.numel = w->numel;
    tl.w.t_wgrad = "wgrad:" + l.name + ".weight";
    tl.t_dgrad = "dgrad:" + l.name;
    if (li == 0) t->stem_w_off = w->off;
    if ((rc = li == 0 ? map_stem_weight(m, t, index_tensor(*w)) : map_conv_weight(m, t, li, index_tensor(*w))) != PNVO_OK) return rc;
    const TocEnt *g = need(m, toc, l.gn + ".weight", &rc);
    if (!g) return rc;
    const TocEnt *b = need(m, toc, l.gn + ".bias", &rc);
    if (!b) return rc;
    tl.gamma = Param{g->off, g->numel};
    tl.beta = Param{b->off, b->numel};
    if ((rc = add_map(m, t, l.gamma, index_tensor(*g))) != PNVO_OK) return rc;
    if ((rc = add_map(m, t, l.beta, index_tensor(*b))) != PNVO_OK) return rc;
  }
  return PNVO_OK;
}

int bind_linears(pnvo_handle m, TrainState *t, const Toc &toc) {
  int rc = PNVO_OK;
  const pnvo_config &c = m->cfg;
  const int T = m->fh * m->fw, flat = m->comp_c * T;
  const TocEnt *w1 = need(m, toc, m->fc.name + ".weight", &rc);
  if (!w1) return rc;
  const TocEnt *b1 = need(m, toc, m->fc.name + ".bias", &rc);
  if (!b1) return rc;
  const TocEnt *w2 = need(m, toc, m->head.name + ".weight", &rc);
  if (!w2) return rc;
  const TocEnt *b2 = need(m, toc, m->head.name + ".bias", &rc);
  if (!b2) return rc;
  const int fc_in = flat + (c.act_embed ? 32 : 0);
  if ((int)w1->shape[1] != fc_in) return pnvo_fail(m, PNVO_ERR_ARG, m->fc.name + ".weight has the wrong number of columns");
  t->fc = TrainLinear{{{w1->off, w1->numel}, "wgrad:" + m->fc.name + ".weight"}, {b1->off, b1->numel}};
  t->head = TrainLinear{{{w2->off, w2->numel}, "wgrad:" + m->head.name + ".weight"}, {b2->off, b2->numel}};
  t->w1_pitch = fc_in;
  if (c.act_embed) {
    const TocEnt *emb = need(m, toc, "action_embedding.weight", &rc);
    if (!emb) return rc;
    if (emb->shape.size() != 2 || emb->shape[0] != c.n_acts + 1 || emb->shape[1] != 32)
      return pnvo_fail(m, PNVO_ERR_ARG, "action_embedding.weight must be [n_acts + 1, 32]");
    t->emb_off = emb->off;
    HIPCHK(m, t->embed_err.alloc_host(1, hipHostMallocMapped));
    *t->embed_err = 0;
  }
  const std::vector<float> i1full = index_tensor(*w1), i2 = index_tensor(*w2);
  std::vector<float> i1((size_t)c.hidden * flat);          // the visual columns
  for (int o = 0; o < c.hidden; ++o)
    std::memcpy(&i1[(size_t)o * flat], &i1full[(size_t)o * fc_in], sizeof(float) * (size_t)flat);
  std::vector<float> pk;
  pnvo_pack_conv_weight_cinp(i1.data(), c.hidden, m->comp_c, m->comp_cp, m->fh, m->fw, pk);
  if ((rc = add_map(m, t, m->fc.wpk, pk)) != PNVO_OK) return rc;
  if (!c.act_embed)        // act-embed: the per-action bias rows are rebuilt by pnvo_train_refresh
    if ((rc = add_map(m, t, m->fc_bias, index_tensor(*b1))) != PNVO_OK) return rc;
  pnvo_pack_conv_weight_cinp(i2.data(), c.out_dim, c.hidden, c.hidden, 1, 1, pk);
  if ((rc = add_map(m, t, m->head.wpk, pk)) != PNVO_OK) return rc;
  if ((rc = add_map(m, t, m->head_bias, index_tensor(*b2))) != PNVO_OK) return rc;
  // dz = g_h . W1 as a 1x1 conv: CIN' = hidden, COUT' = T*comp_cp, W'[tap*comp_cp + ch][o] = W1[o][ch*T + tap]
  std::vector<float> wt((size_t)T * m->comp_cp * c.hidden, 0.f);
  for (int o = 0; o < c.hidden; ++o)
    for (int ch = 0; ch < m->comp_c; ++ch)
      for (int tap = 0; tap < T; ++tap)
        wt[((size_t)tap * m->comp_cp + ch) * c.hidden + o] = i1[(size_t)o * flat + (size_t)ch * T + tap];
  pnvo_pack_conv_weight_cinp(wt.data(), T * m->comp_cp, c.hidden, c.hidden, 1, 1, pk);
  HIPCHK(m, t->fc_t.alloc(pk.size()));
  if ((rc = add_map(m, t, t->fc_t, pk)) != PNVO_OK) return rc;
  // dh = dOut . W2: CIN' = 8 (out_dim padded), COUT' = hidden, W'[o][d] = W2[d][o]
  std::vector<float> ht((size_t)c.hidden * c.out_dim);
  for (int o = 0; o < c.hidden; ++o)
    for (int d = 0; d < c.out_dim; ++d) ht[(size_t)o * c.out_dim + d] = i2[(size_t)d * c.hidden + o];
  pnvo_pack_conv_weight_cinp(ht.data(), c.hidden, c.out_dim, rup(c.out_dim, 8), 1, 1, pk);
  HIPCHK(m, t->head_t.alloc(pk.size()));
  return add_map(m, t, t->head_t, pk);
}

// stem channel tables on the device, and the maps of the device-side stem re-packs
int build_stem_tables(pnvo_handle m, TrainState *t) {
  std::vector<int> ron(m->CPL, -1), ton(m->CPL, -1), perm(32, -1);
  for (int k = 0; k < m->CP; ++k) {
    ron[k] = m->stem_ref_of_new[k];
    ton[k] = m->stem_tensor_of_new[k];
    if (k < 32) perm[k] = m->stem_ref_of_new[k];
  }
  HIPCHK(m, t->d_ref_of_new.upload(ron.data(), ron.size()));
  HIPCHK(m, t->d_tensor_of_new.upload(ton.data(), ton.size()));
  HIPCHK(m, t->d_ciperm.upload(perm.data(), perm.size()));
  m->train_mx = false;
  if (m->mx_ok && m->convs[0].cout == 32 && m->mx_slot_ref.size() == 32) {   // stem on the bf16 matrix cores: device-side repack
    std::vector<int> mp(68, -1);
    for (int k = 0; k < 32; ++k) {
      mp[k] = m->mx_slot_ref[k];
      mp[32 + k] = m->mx_slot_new[k];
    }
    for (int x = 0; x < 4; ++x) mp[64 + x] = m->mx_xslot[x];
    HIPCHK(m, t->d_mxmaps.upload(mp.data(), mp.size()));
    m->train_mx = true;
  }
  if (!m->dd_ok) return PNVO_OK;
  // the one-hot-aware stem's operands are rebuilt on the device after every step
  const int bins = m->dd_bins;
  std::vector<int> mp(24 + 4 * bins, -1);
  auto find_new = [&](int tensor, int ch) {
    for (int nc = 0; nc < m->CP; ++nc)
      if (m->stem_tensor_of_new[nc] == tensor && m->stem_ch_of_new[nc] == ch && m->stem_ref_of_new[nc] >= 0) return nc;
    return -1;
  };
  for (int d = 0; d < 12; ++d) {
    if (m->dd_dense_tensor[d] < 0) continue;
    const int nc = find_new(m->dd_dense_tensor[d], m->dd_dense_ch[d]);
    mp[d] = m->stem_ref_of_new[nc];
    mp[12 + d] = nc;
    t->dd_nd = d + 1;
  }
  for (int k = 0; k < 2 * bins; ++k) {
    const int nc = find_new(2, k);
    mp[24 + k] = m->stem_ref_of_new[nc];
    mp[24 + 2 * bins + k] = nc;
  }
  HIPCHK(m, t->d_ddmaps.upload(mp.data(), mp.size()));
  return PNVO_OK;
}

// What pnvo_train_refresh launches over: the segment table of all re-pack maps, one float16 scale row per 3x3 / strided conv
// conv_x3.hip may take, and the GroupNorm-bound segments with their host-mapped ring.  The maps never change after attach.
int build_refresh_tables(pnvo_handle m, TrainState *t) {
  std::vector<GatherSeg> segs;
  for (const PackMap &pm : t->maps) {
    segs.push_back(GatherSeg{pm.map, pm.dst, t->seg_total});
    t->seg_total += (long)pm.map.size();
  }
  t->nseg = (int)segs.size();
  HIPCHK(m, t->d_segs.upload(segs.data(), segs.size()));
  if (m->bottleneck) return PNVO_OK;
  std::vector<long> x2;
  std::vector<TrainState::GnbSeg> gnb(m->convs.size(), TrainState::GnbSeg{0, 0, 0, 0.f});
  for (size_t li = 0; li < m->convs.size(); ++li) {
    const Layer &l = m->convs[li];
    TrainLayer &tl = t->conv[li];
    if (li >= 1) {
      tl.x2_row = t->x2_rows++;
      x2.push_back((long)tl.w.off);
      x2.push_back((long)tl.w.numel);
    }
    if (l.groups > 0)
      gnb[li] = TrainState::GnbSeg{(long)tl.gamma.off, (long)tl.beta.off, l.cout, (float)std::sqrt((double)(l.cout / l.groups) * l.hout * l.wout)};
  }
  if (!x2.empty()) {
    HIPCHK(m, t->x2_seg.upload(x2.data(), x2.size()));
    // {scale, 1/scale} per conv + the integer maxima launch_conv_x2_scales reduces into (zero between calls)
    HIPCHK(m, t->x2_scale.alloc(x2.size() + x2.size() / 2));
    HIPCHK(m, hipMemset(t->x2_scale, 0, t->x2_scale.size() * sizeof(float)));
  }
  t->gnb_n = (int)gnb.size();
  HIPCHK(m, t->gnb_seg.upload(gnb.data(), gnb.size()));
  HIPCHK(m, t->gnb_host.alloc_host(3 * gnb.size(), hipHostMallocMapped | hipHostMallocCoherent));
  for (int i = 0; i < 3 * t->gnb_n; ++i) t->gnb_host[i] = -1.f;
  for (hipEvent_t &e : t->gnb_ev) HIPCHK(m, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return PNVO_OK;
}

// Buckets of the gradient-ready hook.  The backward finishes the parameters in the order head, hidden layer, compression,
// layer4 ... layer1, stem; a range can be reported early when everything at or above its first offset belongs to layers
// the backward has left (true for the reference's state_dict order; any other order falls back to one final range).
void build_buckets(TrainState *t, const Toc &toc) {
  auto stage_of = [](const std::string &nm) {          // 5: after the residual stages, 1..4: residual stage, 0: stem / other
    const std::string bb = "visual_encoder.backbone.layer";
    if (nm.rfind(bb, 0) == 0 && nm.size() > bb.size()) return nm[bb.size()] - '0';
    if (nm.rfind("visual_encoder.backbone.", 0) == 0 || nm.rfind("action_embedding", 0) == 0) return 0;
    return 5;
  };
  for (int lo_stage : {4, 2}) {
    size_t first = t->n, below_end = 0;
    for (auto &kv : toc) {
      if (stage_of(kv.first) >= lo_stage) first = std::min(first, kv.second.off);
      else below_end = std::max(below_end, kv.second.off + kv.second.numel);
    }
    if (first < t->n && below_end <= first && (t->bucket_first.empty() || first < t->bucket_first.back()) && first > 0)
      t->bucket_first.push_back(first);
  }
  t->bucket_first.push_back(0);
}

// ---- workspace -----------------------------------------------------------------------------------------------------------

// What the forward conv of a weight-gradient launch read.
struct ConvInput {
  const float *x = nullptr;        // a plain tensor (a block input, the dropped activations), or
  const ConvSave *gn = nullptr;    // relu(GroupNorm(gn->raw)) of the producer, recomputed in the fetch, or
  bool obs = false;                // the stem's gathered, whitened observation tensors
};

// The weight-gradient launch of layer l (a conv of m->convs, m->fc or m->head) at B samples: problem (input geometry = the forward
// conv's), plan, and the kernel arguments with their operands.  ensure_train_ws sizes the scratch through it (null tensors), the backward
// launches through it.  dy_absmax: the absolute-maximum record of dy where the caller permits the float16 form, else nullptr.
struct WgradRequest {
  WgradPlan plan;
  WgradArgs args;
};
WgradRequest wgrad_request(pnvo_handle m, const TrainState *t, const Layer &l, int B, const ConvInput &in, const float *dy,
                           const unsigned *dy_absmax = nullptr) {
  const pnvo_config &c = m->cfg;
  WgradProblem q{.B = B, .H = l.hin, .W = l.win, .Ho = l.hout, .Wo = l.wout, .COUT = l.cout, .KH = l.k, .KW = l.kw, .stride = l.stride, .pad = l.pad};
  q.DYC = &l == &m->head ? 8 : &l == &m->fc ? c.hidden : l.coutp;       // dout8 / gh / a conv's raw-output gradient
  // channels per pixel of what the kernel reads.  The hidden layer reads the channel-PADDED compression map (H/W/CIN = fh, fw,
  // comp_cp tell the kernel the real row pitch); comp_cp is comp_c rounded up to whole 32-channel tiles, so the plan is the same.
  q.CIN = in.obs ? 32 : &l == &m->fc ? m->comp_cp : l.cin;
  q.mode = in.obs ? 2 : in.gn != nullptr ? 1 : 0;
  q.np = dy_absmax != nullptr ? 2 : 3;
  q.wgrad3 = m->opt.wgrad3;
  q.wgrad = m->opt.wgrad;
  WgradRequest r;
  r.plan = wgrad_plan(q);          // picks the kernel by mode, geometry and the two options
  WgradArgs &a = r.args = wgrad_args(q, r.plan);
  a.dy = dy;
  if (r.plan.np == 2) a.dy_absmax = dy_absmax;
  if (in.obs) {                    // mode 2 reads its per-channel whitening from the device tables
    const int nsrc[4] = {c.n_rgb, c.n_depth, c.n_dd, c.n_tdv};
    for (int k = 0; k < 32; ++k) {
      const int tn = k < m->CP ? m->stem_tensor_of_new[k] : -1;
      if (tn >= 0) a.src[k] = SrcLane{t->src[tn], nsrc[tn], m->stem_ch_of_new[k], 0.f, 0.f};
    }
    a.in_scale = m->stem_sc;
    a.in_shift = m->stem_sh;
  } else if (in.gn != nullptr) {
    a.x = in.gn->raw;
    a.in_scale = in.gn->ss[0];
    a.in_shift = in.gn->ss[1];
  } else {
    a.x = in.x;
  }
  return r;
}

// stem weight gradient on the bf16 matrix cores
WgradStemMXArgs wgrad_stem_mx_request(pnvo_handle m, const TrainState *t, int B) {
  WgradStemMXArgs a;
  std::memset(&a, 0, sizeof(a));
  for (int k = 0; k < 4; ++k) a.src[k] = t->src[k];
  a.dy = t->ws.dStem;
  a.zero_page = m->zero_page;
  a.B = B;
  a.H = m->cfg.height;
  a.W = m->cfg.width;
  a.Ho = m->Hs;
  a.Wo = m->Ws;
  wgrad_stem_mx_plan(a);
  return a;
}

// the same launch from the sensor frames of the last forward
WgradStemMXFrameArgs wgrad_stem_mx_frames_request(pnvo_handle m, const TrainState *t, int B) {
  WgradStemMXFrameArgs a;
  std::memset(&a, 0, sizeof(a));
  static_cast<WgradStemMXArgs &>(a) = wgrad_stem_mx_request(m, t, B);
  a.rgb_frames = t->f_rgb;
  a.depth_frames = t->f_depth;
  std::memcpy(a.edges, t->f_edges, sizeof(a.edges));
  a.flags = (m->cfg.n_depth > 0 ? 1 : 0) | (m->cfg.n_dd > 0 ? 2 : 0);
  return a;
}

// Do the frame-reading kernels serve this handle's training step — the 16-bit-matrix-core stem in the forward (stem plan MX) and
// wgrad_stem_mx_kernel<FRAMES> in the backward?  Else every frame entry materialises the pairs into the handle's workspace and takes
// the pair path (the rule of pnvo_forward_raw): same results as the pair path, the cost of the separate path.
bool train_frames_direct(pnvo_handle m) {
  const StemPlan sp = pnvo_stem_plan(m, true, {});
  return m->train_mx && sp.kernel == StemPlan::MX && !sp.standin && m->opt.wgrad_stem != 1 && !m->dense_sticky &&
         m->convs[0].coutp == 32 && (m->cfg.n_dd == 0 || m->cfg.n_dd == 20);
}

// floats of the largest weight-gradient scratch of a backward at B samples
size_t wgrad_scratch_floats(pnvo_handle m, const TrainState *t, int B) {
  size_t n = 0;
  for (size_t li = 0; li < m->convs.size(); ++li)
    n = std::max(n, wgrad_partial_floats(wgrad_request(m, t, m->convs[li], B, ConvInput{.obs = li == 0}, nullptr).plan));
  n = std::max(n, wgrad_partial_floats(wgrad_request(m, t, m->fc, B, {}, nullptr).plan));
  n = std::max(n, wgrad_partial_floats(wgrad_request(m, t, m->head, B, {}, nullptr).plan));
  if (m->train_mx) n = std::max(n, wgrad_stem_mx_scratch_floats(wgrad_stem_mx_request(m, t, B)));
  return n;
}

// Before a regrow: the old workspace goes first (not old and new side by side), and a failed regrow leaves capB = 0.
void free_train_ws(TrainState *t) {
  t->ws = TrainWs{};
  t->capB = 0;
}

int ensure_train_ws(pnvo_handle m, TrainState *t, int B) {
  if (B <= t->capB) return PNVO_OK;
  free_train_ws(t);
  int rc = pnvo_ensure_workspace(m, B);    // stats buffer etc. of the inference path are reused
  if (rc != PNVO_OK) return rc;
  const pnvo_config &c = m->cfg;
  TrainWs &w = t->ws;
  w.cs.resize(m->convs.size());
  // scratch gradients are as large as the largest activation
  size_t act = (size_t)B * m->Hp * m->Wp * c.baseplanes;
  int maxc = m->comp_cp, maxg = 1;
  for (size_t li = 0; li < m->convs.size(); ++li) {
    const Layer &l = m->convs[li];
    ConvSave &s = w.cs[li];
    HIPCHK(m, s.raw.alloc((size_t)B * l.hout * l.wout * l.coutp));
    for (int k = 0; k < 2; ++k) {
      HIPCHK(m, s.ss.alloc(k, (size_t)B * l.coutp));
      HIPCHK(m, hipMemset(s.ss[k], 0, (size_t)B * l.coutp * 4));
    }
    HIPCHK(m, s.mu.alloc((size_t)B * l.groups));
    HIPCHK(m, s.rstd.alloc((size_t)B * l.groups));
    if (li >= 1) act = std::max({act, (size_t)B * l.hout * l.wout * l.coutp, (size_t)B * l.hin * l.win * l.cinp});
    maxc = std::max(maxc, l.coutp);
    maxg = std::max(maxg, l.groups);
  }
  HIPCHK(m, w.wg_partial.alloc(wgrad_scratch_floats(m, t, B)));
  // block outputs: y[0] = pooled stem output, y[k] = output of m->blocks[k - 1]
  w.y.resize(m->blocks.size() + 1);
  HIPCHK(m, w.y[0].alloc((size_t)B * m->Hp * m->Wp * c.baseplanes));
  for (size_t k = 1; k <= m->blocks.size(); ++k) {
    const Layer &last = m->last(m->blocks[k - 1]);
    HIPCHK(m, w.y[k].alloc((size_t)B * last.hout * last.wout * last.coutp));
  }
  HIPCHK(m, w.pool_idx.alloc(act));
  const size_t nh = (size_t)B * c.hidden, nz = (size_t)B * m->fh * m->fw * m->comp_cp;
  const std::pair<DevBuf<float> *, size_t> bufs[] = {
      {&w.hid, nh},      {&w.dYa, act},     {&w.dYb, act}, {&w.G, act},   {&w.dRaw, act},
      {&w.dA, act},      {&w.dStem, (size_t)B * m->Hs * m->Ws * c.baseplanes},
      {&w.dout8, (size_t)B * 8},            {&w.dh, nh},   {&w.gh, nh},   {&w.dz, nz},
      {&w.gn_part, (size_t)B * 65 * maxc * 2},   // 64 chunks + [B][C][2]
      {&w.gn_coef, (size_t)B * maxg * 2},   {&w.zdrop, nz}, {&w.hdrop, nh}, {&w.dmask, std::max(nz, nh)}};
  for (const auto &b : bufs) HIPCHK(m, b.first->alloc(b.second));
  HIPCHK(m, w.mom_part.alloc((size_t)128 * MOMENTS_BLOCKS));
  if (c.act_embed) {
    const int rows = std::max(B, c.n_acts + 1);
    for (DevBuf<float> *b : {&w.egath, &w.efeat, &w.dfeat}) HIPCHK(m, b->alloc((size_t)rows * 32));
    HIPCHK(m, w.biasB.alloc((size_t)rows * c.hidden));
    std::vector<int64_t> io(rows);
    for (int k = 0; k < rows; ++k) io[k] = k;
    HIPCHK(m, w.iota.upload(io.data(), io.size()));
  }
  t->capB = B;
  return PNVO_OK;
}

// ---- backward launches -----------------------------------------------------------------------------------------------------

// The backward-data conv of layer l as a float32-MFMA problem: dX[B, hin, win, cin] (+)= conv(dRaw[B, hout, wout, coutp], flipped /
// transposed weights).  phase < 0: the full form (every tap, the forward's stride as upsampling).  phase = ph*2 + pw: the 1- or 2-tap
// dense stride-1 conv that produces output parity (ph, pw) of a stride-2 3x3 conv (Ho or Wo may come out 0: nothing to launch).
// What is off: the gradient is read as stored (mode 0), nothing is normalised behind it (no statistics), there is no bias or ReLU, and
// no split-K scratch is handed over.  The full form may take an LDS-staged kernel whatever option conv says — backward-data of a 3x3
// stride-1 conv is a 3x3 stride-1 conv; a phase writes a strided map, which only the generic kernel has.
ConvFp32Problem dgrad_problem(pnvo_handle m, const Layer &l, int B, bool accum, int phase) {
  const bool full = phase < 0;
  const int ph = full ? 0 : phase >> 1, pw = full ? 0 : phase & 1;
  ConvFp32Problem q{.B = B, .H = l.hout, .W = l.wout, .CIN = l.coutp, .Ho = full ? l.hin : (l.hin - ph + 1) / 2, .Wo = full ? l.win : (l.win - pw + 1) / 2,
                    .COUT = l.cin, .COUTP = rup(l.cin, 32), .KH = full ? l.k : ph ? 2 : 1, .KW = full ? l.kw : pw ? 2 : 1, .stride = 1,
                    .pad = full ? l.k - 1 - l.pad : 0, .up = full ? l.stride : 1, .y_cstride = l.cin, .mode = 0, .accum = accum};
  if (!full) {
    q.y_sh = q.y_sw = 2;
    q.y_oh = ph;
    q.y_ow = pw;
    q.y_H = l.hin;
    q.y_W = l.win;
  }
  q.linear = q.stats = q.ksplit_ok = false;
  q.head = 0;
  q.lds_ok = full;
  q.opt = pnvo_fp32_opts(m->opt, m->num_cus);
  return q;
}

// A transposed Linear as a 1x1 conv over B one-pixel samples, y[B, cout] = x[B, cin] . wpk: plain operand, no epilogue, no statistics,
// no split-K scratch, nothing for an LDS-staged kernel to stage.
ConvFp32Problem linear_t_problem(pnvo_handle m, int B, int cin, int cout) {
  ConvFp32Problem q{.B = B, .H = 1, .W = 1, .CIN = cin, .Ho = 1, .Wo = 1, .COUT = cout, .COUTP = rup(cout, 32), .KH = 1, .KW = 1, .stride = 1, .pad = 0,
                    .up = 1, .y_cstride = cout};
  q.opt = pnvo_fp32_opts(m->opt, m->num_cus);
  return q;
}

// Plan q and launch it on (x, wpk) -> y; a problem no instantiated kernel serves is an error named after `what`.
int run_fp32(pnvo_handle m, const ConvFp32Problem &q, const float *x, const float *wpk, float *y, const std::string &what, hipStream_t s) {
  const ConvFp32Plan p = conv_fp32_plan(q);
  if (!p) return pnvo_fail(m, PNVO_ERR_STATE, what + ": no float32-MFMA kernel is instantiated for this launch (check options fp32_tile, fp32_form)");
  ConvArgs a = conv_fp32_args(q, p);
  a.x = x;
  a.wpk = wpk;
  a.y = y;
  HIPCHK(m, launch_conv_fp32(a, p, s));
  return PNVO_OK;
}

// The conv_x3 operand of conv li's backward-data conv in np pieces (2: float16 on the forward's per-tensor scale wsc, 3: bf16),
// rebuilt from the flat parameters when m's weights moved since it was made.
int dgrad_x3_operand(pnvo_handle m, TrainState *t, size_t li, int np, const float *wsc, hipStream_t s) {
  const Layer &l = m->convs[li];
  TrainLayer &tl = t->conv[li];
  DevBuf<unsigned short> &wpk = tl.dgrad_x[np - 2];
  if (wpk && tl.dgrad_x_gen[np - 2] == m->weights_gen) return PNVO_OK;
  if (!wpk) HIPCHK(m, wpk.alloc((size_t)9 * l.coutp * l.cin * np));
  if (np == 2)
    HIPCHK(m, launch_conv_x2_repack(t->params + tl.w.off, l.cin, l.cout, l.coutp, l.cin, 3, 3, wsc, wpk, s, 1));
  else
    HIPCHK(m, launch_conv_x3_repack(t->params + tl.w.off, l.cin, l.cout, l.coutp, l.cin, 3, 3, 1, wpk, s));
  tl.dgrad_x_gen[np - 2] = m->weights_gen;
  return PNVO_OK;
}

// backward-data of conv li: dX[B, hin, win, cin] (+)= conv(dRaw[B, hout, wout, coutp], flipped/transposed weights)
int run_dgrad(pnvo_handle m, TrainState *t, size_t li, int B, const float *draw, float *dx, bool accum, hipStream_t s) {
  const Layer &l = m->convs[li];
  TrainLayer &tl = t->conv[li];
  const double flops = 2.0 * (double)B * l.hout * l.wout * l.cout * l.cin * l.k * l.kw;
  if (tl.dgrad_wph[0] != nullptr && m->opt.dgrad) {   // stride-2 3x3: four dense parity-phase convs instead of 9 taps, 3/4 masked
    PnvoTimed tm(m, s, tl.t_dgrad, flops, 0.0);
    for (int phase = 0; phase < 4; ++phase) {
      const ConvFp32Problem q = dgrad_problem(m, l, B, accum, phase);
      if (q.Ho > 0 && q.Wo > 0)
        if (int rc = run_fp32(m, q, draw, tl.dgrad_wph[phase], dx, "backward-data phase of " + l.name, s)) return rc;
    }
    return PNVO_OK;
  }
  // 3x3 stride-1: float32 results from the bf16 matrix cores (three-piece operands), as in the forward (PNVO_CONV=fp32: off)
  if (l.k == 3 && l.kw == 3 && l.stride == 1 && l.pad == 1 && !accum && l.cin % 32 == 0 && m->opt.conv <= 1) {
    // two float16 pieces (three terms) when the training forward uses them: the gradient is scaled by a power of two from its
    // absolute maximum (tracked by the GroupNorm backward that produced it), the weights carry the forward's per-tensor scale
    const float *wsc = m->opt.train_pieces == 2 && t->dmax != nullptr ? pnvo_train_x2_scale(m, l) : nullptr;
    // the transposed conv: input and output channels and sizes swapped, plain stager
    ConvX3Problem q{.B = B, .H = l.hout, .W = l.wout, .CIN = l.coutp, .Ho = l.hin, .Wo = l.win, .COUTP = l.cin, .ks = 3, .stride = 1};
    q.np = wsc != nullptr ? 2 : 3;
    q.absmax = wsc != nullptr;
    q.opt = {.force = m->opt.conv == 1, .strip = m->opt.x3_strip, .fine = 0, .w8 = 0, .m16 = 0, .ksw = 0,   // backward-data: the fine plan, W8, M16 and the K split stay off
             .persist_wgs = m->opt.x3_persist ? 3 * m->num_cus : 0,   // (32 -> 32 backward-data convs: resident weights, conv_x3p_kernel)
             .rows = 0, .num_cus = m->num_cus};                       // ... and the rows form, which has no gradient-input scaling
    if (const ConvX3Plan p = conv_x3_plan(q)) {
      if (int rc = dgrad_x3_operand(m, t, li, q.np, wsc, s)) return rc;
      ConvX3Args xa = conv_x3_args(q, p);
      xa.x = draw;
      xa.wpk = tl.dgrad_x[q.np - 2];
      xa.y = dx;
      if (wsc != nullptr) {
        xa.oscale_ptr = wsc + 1;
        xa.in_absmax = t->dmax + li * PNVO_ABSMAX_UINTS;
      }
      PnvoTimed tm(m, s, tl.t_dgrad, flops, 0.0);
      HIPCHK(m, launch_conv_x3(xa, p, s));
      return PNVO_OK;
    }
  }
  PnvoTimed tm(m, s, tl.t_dgrad, flops, 0.0);
  return run_fp32(m, dgrad_problem(m, l, B, accum, -1), draw, tl.dgrad_w, dx, "backward-data of " + l.name, s);
}

int run_wgrad(pnvo_handle m, TrainState *t, WgradRequest &r, const Weight &w, const int *perm, int cin_out, hipStream_t s) {
  WgradArgs &a = r.args;
  if (wgrad_partial_floats(r.plan) > t->ws.wg_partial.size()) return pnvo_fail(m, PNVO_ERR_STATE, "wgrad scratch too small");
  a.partial = t->ws.wg_partial;
  a.zero_page = m->zero_page;
  PnvoTimed tm(m, s, w.t_wgrad, 2.0 * (double)a.B * a.Ho * a.Wo * a.COUT * a.CIN * a.KH * a.KW, 0.0);
  HIPCHK(m, launch_wgrad(a, r.plan, t->grads + w.off, perm, cin_out, s));
  return PNVO_OK;
}

int run_gn_bwd(pnvo_handle m, TrainState *t, size_t li, int B, const float *dout, int mask, float *dx, hipStream_t s) {
  const Layer &l = m->convs[li];
  const TrainLayer &tl = t->conv[li];
  const ConvSave &c = t->ws.cs[li];
  PnvoTimed tm(m, s, T_GN_BWD, 0.0, 0.0);
  HIPCHK(m, launch_gn_bwd(c.raw, dout, c.ss[0], c.ss[1], c.mu, c.rstd, l.gamma, B, (long)l.hout * l.wout, l.coutp, l.cout, l.groups, mask,
                          t->ws.gn_part, t->ws.gn_coef, t->grads + tl.gamma.off, t->grads + tl.beta.off, dx, s,
                          t->dmax ? t->dmax + li * PNVO_ABSMAX_UINTS : nullptr));
  return PNVO_OK;
}

// Rebuild the stem's operands from the flat parameters and the current whitening tables: the three-piece bf16 B operand of
// stem_mx.hip when the model runs it (32 stem outputs), else the one-hot-aware stem's table / dense weights.
int refresh_stem_dd(pnvo_handle m, TrainState *t, hipStream_t s) {
  if (m->train_mx) {
    HIPCHK(m, launch_stem_mx_repack(t->params + t->stem_w_off, m->convs[0].cin, m->stem_sc, m->stem_sh, t->d_mxmaps, t->d_mxmaps + 32,
                                    t->d_mxmaps + 64, m->mx_wpk3, s));
    if (m->opt.train_pieces == 2 && m->mx_wpk2 != nullptr) {      // the float16 operand of the training forward, with its own scale
      if (!m->mx_scale2_dev) {                    // {scale, 1/scale, integer maximum of the folded weights (zero between calls)}
        HIPCHK(m, m->mx_scale2_dev.alloc(4));
        HIPCHK(m, hipMemset(m->mx_scale2_dev, 0, 4 * sizeof(float)));
      }
      HIPCHK(m, launch_stem_mx_repack_h(t->params + t->stem_w_off, m->convs[0].cin, m->stem_sc, m->stem_sh, t->d_mxmaps, t->d_mxmaps + 32,
                                        t->d_mxmaps + 64, m->mx_scale2_dev, m->mx_wpk2, s));
      m->mx_wpk2_dev = true;
    }
    if (!(m->dd_ok && m->opt.stem == 2)) return PNVO_OK;       // (option stem=dd on a model that trains on the mx stem: keep the
  }                                                             //  one-hot stem's operands current as well)
  if (!m->dd_ok) return PNVO_OK;
  const int bins = m->dd_bins;
  HIPCHK(m, launch_stem_dd_repack(t->params + t->stem_w_off, m->convs[0].cin, m->stem_sc, m->stem_sh, t->d_ddmaps,
                                  t->d_ddmaps + 12, t->dd_nd, t->d_ddmaps + 24, t->d_ddmaps + 24 + 2 * bins, bins,
                                  m->dd_table, m->dd_wpk, m->dd_sc, m->dd_sh, s));
  return PNVO_OK;
}

}  // namespace

void pnvo_train_free(pnvo_handle m) {
  if (!m || !m->train) return;
  TrainState *t = TS(m);
  for (hipEvent_t &e : t->gnb_ev)
    if (e) (void)hipEventDestroy(e);
  m->train_mx = false;
  delete t;
  m->train = nullptr;
}

// device {scale, 1/scale} of conv l's float16 pieces (nullptr: not attached, a Bottleneck model, not a conv that has a row)
const float *pnvo_train_x2_scale(pnvo_handle m, const Layer &l) {
  if (!m || !m->train) return nullptr;
  TrainState *t = TS(m);
  const long li = conv_index(m, l);
  return li < 0 || t->conv[li].x2_row < 0 || !t->x2_scale ? nullptr : t->x2_scale + 2 * t->conv[li].x2_row;
}

// device pointer of l's weight inside the caller's flat buffer (nullptr: not attached / not a layer of m)
const float *pnvo_train_weight_ptr(pnvo_handle m, const Layer &l) {
  if (!m || !m->train) return nullptr;
  TrainState *t = TS(m);
  if (&l == &m->fc || &l == &m->head) return t->params + (&l == &m->fc ? t->fc : t->head).w.off;
  const long li = conv_index(m, l);
  return li < 0 ? nullptr : t->params + t->conv[li].w.off;
}

extern "C" __global__ __launch_bounds__(64) void gn_bound_kernel(const float *params, const TrainState::GnbSeg *seg, float *out) {
  const TrainState::GnbSeg sg = seg[blockIdx.x];
  if (sg.c <= 0) {                       // no GroupNorm behind this conv: "no bound", never "not computed yet"
    if (threadIdx.x == 0) __hip_atomic_store(out + blockIdx.x, 3.0e38f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  float mx = 0.f;
  for (int c = threadIdx.x; c < sg.c; c += 64) mx = fmaxf(mx, fabsf(params[sg.goff + c]) * sg.rootn + fabsf(params[sg.boff + c]));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
  if (threadIdx.x == 0) __hip_atomic_store(out + blockIdx.x, fminf(mx, 3.0e38f), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Layer::in_bound from the bounds of the parameters TWO refreshes back (a fixed lag, so the float16-piece / three-piece choice
// per layer is the same run to run and rank to rank however far the host runs ahead of the stream): the ring entry is waited for
// through its event — the kernel behind it ran two optimiser steps ago, so the wait is over before it starts unless the host is
// more than two whole steps ahead.  Until two refreshes exist the load-time bounds stay.
static void chain_tracked_bounds(pnvo_handle m, TrainState *t) {
  if (!t->gnb_host || m->bottleneck || t->gnb_refreshes < 2) return;
  const int e = (int)((t->gnb_refreshes - 2) % 3);
  if (t->gnb_ev[e] == nullptr || hipEventSynchronize(t->gnb_ev[e]) != hipSuccess) return;
  const float *tab = t->gnb_host + (size_t)e * t->gnb_n;
  for (int i = 0; i < t->gnb_n; ++i)
    if (!(*(volatile const float *)(tab + i) >= 0.f)) return;
  pnvo_chain_in_bounds(m, [&](const Layer &l) {
    const long i = &l - m->convs.data();
    return i >= 0 && i < t->gnb_n ? *(volatile const float *)(tab + i) : 3.0e38f;
  });
}

// ---- training forward ------------------------------------------------------------------------------------------------------

// residual blocks: a chain of K convs (BasicBlock K = 2, resnet.py:29-55; Bottleneck K = 3, :58-117) + the skip branch
static int forward_blocks(pnvo_handle m, TrainState *t, int B, hipStream_t s) {
  TrainWs &w = t->ws;
  int rc = PNVO_OK;
  BlockTail tail{};
  const ConvSave *tail_x = nullptr;      // non-null: the previous block's tail rides on the next conv's stager
  for (size_t bk = 0; bk < m->blocks.size(); ++bk) {
    const Block &b = m->blocks[bk];
    const int K = b.nconv, *ik = b.conv;
    const float *xin = w.y[bk];
    float *yout = w.y[bk + 1];
    const bool ds = b.ds >= 0;
    // the block's downsample conv rides on its first conv's launch (conv_x3_kernel DSF); the block input stays in memory here —
    // the backward pass reads it
    const bool ds_ride = pnvo_ds_rides(m, b, B);
    DsRide ride{nullptr, nullptr, nullptr, nullptr, nullptr};
    if (ds_ride) {
      ConvSave &sd = w.cs[b.ds];
      ride = DsRide{&m->convs[b.ds], sd.raw, sd.ss, sd.mu, sd.rstd};
    }
    for (int k = 0; k < K; ++k) {
      const Layer &ck = m->convs[ik[k]];
      ConvSave &sk = w.cs[ik[k]];
      const ConvSave *sp = k ? &w.cs[ik[k - 1]] : nullptr;
      const DsRide *rd = (k == 0 && ds_ride) ? &ride : nullptr;
      if (k == 0 && tail_x != nullptr) {       // this conv's stager computes the previous block's tail and writes xin (= tail.out)
        rc = pnvo_run_conv(m, ck, B, {.x = tail_x->raw, .in_scale = tail_x->ss[0], .in_shift = tail_x->ss[1], .y = sk.raw, .y_cstride = ck.coutp,
                                      .ss = sk.ss, .mu = sk.mu, .rstd = sk.rstd, .tail = &tail, .ride = rd, .s = s});
        tail_x = nullptr;
      } else {
        rc = pnvo_run_conv(m, ck, B, {.x = k ? sp->raw : xin, .in_scale = k ? sp->ss[0] : nullptr, .in_shift = k ? sp->ss[1] : nullptr,
                                      .y = sk.raw, .y_cstride = ck.coutp, .ss = sk.ss, .mu = sk.mu, .rstd = sk.rstd, .ride = rd, .s = s});
      }
      if (rc != PNVO_OK) return rc;
    }
    const Layer &cl = m->convs[ik[K - 1]];
    ConvSave &sl = w.cs[ik[K - 1]];
    if (ds) {
      const Layer &cd = m->convs[b.ds];
      ConvSave &sd = w.cs[b.ds];
      if (!ds_ride && (rc = pnvo_run_conv(m, cd, B, {.x = xin, .y = sd.raw, .y_cstride = cd.coutp, .ss = sd.ss, .mu = sd.mu, .rstd = sd.rstd,
                                                     .s = s})) != PNVO_OK)
        return rc;
      tail = BlockTail{sd.raw, sd.ss[0], sd.ss[1], yout};
    } else {
      tail = BlockTail{xin, nullptr, nullptr, yout};
    }
    const bool last = bk + 1 == m->blocks.size();
    if (!last && pnvo_conv_takes_tail(m, m->convs[m->next_conv_after(bk)], B))   // the next block's first conv computes and writes yout
      tail_x = &sl;
    else
      HIPCHK(m, launch_residual(sl.raw, sl.ss[0], sl.ss[1], tail.res, tail.res_scale, tail.res_shift, B, (long)cl.hout * cl.wout, cl.coutp,
                                yout, s));
  }
  return PNVO_OK;
}

// Dropout -> Linear -> ReLU -> Dropout -> Linear (vo_cnn.py:216-227) on the compression conv's output, masks by hash
static int forward_linears(pnvo_handle m, TrainState *t, int B, float *out, hipStream_t s) {
  const pnvo_config &c = m->cfg;
  TrainWs &w = t->ws;
  const ConvSave &sc = w.cs[m->comp];
  int rc = PNVO_OK;
  ++t->drop_step;
  const float *fcb = m->fc_bias;
  const int64_t *fcrow = nullptr;
  if (c.act_embed) {                // the embedding columns of the Linear as per-sample bias rows (vo_cnn_act_embed.py:63-72)
    const int flat = m->comp_c * m->fh * m->fw;
    HIPCHK(m, launch_embed_gather(t->params + t->emb_off, t->actions, B, c.n_acts + 1, w.egath, t->embed_err, s));
    if (t->drop_p > 0.f)            // nn.Dropout acts on the concatenated [visual | embedding] vector: mask "layer" 2
      HIPCHK(m, launch_dropout(w.egath, nullptr, nullptr, B, 1, 32, t->drop_p, t->drop_seed, t->drop_step, 2, w.efeat, s));
    else
      HIPCHK(m, hipMemcpyAsync(w.efeat, w.egath, (size_t)B * 32 * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(m, launch_embed_bias(w.efeat, t->params + t->fc.w.off, t->w1_pitch, flat, t->params + t->fc.b.off, B, c.hidden, w.biasB, s));
    fcb = w.biasB;
    fcrow = w.iota;
  }
  if (t->drop_p > 0.f) {
    HIPCHK(m, launch_dropout(sc.raw, sc.ss[0], sc.ss[1], B, (long)m->fh * m->fw, m->comp_cp, t->drop_p, t->drop_seed, t->drop_step, 0,
                             w.zdrop, s));
    if ((rc = pnvo_run_conv(m, m->fc, B, {.x = w.zdrop, .y = w.hid, .y_cstride = c.hidden, .bias = fcb, .bias_row = fcrow, .relu_out = 1,
                                          .s = s})) != PNVO_OK)
      return rc;
    HIPCHK(m, launch_dropout(w.hid, nullptr, nullptr, B, 1, c.hidden, t->drop_p, t->drop_seed, t->drop_step, 1, w.hdrop, s));
    return pnvo_run_conv(m, m->head, B, {.x = w.hdrop, .y = out, .y_cstride = c.out_dim, .bias = m->head_bias, .s = s});
  }
  if ((rc = pnvo_run_conv(m, m->fc, B, {.x = sc.raw, .in_scale = sc.ss[0], .in_shift = sc.ss[1], .y = w.hid, .y_cstride = c.hidden,
                                        .bias = fcb, .bias_row = fcrow, .relu_out = 1, .s = s})) != PNVO_OK)
    return rc;
  return pnvo_run_conv(m, m->head, B, {.x = w.hid, .y = out, .y_cstride = c.out_dim, .bias = m->head_bias, .s = s});
}

// raw != nullptr: the sensor frames feed the stem (rgb / depth / dd are null; the caller checked them against the model)
static int train_forward_body(pnvo_handle m, const float *rgb, const float *depth, const float *dd, const float *tdv, int B,
                              const float *run_mean, const float *run_var, float *out, void *stream, const RawFrames *raw = nullptr) {
  if (!m || !m->train) return pnvo_fail(m, PNVO_ERR_STATE, "pnvo_train_attach first");
  if (B <= 0 || !out) return pnvo_fail(m, PNVO_ERR_ARG, "bad batch / null output");
  const pnvo_config &c = m->cfg;
  if (raw == nullptr && ((c.n_rgb > 0) != (rgb != nullptr) || (c.n_depth > 0) != (depth != nullptr) || (c.n_dd > 0) != (dd != nullptr) ||
      (c.n_tdv > 0) != (tdv != nullptr)))
    return pnvo_fail(m, PNVO_ERR_ARG, "observation tensors do not match the model's observation_space");
  if (c.normalize && (!run_mean || !run_var)) return pnvo_fail(m, PNVO_ERR_ARG, "running statistics required");
  HIPCHK(m, hipSetDevice(m->device));
  TrainState *t = TS(m);
  chain_tracked_bounds(m, t);            // float16-piece range guard follows the parameters as they train
  int rc = ensure_train_ws(m, t, B);
  if (rc != PNVO_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (c.act_embed && !t->actions) return pnvo_fail(m, PNVO_ERR_ARG, "act_embed model: pnvo_train_set_actions first");
  t->lastB = B;
  t->src[0] = rgb;
  t->src[1] = depth;
  t->src[2] = dd;
  t->src[3] = tdv;
  t->from_frames = raw != nullptr;
  if (raw != nullptr) {
    t->f_rgb = raw->rgb;
    t->f_depth = raw->depth;
    for (int i = 0; i < 12; ++i) t->f_edges[i] = i >= 10 ? 1.0f : raw->edges != nullptr ? raw->edges[i] : (float)((double)i * 1.0 / 10.0);
    if (raw->edges != nullptr) t->f_edges[10] = raw->edges[10];
  }
  if (c.normalize)   // RunningMeanAndVar buffers live on the device and change every step (running_mean_and_var.py:54-60)
    HIPCHK(m, launch_whiten_table(run_mean, run_var, t->d_ref_of_new, t->d_tensor_of_new, m->CPL, m->stem_sc, m->stem_sh, s));
  if ((rc = refresh_stem_dd(m, t, s)) != PNVO_OK) return rc;   // W/std table, indicator weights: both move every step
  TrainWs &w = t->ws;
  ConvSave &cs = w.cs[0];
  if ((rc = pnvo_run_stem(m, B, {.src = {t->src[0], t->src[1], t->src[2], t->src[3]}, .raw = raw ? *raw : RawFrames{}, .y = cs.raw, .ss = cs.ss, .mu = cs.mu, .rstd = cs.rstd,
                                 .train_fwd = true, .s = s})) != PNVO_OK)
    return rc;
  HIPCHK(m, launch_maxpool_train(cs.raw, cs.ss[0], cs.ss[1], B, m->Hs, m->Ws, m->convs[0].coutp, w.y[0], w.pool_idx, s));
  if ((rc = forward_blocks(m, t, B, s)) != PNVO_OK) return rc;
  const Layer &comp = m->convs[m->comp];
  ConvSave &sc = w.cs[m->comp];
  if ((rc = pnvo_run_conv(m, comp, B, {.x = w.y[m->blocks.size()], .y = sc.raw, .y_cstride = comp.coutp, .ss = sc.ss, .mu = sc.mu, .rstd = sc.rstd,
                                       .s = s})) != PNVO_OK)
    return rc;
  return forward_linears(m, t, B, out, s);
}

// ---- backward --------------------------------------------------------------------------------------------------------------

// bucket k of the gradient-ready hook is final: report it (host callback; the launches that produce it are enqueued on `s`)
static void report_bucket(TrainState *t, size_t k, hipStream_t s) {
  if (k >= t->bucket_first.size()) return;
  if (t->bucket_done.size() != t->bucket_first.size()) t->bucket_done.assign(t->bucket_first.size(), 0);
  if (t->bucket_done[k]) return;
  t->bucket_done[k] = 1;
  if (!t->hook) return;
  const size_t end = k == 0 ? t->n : t->bucket_first[k - 1];
  t->hook(t->hook_user, (uint64_t)t->bucket_first[k], (uint64_t)(end - t->bucket_first[k]), (void *)s);
}

// output head: out = hid . W2^T + b2
static int backward_head(pnvo_handle m, TrainState *t, int B, const float *grad_out, hipStream_t s) {
  const pnvo_config &c = m->cfg;
  TrainWs &w = t->ws;
  HIPCHK(m, launch_padcopy(grad_out, B, c.out_dim, 8, w.dout8, s));
  HIPCHK(m, launch_colsum(grad_out, B, c.out_dim, c.out_dim, t->grads + t->head.b.off, s));
  WgradRequest a = wgrad_request(m, t, m->head, B, {.x = t->drop_p > 0.f ? w.hdrop : w.hid}, w.dout8);
  if (int rc = run_wgrad(m, t, a, t->head.w, nullptr, c.hidden, s)) return rc;
  return run_fp32(m, linear_t_problem(m, B, 8, c.hidden), w.dout8, t->head_t, w.dh, "transposed output head", s);
}

// hidden layer: hid = relu(z . W1^T + b1); dh -> dz (stop_after_fc: only the layer's own gradients)
static int backward_hidden(pnvo_handle m, TrainState *t, int B, bool stop_after_fc, hipStream_t s) {
  const pnvo_config &c = m->cfg;
  TrainWs &w = t->ws;
  const bool drop = t->drop_p > 0.f;
  if (drop)                         // dropout backward: the same mask, then the ReLU mask of the un-dropped activation
    HIPCHK(m, launch_dropout(w.dh, nullptr, nullptr, B, 1, c.hidden, t->drop_p, t->drop_seed, t->drop_step, 1, w.dh, s));
  HIPCHK(m, launch_relu_mask(w.dh, w.hid, nullptr, (long)B * c.hidden, w.gh, s));
  HIPCHK(m, launch_colsum(w.gh, B, c.hidden, c.hidden, t->grads + t->fc.b.off, s));
  // with dropout the Linear saw the dropped, already activated feature
  WgradRequest a = wgrad_request(m, t, m->fc, B, drop ? ConvInput{.x = w.zdrop} : ConvInput{.gn = &w.cs[m->comp]}, w.gh);
  if (c.act_embed) {                // gradient rows are [flat | 32] wide; the embedding columns and rows come from embed_*
    const int flat = m->comp_c * m->fh * m->fw;
    a.args.grad_pitch = t->w1_pitch;
    HIPCHK(m, launch_embed_backward(w.gh, w.efeat, t->params + t->fc.w.off, t->w1_pitch, flat, B, c.hidden, t->grads + t->fc.w.off, w.dfeat,
                                    s));
    if (drop) HIPCHK(m, launch_dropout(w.dfeat, nullptr, nullptr, B, 1, 32, t->drop_p, t->drop_seed, t->drop_step, 2, w.dfeat, s));
    HIPCHK(m, launch_embed_scatter(w.dfeat, t->actions, B, c.n_acts + 1, t->grads + t->emb_off, s));
  }
  if (int rc = run_wgrad(m, t, a, t->fc.w, nullptr, m->comp_c, s)) return rc;
  if (stop_after_fc) return PNVO_OK;
  if (int rc = run_fp32(m, linear_t_problem(m, B, c.hidden, m->fh * m->fw * m->comp_cp), w.gh, t->fc_t, w.dz, "transposed hidden layer", s)) return rc;
  if (drop)
    HIPCHK(m, launch_dropout(w.dz, nullptr, nullptr, B, (long)m->fh * m->fw, m->comp_cp, t->drop_p, t->drop_seed, t->drop_step, 0, w.dz, s));
  return PNVO_OK;
}

// compression conv + GroupNorm(1) + ReLU: dz -> dY
static int backward_compression(pnvo_handle m, TrainState *t, int B, float *dY, hipStream_t s) {
  TrainWs &w = t->ws;
  const size_t li = m->comp;
  const Layer &l = m->convs[li];
  int rc = run_gn_bwd(m, t, li, B, w.dz, 1, w.dz, s);   // in place: dz -> dCompRaw
  if (rc != PNVO_OK) return rc;
  WgradRequest a = wgrad_request(m, t, l, B, {.x = w.y[m->blocks.size()]}, w.dz);
  if ((rc = run_wgrad(m, t, a, t->conv[li].w, nullptr, l.cin, s)) != PNVO_OK) return rc;
  return run_dgrad(m, t, li, B, w.dz, dY, false, s);
}

// residual block b, whose input is y[blk - 1] and output y[blk]: dY (gradient of the output) -> dX (of the input)
static int backward_block(pnvo_handle m, TrainState *t, size_t blk, int B, const float *dY, float *dX, hipStream_t s) {
  TrainWs &w = t->ws;
  const Block &b = m->blocks[blk - 1];
  const int K = b.nconv, *ik = b.conv;
  const Layer &c1 = m->convs[ik[0]], &cl = m->convs[ik[K - 1]];
  const float *xin = w.y[blk - 1];
  int rc = PNVO_OK;
  // G = dY * (y > 0)
  HIPCHK(m, launch_relu_mask(dY, w.y[blk], nullptr, (long)B * cl.hout * cl.wout * cl.coutp, w.G, s));
  // the chain, last conv first: GroupNorm (+ ReLU mask for every conv but the last) <- incoming gradient
  const float *din = w.G;
  for (int k = K - 1; k >= 0; --k) {
    const Layer &ck = m->convs[ik[k]];
    if ((rc = run_gn_bwd(m, t, ik[k], B, din, k == K - 1 ? 0 : 1, w.dRaw, s)) != PNVO_OK) return rc;
    // conv k > 0 saw relu(GN(raw of the previous conv))
    // float16 pieces are permitted with X inside float16's range (the forward's bound) and dY scaled from its recorded maximum
    const bool f16 = m->opt.train_pieces == 2 && t->dmax != nullptr && ck.in_bound < 6.0e4f;
    WgradRequest a = wgrad_request(m, t, ck, B, k ? ConvInput{.gn = &w.cs[ik[k - 1]]} : ConvInput{.x = xin}, w.dRaw,
                                   f16 ? t->dmax + ik[k] * PNVO_ABSMAX_UINTS : nullptr);
    if ((rc = run_wgrad(m, t, a, t->conv[ik[k]].w, nullptr, ck.cin, s)) != PNVO_OK) return rc;
    if ((rc = run_dgrad(m, t, ik[k], B, w.dRaw, k ? w.dA : dX, false, s)) != PNVO_OK) return rc;
    din = w.dA;
  }
  if (b.ds < 0) {                   // identity skip
    HIPCHK(m, launch_add(dX, w.G, (long)B * c1.hin * c1.win * c1.cin, dX, s));
    return PNVO_OK;
  }
  const Layer &cd = m->convs[b.ds];
  if ((rc = run_gn_bwd(m, t, b.ds, B, w.G, 0, w.dRaw, s)) != PNVO_OK) return rc;
  WgradRequest a = wgrad_request(m, t, cd, B, {.x = xin}, w.dRaw);
  if ((rc = run_wgrad(m, t, a, t->conv[b.ds].w, nullptr, cd.cin, s)) != PNVO_OK) return rc;
  return run_dgrad(m, t, b.ds, B, w.dRaw, dX, true, s);
}

// stem: maxpool <- dY, GroupNorm + ReLU, weight gradient (no input gradient)
static int backward_stem(pnvo_handle m, TrainState *t, int B, const float *dY, hipStream_t s) {
  TrainWs &w = t->ws;
  const Layer &l = m->convs[0];
  const TrainLayer &tl = t->conv[0];
  if (m->opt.pool_bwd && l.coutp == l.cout && l.cout % 4 == 0 && l.cout <= 256 && 256 % (l.cout / 4) == 0) {
    // max-pool backward folded into the stem's GroupNorm backward: the un-pooled gradient is never materialised
    const ConvSave &cs0 = w.cs[0];
    PnvoTimed tm(m, s, T_GN_BWD, 0.0, 0.0);
    HIPCHK(m, launch_gn_bwd_pool(cs0.raw, dY, w.pool_idx, m->Hs, m->Ws, m->Hp, m->Wp, cs0.ss[0], cs0.ss[1], cs0.mu, cs0.rstd, l.gamma, B, l.cout,
                                 l.groups, w.gn_part, w.gn_coef, t->grads + tl.gamma.off, t->grads + tl.beta.off, w.dStem, s));
  } else {
    HIPCHK(m, launch_maxpool_bwd(dY, w.pool_idx, B, m->Hs, m->Ws, l.coutp, w.dStem, s));
    if (int rc = run_gn_bwd(m, t, 0, B, w.dStem, 1, w.dStem, s)) return rc;
  }
  // option wgrad_stem=fp32: the float32-MFMA kernel; also once an input outside the exact-operand contract was met
  const bool stem_fp32 = m->opt.wgrad_stem == 1 || m->dense_sticky;
  // the matrix-core stem kernel, from the pair tensors or the sensor frames: scratch check, timing entry, launch
  const auto run_mx = [&](const auto &a, auto launch) -> int {
    if (wgrad_stem_mx_scratch_floats(a) > w.wg_partial.size()) return pnvo_fail(m, PNVO_ERR_STATE, "wgrad scratch too small");
    PnvoTimed tm(m, s, tl.w.t_wgrad, 2.0 * (double)B * m->Hs * m->Ws * l.cout * l.cin * 49, 0.0);
    HIPCHK(m, launch(a, w.wg_partial, m->stem_sc, m->stem_sh, t->d_mxmaps, t->d_mxmaps + 32, l.cin, t->grads + tl.w.off, s));
    return PNVO_OK;
  };
  if (t->from_frames) {              // the forward read sensor frames: wgrad_stem_mx_kernel<FRAMES> reads them again, nothing else can
    if (!train_frames_direct(m))
      return pnvo_fail(m, PNVO_ERR_STATE, "the last forward came from sensor frames and an option moved the handle off the frame-reading "
                                          "kernels before its backward: run pnvo_train_forward_raw again");
    return run_mx(wgrad_stem_mx_frames_request(m, t, B), launch_wgrad_stem_mx_frames);
  }
  if (m->train_mx && l.coutp == 32 && !stem_fp32) return run_mx(wgrad_stem_mx_request(m, t, B), launch_wgrad_stem_mx);
  WgradRequest a = wgrad_request(m, t, l, B, {.obs = true}, w.dStem);
  return run_wgrad(m, t, a, tl.w, t->d_ciperm, l.cin, s);
}

// grad_out: dLoss / dOut, or nullptr with dh_in = dLoss / d(hidden vector) from the caller (the head's gradients are left alone)
static int train_backward_body(pnvo_handle m, TrainState *t, const float *grad_out, const float *dh_in, bool stop_after_fc, hipStream_t s) {
  if (t->lastB <= 0 || (!grad_out && !dh_in)) return pnvo_fail(m, PNVO_ERR_STATE, "pnvo_train_forward first");
  HIPCHK(m, hipSetDevice(m->device));
  const int B = t->lastB;
  int rc = PNVO_OK;
  if (!t->dmax && !m->bottleneck) HIPCHK(m, t->dmax.alloc(m->convs.size() * PNVO_ABSMAX_UINTS));
  if (t->dmax) HIPCHK(m, hipMemsetAsync(t->dmax, 0, t->dmax.size() * sizeof(unsigned), s));   // maxima of this backward's gradients
  if (dh_in != nullptr)
    HIPCHK(m, hipMemcpyAsync(t->ws.dh, dh_in, (size_t)B * m->cfg.hidden * sizeof(float), hipMemcpyDeviceToDevice, s));
  else if ((rc = backward_head(m, t, B, grad_out, s)) != PNVO_OK)
    return rc;
  if ((rc = backward_hidden(m, t, B, stop_after_fc, s)) != PNVO_OK || stop_after_fc) return rc;
  float *dY = t->ws.dYa, *dX = t->ws.dYb;
  if ((rc = backward_compression(m, t, B, dY, s)) != PNVO_OK) return rc;
  // residual blocks, last to first: m->blocks in reverse (y[blk] is the output of m->blocks[blk - 1])
  for (size_t blk = m->blocks.size(); blk >= 1; --blk) {
    if ((rc = backward_block(m, t, blk, B, dY, dX, s)) != PNVO_OK) return rc;
    std::swap(dY, dX);
    // leaving residual stage 4 / stage 2: every parameter from that stage's first offset upwards has its final gradient
    const Block &b = m->blocks[blk - 1];
    if (t->bucket_first.size() == 3 && b.index == 0 && (b.stage == 4 || b.stage == 2)) report_bucket(t, b.stage == 4 ? 0 : 1, s);
  }
  return backward_stem(m, t, B, dY, s);
}

// One backward of the gradient-ready hook's contract: reset the buckets, run, report what is left.  The end of the backward
// reports every range not reported on the way (whatever the number of split points a parameter order allowed — with exactly one of
// them the in-backward reports are skipped and BOTH ranges are due here), latest layers first.
static int run_backward(pnvo_handle m, const float *grad_out, const float *dh_in, bool stop_after_fc, void *stream) {
  if (!m || !m->train) return pnvo_fail(m, PNVO_ERR_STATE, "pnvo_train_attach first");
  TrainState *t = TS(m);
  t->bucket_done.assign(t->bucket_first.size(), 0);
  const int rc = train_backward_body(m, t, grad_out, dh_in, stop_after_fc, (hipStream_t)stream);
  for (size_t k = 0; rc == PNVO_OK && k < t->bucket_first.size(); ++k) report_bucket(t, k, (hipStream_t)stream);
  return rc;
}

// The hidden vector of the last pnvo_train_forward (visual_fc's output after its ReLU), [B, hidden] on the device; nullptr before one.
const float *pnvo_train_hidden(pnvo_handle m) { return m && m->train && TS(m)->lastB > 0 ? TS(m)->ws.hid : nullptr; }

// The backward entered BELOW the output head: dh [B, hidden] = dLoss / d(hidden vector) comes from the caller (the navigation policy's
// recurrent part, policy_train.hip), the head's own gradients are left alone.  stop_after_fc: only visual_fc's weight and bias
// gradients are written (a frozen visual encoder).
int pnvo_train_backward_from_hidden(pnvo_handle m, const float *dh, bool stop_after_fc, void *stream) {
  if (!dh) return pnvo_fail(m, PNVO_ERR_ARG, "null hidden gradient");
  return run_backward(m, nullptr, dh, stop_after_fc, stream);
}

extern "C" {

int pnvo_train_attach(pnvo_handle m, float *params, float *grads, size_t n_floats, const pnvo_tensor_desc *toc, int ntoc) {
  if (!m || !params || !grads || !toc) return pnvo_fail(m, PNVO_ERR_ARG, "null argument");
  if (!m->loaded) return pnvo_fail(m, PNVO_ERR_STATE, "pnvo_train_attach before pnvo_load_weights");
  if (m->grouped_se)
    return pnvo_fail(m, PNVO_ERR_STATE, "pnvo_train_attach: SE / ResNeXt backbones have no backward (the grouped conv and the gate are "
                                        "inference kernels): these encoders run frozen");
  if (n_floats >= (1u << 24)) return pnvo_fail(m, PNVO_ERR_ARG, "flat parameter buffer too large for the index maps");
  HIPCHK(m, hipSetDevice(m->device));
  pnvo_train_free(m);
  TrainState *t = new TrainState();
  m->train = t;
  auto failed = [&](int rc) {          // a failed attach leaves no training state behind
    pnvo_train_free(m);
    return rc;
  };
  t->params = params;
  t->grads = grads;
  t->n = n_floats;
  Toc names;
  for (int k = 0; k < ntoc; ++k) {
    TocEnt e;
    e.off = toc[k].offset;
    e.numel = 1;
    for (int d = 0; d < toc[k].ndim; ++d) {
      e.shape.push_back(toc[k].shape[d]);
      e.numel *= (size_t)toc[k].shape[d];
    }
    if (e.off + e.numel > n_floats) return failed(pnvo_fail(m, PNVO_ERR_ARG, std::string("parameter '") + toc[k].name + "' out of range"));
    names[toc[k].name] = e;
  }
  int rc = PNVO_OK;
  if ((rc = bind_convs(m, t, names)) != PNVO_OK || (rc = bind_linears(m, t, names)) != PNVO_OK || (rc = build_stem_tables(m, t)) != PNVO_OK ||
      (rc = build_refresh_tables(m, t)) != PNVO_OK)
    return failed(rc);
  build_buckets(t, names);
  rc = pnvo_train_refresh(m, nullptr);
  return rc == PNVO_OK ? rc : failed(rc);
}

int pnvo_train_set_grad_hook(pnvo_handle m, pnvo_grad_ready_fn fn, void *user) {
  if (!m || !m->train) return pnvo_fail(m, PNVO_ERR_STATE, "pnvo_train_attach first");
  TS(m)->hook = fn;
  TS(m)->hook_user = user;
  return PNVO_OK;
}

int pnvo_train_grad_buckets(pnvo_handle m, uint64_t *first, uint64_t *count, int cap, int *n_out) {
  if (!m || !m->train || !n_out) return pnvo_fail(m, PNVO_ERR_STATE, "pnvo_train_attach first");
  TrainState *t = TS(m);
  *n_out = (int)t->bucket_first.size();
  size_t end = t->n;
  for (int k = 0; k < *n_out && k < cap && first && count; ++k) {
    first[k] = t->bucket_first[k];
    count[k] = end - t->bucket_first[k];
    end = t->bucket_first[k];
  }
  return PNVO_OK;
}

// The operands that follow the flat parameters, rebuilt after every optimiser step.  Only launches: every table was built by attach.
int pnvo_train_refresh(pnvo_handle m, void *stream) {
  if (!m || !m->train) return pnvo_fail(m, PNVO_ERR_STATE, "pnvo_train_attach first");
  HIPCHK(m, hipSetDevice(m->device));
  TrainState *t = TS(m);
  hipStream_t s = (hipStream_t)stream;
  m->weights_gen += 1;               // operands derived lazily from the weights (conv_x3) are rebuilt at their next use
  HIPCHK(m, launch_gather_all(t->params, t->d_segs, t->nseg, t->seg_total, s));
  if (t->x2_seg) HIPCHK(m, launch_conv_x2_scales(t->params, t->x2_seg, t->x2_rows, t->x2_scale, s));
  if (!m->bottleneck) {                // GroupNorm bounds of the CURRENT parameters -> host-mapped table (chain_tracked_bounds)
    // A refresh that is being CAPTURED would bake one ring entry into the graph: every replay rewrites that entry while the host reads
    // another one behind an event that is never recorded.  So a captured refresh leaves the ring alone and marks every entry unknown
    // (-1) and restarts the two-refresh lag: chain_tracked_bounds then leaves Layer::in_bound as last chained (the load-time bounds
    // when nothing was chained yet) instead of reading an entry that no event orders.
    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(s, &cst) != hipSuccess || cst != hipStreamCaptureStatusNone;
    if (capturing) {
      for (int i = 0; i < 3 * t->gnb_n; ++i) t->gnb_host[i] = -1.f;
      t->gnb_refreshes = 0;
    } else {
      const int e = (int)(t->gnb_refreshes % 3);
      hipLaunchKernelGGL(gn_bound_kernel, dim3((unsigned)t->gnb_n), dim3(64), 0, s, t->params, t->gnb_seg, t->gnb_host + (size_t)e * t->gnb_n);
      HIPCHK(m, hipGetLastError());
      HIPCHK(m, hipEventRecord(t->gnb_ev[e], s));
      t->gnb_refreshes += 1;
    }
  }
  if (m->cfg.act_embed) {      // eval-mode bias rows bias[a][o] = b1[o] + W1[o][flat:] . emb[a]  (pnvo_load_weights does this on the host)
    const pnvo_config &c = m->cfg;
    const int rows = c.n_acts + 1, flat = m->comp_c * m->fh * m->fw;
    int rc = ensure_train_ws(m, t, t->capB > 0 ? t->capB : 1);
    if (rc != PNVO_OK) return rc;
    HIPCHK(m, launch_embed_gather(t->params + t->emb_off, nullptr, rows, rows, t->ws.egath, nullptr, s));
    HIPCHK(m, launch_embed_bias(t->ws.egath, t->params + t->fc.w.off, t->w1_pitch, flat, t->params + t->fc.b.off, rows, c.hidden, m->fc_bias, s));
  }
  return refresh_stem_dd(m, t, s);
}

int pnvo_train_forward(pnvo_handle m, const float *rgb, const float *depth, const float *dd, const float *tdv, int B,
                       const float *run_mean, const float *run_var, float *out, void *stream) {
  int rc = train_forward_body(m, rgb, depth, dd, tdv, B, run_mean, run_var, out, stream);
  if (rc != PNVO_OK) return rc;
  bool rerun = false;                  // an input outside the fused stems' contract: once more on the dense stem (pnvo_api.hip)
  if ((rc = pnvo_input_fallback(m, (hipStream_t)stream, &rerun)) != PNVO_OK) return rc;
  return rerun ? train_forward_body(m, rgb, depth, dd, tdv, B, run_mean, run_var, out, stream) : PNVO_OK;
}

// pnvo_train_forward from the sensor frames.  On the frame-reading kernels nothing is waited for: frames are inside the stems' input
// contract by construction (no event, no re-run), and the record on the training state tells the backward which stem ran.
int pnvo_train_forward_raw(pnvo_handle m, const uint8_t *rgb_frames, const float *depth_frames, const float *tdv, const float *edges, int B,
                           const float *run_mean, const float *run_var, float *out, int32_t *err_flag, void *stream) {
  if (int rc0 = pnvo_check_frames(m, "pnvo_train_forward_raw", rgb_frames, depth_frames, tdv, B, out)) return rc0;
  if (!m->train) return pnvo_fail(m, PNVO_ERR_STATE, "pnvo_train_attach first");
  if (!depth_frames) return pnvo_fail(m, PNVO_ERR_ARG, "pnvo_train_forward_raw: depth_frames is required");
  const pnvo_config &c = m->cfg;
  if (!train_frames_direct(m)) {
    HIPCHK(m, hipSetDevice(m->device));
    TrainState *t = TS(m);
    if (int rc = pnvo_raw_materialise(m, rgb_frames, depth_frames, B, edges, err_flag, (hipStream_t)stream, t->fpairs, &t->fpairs_cap)) return rc;
    return pnvo_train_forward(m, c.n_rgb ? t->fpairs[0] : nullptr, c.n_depth ? t->fpairs[1] : nullptr, c.n_dd ? t->fpairs[2] : nullptr, tdv, B,
                              run_mean, run_var, out, stream);
  }
  const RawFrames raw{rgb_frames, depth_frames, err_flag, edges};
  return train_forward_body(m, nullptr, nullptr, nullptr, tdv, B, run_mean, run_var, out, stream, &raw);
}

int pnvo_train_backward(pnvo_handle m, const float *grad_out, void *stream) { return run_backward(m, grad_out, nullptr, false, stream); }

int pnvo_train_set_dropout(pnvo_handle m, float p, uint64_t seed) {
  if (!m || !m->train) return pnvo_fail(m, PNVO_ERR_STATE, "pnvo_train_attach first");
  if (!(p >= 0.f && p < 1.f)) return pnvo_fail(m, PNVO_ERR_ARG, "dropout p must be in [0, 1)");
  TrainState *t = TS(m);
  t->drop_p = p;
  t->drop_seed = seed;
  return PNVO_OK;
}

int pnvo_train_set_actions(pnvo_handle m, const int64_t *actions) {
  if (!m || !m->train) return pnvo_fail(m, PNVO_ERR_STATE, "pnvo_train_attach first");
  TrainState *t = TS(m);
  if (t->embed_err && *t->embed_err) {
    *t->embed_err = 0;
    return pnvo_fail(m, PNVO_ERR_INPUT, "an action of the previous step was outside the embedding table");
  }
  t->actions = reinterpret_cast<const long long *>(actions);
  return PNVO_OK;
}

int pnvo_train_dropout_mask(pnvo_handle m, int layer, float *out, void *stream) {
  if (!m || !m->train) return pnvo_fail(m, PNVO_ERR_STATE, "pnvo_train_attach first");
  TrainState *t = TS(m);
  if (t->lastB <= 0 || !out || layer < 0 || layer > 2) return pnvo_fail(m, PNVO_ERR_ARG, "bad argument / no forward yet");
  const pnvo_config &c = m->cfg;
  const float p = t->drop_p;
  if (layer == 2)
    HIPCHK(m, launch_dropout(nullptr, nullptr, nullptr, t->lastB, 1, 32, p, t->drop_seed, t->drop_step, 2, out,
                             (hipStream_t)stream));
  else if (layer == 0)
    HIPCHK(m, launch_dropout(nullptr, nullptr, nullptr, t->lastB, (long)m->fh * m->fw, m->comp_cp, p, t->drop_seed,
                             t->drop_step, 0, out, (hipStream_t)stream));
  else
    HIPCHK(m, launch_dropout(nullptr, nullptr, nullptr, t->lastB, 1, c.hidden, p, t->drop_seed, t->drop_step, 1, out,
                             (hipStream_t)stream));
  return PNVO_OK;
}

int pnvo_input_moments(pnvo_handle m, const float *rgb, const float *depth, const float *dd, const float *tdv, int B,
                       const float *center, int power, float *out, void *stream) {
  if (!m || !m->train) return pnvo_fail(m, PNVO_ERR_STATE, "pnvo_train_attach first");
  if (!out || power < 1 || power > 3) return pnvo_fail(m, PNVO_ERR_ARG, "bad argument");
  HIPCHK(m, hipSetDevice(m->device));
  TrainState *t = TS(m);
  int rc = ensure_train_ws(m, t, B);
  if (rc != PNVO_OK) return rc;
  const pnvo_config &c = m->cfg;
  MomentsArgs a;
  std::memset(&a, 0, sizeof(a));
  a.src[0] = rgb;
  a.src[1] = depth;
  a.src[2] = dd;
  a.src[3] = tdv;
  a.nch[0] = c.n_rgb;
  a.nch[1] = c.n_depth;
  a.nch[2] = c.n_dd;
  a.nch[3] = c.n_tdv;
  for (int k = 0; k < m->CP; ++k) {
    const int r = m->stem_ref_of_new[k];
    if (r < 0) continue;
    a.tensor[r] = m->stem_tensor_of_new[k];
    a.ch[r] = m->stem_ch_of_new[k];
  }
  a.center = center;
  a.npix = (long)B * c.height * c.width;
  a.pw = power;
  HIPCHK(m, launch_moments(a, m->C, t->ws.mom_part, out, (hipStream_t)stream));
  return PNVO_OK;
}

// pnvo_input_moments from the sensor frames: one pass over the frames (moments_raw_partial_kernel) where the frame-reading kernels
// serve the handle, else the pair kernel on the materialised pairs (bit-equal to pnvo_input_moments on pnvo_build_obs_pairs' tensors).
int pnvo_input_moments_raw(pnvo_handle m, const uint8_t *rgb_frames, const float *depth_frames, const float *tdv, const float *edges, int B,
                           const float *center, int power, float *out, int32_t *err_flag, void *stream) {
  if (int rc0 = pnvo_check_frames(m, "pnvo_input_moments_raw", rgb_frames, depth_frames, tdv, B, out)) return rc0;
  if (!m->train) return pnvo_fail(m, PNVO_ERR_STATE, "pnvo_train_attach first");
  if (!depth_frames || power < 1 || power > 3) return pnvo_fail(m, PNVO_ERR_ARG, "bad argument");
  HIPCHK(m, hipSetDevice(m->device));
  const pnvo_config &c = m->cfg;
  if (!train_frames_direct(m)) {
    TrainState *t = TS(m);
    if (int rc = pnvo_raw_materialise(m, rgb_frames, depth_frames, B, edges, err_flag, (hipStream_t)stream, t->fpairs, &t->fpairs_cap)) return rc;
    return pnvo_input_moments(m, c.n_rgb ? t->fpairs[0] : nullptr, c.n_depth ? t->fpairs[1] : nullptr, c.n_dd ? t->fpairs[2] : nullptr, tdv, B,
                              center, power, out, stream);
  }
  TrainState *t = TS(m);
  int rc = ensure_train_ws(m, t, B);
  if (rc != PNVO_OK) return rc;
  MomentsRawArgs a;
  std::memset(&a, 0, sizeof(a));
  a.rgb = rgb_frames;
  a.depth = depth_frames;
  a.tdv = tdv;
  for (int &q : a.cof) q = -1;
  for (int k = 0; k < m->CP; ++k) {
    const int r = m->stem_ref_of_new[k];
    if (r < 0) continue;
    const int tn = m->stem_tensor_of_new[k], ch = m->stem_ch_of_new[k];
    a.cof[tn == 0 ? ch : tn == 1 ? 6 + ch : tn == 2 ? 8 + ch : 28 + ch] = r;
  }
  a.center = center;
  a.fpix = (long)c.height * c.width;
  a.npix = (long)B * a.fpix;
  a.pw = power;
  a.err_flag = err_flag;
  for (int i = 0; i < 12; ++i) a.edges[i] = i >= 10 ? 1.0f : edges != nullptr ? edges[i] : (float)((double)i * 1.0 / 10.0);
  if (edges != nullptr) a.edges[10] = edges[10];
  HIPCHK(m, launch_moments_raw(a, m->C, t->ws.mom_part, out, (hipStream_t)stream));
  return PNVO_OK;
}

int pnvo_rmv_merge(const float *m12, int C, int B, float *mean, float *var, float *count, void *stream) {
  if (!m12 || !mean || !var || !count || C < 1 || C > 1024 || B < 1) return PNVO_ERR_ARG;
  return launch_rmv_merge(m12, C, B, mean, var, count, (hipStream_t)stream) == hipSuccess ? PNVO_OK : PNVO_ERR_HIP;
}

int pnvo_mse_loss(const float *pred, const float *target, int B, int D, float *loss, float *grad, void *stream) {
  if (!pred || !target || B <= 0 || D <= 0) return pnvo_fail(nullptr, PNVO_ERR_ARG, "bad argument");
  HIPCHK(nullptr, launch_mse_loss(pred, target, B, D, loss, grad, (hipStream_t)stream));
  return PNVO_OK;
}

int pnvo_mse_loss_coef(const float *pred, const float *target, const float *coef, int n, float *loss, float *grad,
                       void *stream) {
  if (!pred || !target || !coef || n <= 0) return pnvo_fail(nullptr, PNVO_ERR_ARG, "bad argument");
  HIPCHK(nullptr, launch_mse_loss_coef(pred, target, coef, n, loss, grad, (hipStream_t)stream));
  return PNVO_OK;
}

int pnvo_geo_inverse_loss(const float *deltas, const int32_t *actions, int n_entries, int move_forward, float weight,
                          float *out4, float *grad, void *stream) {
  if (!deltas || !actions || n_entries <= 0 || (n_entries & 1))
    return pnvo_fail(nullptr, PNVO_ERR_ARG, "deltas must hold an even number of alternating (cur_rel_to_prev, prev_rel_to_cur) rows");
  HIPCHK(nullptr, launch_geo_inverse_loss(deltas, actions, n_entries / 2, move_forward, weight, out4, grad, (hipStream_t)stream));
  return PNVO_OK;
}

int pnvo_adam_step(float *p, const float *g, float *mom, float *var, size_t n, float lr, float beta1, float beta2, float eps,
                   int step, void *stream) {
  if (!p || !g || !mom || !var || step < 1) return pnvo_fail(nullptr, PNVO_ERR_ARG, "bad argument");
  HIPCHK(nullptr, launch_adam(p, g, mom, var, (long)n, lr, beta1, beta2, eps, step, (hipStream_t)stream));
  return PNVO_OK;
}

}  // extern "C"
