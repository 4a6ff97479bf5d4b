// pnvo_bf16.hip — host side of the native-bf16 forward (BASELINE config 3: the geometric-invariance dual forward in
// bf16).  pnvo_set_precision(h, 1) routes pnvo_forward here; pnvo_forward_dual runs TWO action models in every launch
// (blockIdx.z / the stem's second N-tile), the second one on the channel-swapped (cur, prev) pair that the reference's
// dataset builds for the opposite action (regression_geo_invariance_iter_dataset.py:342-386, engine :569-602) — here a
// permutation of that model's stem weights, so the observation tensors are read from HBM once for both models.
//
// Numerics: bf16 operands on the matrix cores, fp32 accumulation; activations are stored in bf16 (raw conv outputs,
// block outputs); GroupNorm statistics come from the fp32 accumulators and stay fp32 (scale/shift, whitening constants,
// the compression output, both Linear layers).  Kernels: stem_mx.hip (PIECES = 1), conv_bf16.hip, the fp32 split-K
// linear kernels of conv_mfma.hip for visual_fc / output_head.
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pnvo_model.h"

using namespace pnvo;

namespace {

struct BLayer {
  ConvBArgs plan;               // shape + tile plan (pointers filled per launch)
  int mw = 1, nw = 1;
  size_t lds = 0;
  DevBuf<unsigned short> wpk;
};

struct Bf16State {
  unsigned long long gen = 0;
  std::vector<BLayer> layers;   // parallel to m->convs (index 0 unused: the stem)
  DevBuf<unsigned short> stem_wpk;           // PIECES = 1 packing, one N-tile group (this model on (prev, cur))
  std::vector<unsigned short> stem_host, stem_host_sw;   // host copies: as is / for the swapped pair
  DevBuf<unsigned short> dual_stem;          // [tap][fragment][2 models][lane]: this model + a partner's swapped packing
  unsigned long long dual_partner = 0;       // process-unique id of the partner handle (an address can be re-used)
  unsigned long long dual_partner_gen = 0, dual_self_gen = 0;
  int cap = 0;
  DevBuf<unsigned short> stem_raw, bufY0, bufY1, rawA, rawB, rawD;
  DevBuf<float> comp_raw, hid, stats, stats_ds;   // stats_ds: partial sums of a riding downsample conv
  DevPair<float> ssA, ssB, ssD, ssC;
};

// Before a regrow: the old workspace goes first (not old and new side by side), and a failed regrow leaves cap = 0.
void free_ws(Bf16State *b) {
  for (DevBuf<unsigned short> *q : {&b->stem_raw, &b->bufY0, &b->bufY1, &b->rawA, &b->rawB, &b->rawD}) q->reset();
  for (DevBuf<float> *q : {&b->comp_raw, &b->hid, &b->stats, &b->stats_ds}) q->reset();
  for (DevPair<float> *q : {&b->ssA, &b->ssB, &b->ssD, &b->ssC}) q->reset();
  b->cap = 0;
}

int prepare(pnvo_handle m) {
  Bf16State *b = static_cast<Bf16State *>(m->bf);
  // The bf16 operands are packed from the host copies pnvo_load_weights took.  Parameters that moved on the device since
  // then (pnvo_adam_step + pnvo_train_refresh bump weights_gen) would silently evaluate as the pre-training weights.
  if (m->weights_gen != m->weights_gen_at_load)
    return pnvo_fail(m, PNVO_ERR_STATE, "the bfloat16 operands are built from the weights given to pnvo_load_weights, and the parameters "
                                        "have been updated on the device since (pnvo_train_refresh): call pnvo_load_weights with the "
                                        "current parameters before a bfloat16 forward");
  if (b && b->gen == m->load_gen) return PNVO_OK;
  const pnvo_config &c = m->cfg;
  if (m->bottleneck || c.baseplanes != 32 || !m->mx_ok || m->convs[0].cout != 32)
    return pnvo_fail(m, PNVO_ERR_ARG, "the bfloat16 path covers the resnet18 (BasicBlock, baseplanes 32) models");
  if (!b) {
    b = new Bf16State();
    m->bf = b;
  }
  if (b->layers.size() != m->convs.size()) b->layers = std::vector<BLayer>(m->convs.size());
  for (size_t li = 1; li < m->convs.size(); ++li) {
    const Layer &l = m->convs[li];
    BLayer &bl = b->layers[li];
    std::memset(&bl.plan, 0, sizeof(bl.plan));
    bl.plan.H = l.hin;
    bl.plan.W = l.win;
    bl.plan.CIN = rup(l.cin, 32);
    bl.plan.Ho = l.hout;
    bl.plan.Wo = l.wout;
    bl.plan.COUTP = l.coutp;
    if (!conv_bf16_plan(bl.plan, l.k, l.stride, &bl.mw, &bl.nw, &bl.lds))
      return pnvo_fail(m, PNVO_ERR_ARG, "layer '" + l.name + "' is outside the bfloat16 conv kernel's shapes");
    if (l.host_w.empty()) return pnvo_fail(m, PNVO_ERR_STATE, "weights of '" + l.name + "' were not loaded");
    std::vector<unsigned short> pk((size_t)l.k * l.kw * bl.plan.CIN * l.coutp);
    pack_conv_bf16_weight(l.host_w.data(), l.cout, l.cin, bl.plan.CIN, l.coutp, l.k, l.kw, pk.data());
    if (!bl.wpk) HIPCHK(m, bl.wpk.alloc(pk.size()));
    HIPCHK(m, hipMemcpy(bl.wpk, pk.data(), pk.size() * 2, hipMemcpyHostToDevice));
  }
  {
    const size_t n = stem_mx_packed_u16(1, 1);
    b->stem_host.resize(n);
    b->stem_host_sw.resize(n);
    pack_stem_mx_weight(m->mx_wk.data(), 32, 1, m->mx_xslot, b->stem_host.data());
    pack_stem_mx_weight(m->mx_wk_swapped.data(), 32, 1, m->mx_xslot, b->stem_host_sw.data());
    if (!b->stem_wpk) HIPCHK(m, b->stem_wpk.alloc(n));
    HIPCHK(m, hipMemcpy(b->stem_wpk, b->stem_host.data(), n * 2, hipMemcpyHostToDevice));
  }
  b->gen = m->load_gen;
  return PNVO_OK;
}

int ensure_ws(pnvo_handle m, int B) {
  Bf16State *b = static_cast<Bf16State *>(m->bf);
  if (B <= b->cap) return PNVO_OK;
  free_ws(b);
  const pnvo_config &c = m->cfg;
  size_t act = (size_t)B * m->Hp * m->Wp * c.baseplanes, st = (size_t)B * stem_mx_slots(m->Hs, m->Ws) * 32 * 2;
  int maxc = m->comp_cp;
  for (size_t li = 1; li < m->convs.size(); ++li) {
    const Layer &l = m->convs[li];
    act = std::max(act, (size_t)B * l.hout * l.wout * l.coutp);
    st = std::max(st, (size_t)B * b->layers[li].plan.slots * l.coutp * 2);
    maxc = std::max(maxc, l.coutp);
  }
  HIPCHK(m, b->stem_raw.alloc((size_t)B * m->Hs * m->Ws * 32));
  for (DevBuf<unsigned short> *q : {&b->bufY0, &b->bufY1, &b->rawA, &b->rawB, &b->rawD}) HIPCHK(m, q->alloc(act));
  HIPCHK(m, b->comp_raw.alloc((size_t)B * m->fh * m->fw * m->comp_cp));
  HIPCHK(m, b->hid.alloc((size_t)B * c.hidden));
  HIPCHK(m, b->stats.alloc(st));
  HIPCHK(m, b->stats_ds.alloc(st));
  for (int k = 0; k < 2; ++k) {
    HIPCHK(m, b->ssA.alloc(k, (size_t)B * maxc));
    HIPCHK(m, b->ssB.alloc(k, (size_t)B * maxc));
    HIPCHK(m, b->ssD.alloc(k, (size_t)B * maxc));
    HIPCHK(m, b->ssC.alloc(k, (size_t)B * m->comp_cp));
    HIPCHK(m, hipMemset(b->ssC[k], 0, (size_t)B * m->comp_cp * 4));      // pad channels stay (0, 0)
  }
  b->cap = B;
  return PNVO_OK;
}

// the stem's B operand for a dual launch: [tap][fragment][model 0 | model 1 on the swapped pair][lane]
int dual_stem(pnvo_handle m0, pnvo_handle m1) {
  Bf16State *b0 = static_cast<Bf16State *>(m0->bf), *b1 = static_cast<Bf16State *>(m1->bf);
  if (b0->dual_stem && b0->dual_partner == m1->uid && b0->dual_partner_gen == m1->load_gen && b0->dual_self_gen == m0->load_gen)
    return PNVO_OK;
  const size_t n1 = stem_mx_packed_u16(1, 1);            // 49 taps x 2 fragments x 512 u16
  std::vector<unsigned short> pk(2 * n1);
  for (size_t tf = 0; tf < n1 / 512; ++tf) {
    std::memcpy(&pk[(2 * tf) * 512], &b0->stem_host[tf * 512], 1024);
    std::memcpy(&pk[(2 * tf + 1) * 512], &b1->stem_host_sw[tf * 512], 1024);
  }
  if (!b0->dual_stem) HIPCHK(m0, b0->dual_stem.alloc(pk.size()));
  HIPCHK(m0, hipMemcpy(b0->dual_stem, pk.data(), pk.size() * 2, hipMemcpyHostToDevice));
  b0->dual_partner = m1->uid;
  b0->dual_partner_gen = m1->load_gen;
  b0->dual_self_gen = m0->load_gen;
  return PNVO_OK;
}

}  // namespace

void pnvo_bf16_free(pnvo_handle m) {
  delete static_cast<Bf16State *>(m->bf);
  m->bf = nullptr;
}

namespace {

typedef DevBuf<unsigned short> Bf16State::*Act;   // an activation buffer of the workspace, by name
typedef DevPair<float> Bf16State::*Gn;            // a GroupNorm scale / shift pair of it

// The one or two models of a forward.  The batched launches take per-model pointer arrays of two: with one model the second entry
// repeats the first (k).
struct Models {
  pnvo_handle *hs;
  Bf16State *bs[2];
  int nm;
  int k(int z) const { return z < nm ? z : 0; }
};

// One conv of the residual stages or the compression conv (a call site sets the members it uses, in this order).
struct ConvBRequest {
  Act x = nullptr;             // input
  Gn x_gn = nullptr;           // the producer's pair: relu(GN(x)) while staging
  Act skip = nullptr;          // with x_gn: the fused BasicBlock tail relu(GN2(x) + skip) computed while staging — skip is the block input
  Gn skip_gn = nullptr;        //   buffer, or with skip_gn the raw downsample conv (its GroupNorm applied in the fetch)
  Act xout = nullptr;          // where the stager writes that block output for the later readers, or none
  Act y = nullptr;             // raw output; nullptr: the float32 compression output comp_raw
  Gn y_gn = nullptr;           // pair of the GroupNorm that follows
  long ride = -1;              // >= 0: the layer index of the block's 1x1 stride-2 downsample conv, computed by this launch
                               //   (conv_bf16_kernel DSF): raw output -> rawD, GroupNorm -> ssD
};

// GroupNorm finalisation of layer li's partial sums in `stats` into `dst`, both models in one launch
int gn_finalize(const Models &M, int B, size_t li, DevBuf<float> Bf16State::*stats, int slots, Gn dst, hipStream_t s) {
  const Layer &l = M.hs[0]->convs[li];
  const float *st[2], *ga[2], *be[2];
  float *sc[2], *sh[2];
  for (int z = 0; z < 2; ++z) {
    const int k = M.k(z);
    st[z] = M.bs[k]->*stats;
    ga[z] = M.hs[k]->convs[li].gamma;
    be[z] = M.hs[k]->convs[li].beta;
    sc[z] = (M.bs[k]->*dst)[0];
    sh[z] = (M.bs[k]->*dst)[1];
  }
  HIPCHK(M.hs[0], launch_gn_finalize2(st, B, slots, l.coutp, l.cout, l.groups, (long)l.hout * l.wout, ga, be, 1e-5f, sc, sh, M.nm, s));
  return PNVO_OK;
}

// (a4-a7) fused stem, one N-tile per model, its GroupNorm, then GN + ReLU + maxpool -> bufY0
int stem_bf16(const Models &M, int B, const FwdRequest &r) {
  pnvo_handle m = M.hs[0];
  hipStream_t s = r.s;
  const Layer &stem = m->convs[0];
  const int nm = M.nm;
  int rc;
  {
    StemMXArgs a;
    std::memset(&a, 0, sizeof(a));
    pnvo_stem_mx_input(m, B, r.src, r.raw, a);                   // (pnvo_forward_raw: sensor frames instead of src[0..2])
    a.wpk = nm == 2 ? M.bs[0]->dual_stem : M.bs[0]->stem_wpk;
    for (int z = 0; z < nm; ++z) {
      a.y[z] = M.bs[z]->stem_raw;
      a.stats[z] = M.bs[z]->stats;
      a.y_coff[z] = 0;
    }
    a.y_cstride = 32;
    a.stats_cstride = 32;
    const double P = (double)B * m->Hs * m->Ws;
    {
      PnvoTimed t(m, s, "bf16:stem", 2.0 * nm * P * stem.cout * stem.cin * 49, pnvo_stem_in_bytes(m, B, r.raw) + 2.0 * nm * P * stem.cout);
      if ((rc = pnvo_launch_stem_mx(m, a, 1, nm, true, nullptr, s)) != PNVO_OK) return rc;
    }
    PnvoTimed t(m, s, "bf16:gn_finalize", 0.0, 0.0);
    if ((rc = gn_finalize(M, B, 0, &Bf16State::stats, a.slots, &Bf16State::ssA, s)) != PNVO_OK) return rc;
  }
  const unsigned short *x[2];
  const float *sc[2], *sh[2];
  unsigned short *o[2];
  for (int z = 0; z < 2; ++z) {
    const Bf16State *b = M.bs[M.k(z)];
    x[z] = b->stem_raw, sc[z] = b->ssA[0], sh[z] = b->ssA[1], o[z] = b->bufY0;
  }
  PnvoTimed t(m, s, "bf16:gn_relu_maxpool", 0.0, 2.0 * nm * B * ((double)m->Hs * m->Ws + (double)m->Hp * m->Wp) * 32);
  HIPCHK(m, launch_gn_relu_maxpool_bf16(x, sc, sh, B, m->Hs, m->Ws, 32, o, nm, s));
  return PNVO_OK;
}

// One conv + its GroupNorm finalisation (and its riding downsample conv's).  Stager mode 0: plain input; 1: relu(GN(x)) of the
// producer; 2: the block tail.
int run_conv_bf16(const Models &M, int B, size_t li, const ConvBRequest &q, hipStream_t s) {
  pnvo_handle m = M.hs[0];
  const Layer &l = m->convs[li];
  const BLayer &bl = M.bs[0]->layers[li];
  const int mode = q.skip ? 2 : q.x_gn ? 1 : 0, nm = M.nm;
  ConvBArgs a = bl.plan;
  a.B = B;
  a.persist_wgs = m->opt.x3_persist ? 3 * m->num_cus : 0;
  // one tile per sample (the 12 x 22 and 6 x 11 maps): the workgroup that sums a sample's channels finalises its GroupNorm too
  // (gn_finalize_lane: fp64, the butterfly order of the float32 path's fused finalisation) — one launch less per layer
  const int cpg = l.groups > 0 ? l.cout / l.groups : 0;
  const bool gfuse = m->opt.gn_fuse && a.slots == 1 && l.cout == l.coutp && cpg >= 1 && cpg <= 32 && 32 % cpg == 0 && l.cout % cpg == 0;
  for (int z = 0; z < 2; ++z) {
    const int k = M.k(z);
    const Bf16State *b = M.bs[k];
    a.x[z] = b->*q.x;
    a.wpk[z] = b->layers[li].wpk;
    a.y[z] = q.y ? (void *)(b->*q.y) : (void *)b->comp_raw;
    a.stats[z] = b->stats;
    a.in_scale[z] = q.x_gn ? (b->*q.x_gn)[0] : nullptr;
    a.in_shift[z] = q.x_gn ? (b->*q.x_gn)[1] : nullptr;
    a.x2[z] = q.skip ? (const unsigned short *)(b->*q.skip) : nullptr;
    a.in_scale2[z] = q.skip_gn ? (b->*q.skip_gn)[0] : nullptr;
    a.in_shift2[z] = q.skip_gn ? (b->*q.skip_gn)[1] : nullptr;
    a.xout[z] = q.xout ? (unsigned short *)(b->*q.xout) : nullptr;
    a.gn_gamma[z] = gfuse ? M.hs[k]->convs[li].gamma : nullptr;
    a.gn_beta[z] = gfuse ? M.hs[k]->convs[li].beta : nullptr;
    a.gn_scale[z] = gfuse ? (b->*q.y_gn)[0] : nullptr;
    a.gn_shift[z] = gfuse ? (b->*q.y_gn)[1] : nullptr;
    if (q.ride >= 0) {
      a.ds_wpk[z] = b->layers[q.ride].wpk;
      a.ds_y[z] = b->rawD;
      a.ds_stats[z] = b->stats_ds;
      a.ds_gamma[z] = gfuse ? M.hs[k]->convs[q.ride].gamma : nullptr;
      a.ds_beta[z] = gfuse ? M.hs[k]->convs[q.ride].beta : nullptr;
      a.ds_scale[z] = gfuse ? b->ssD[0] : nullptr;
      a.ds_shift[z] = gfuse ? b->ssD[1] : nullptr;
    }
  }
  a.gn_cpg = cpg;
  a.gn_eps = 1e-5f;
  a.gn_P = (long)l.hout * l.wout;
  const double macs = (double)B * l.hout * l.wout * l.cout * l.cin * l.k * l.kw;
  {
    PnvoTimed t(m, s, "bf16:conv:" + l.name, 2.0 * nm * macs,
                2.0 * nm * ((double)B * l.hin * l.win * l.cin * (mode == 2 ? 3 : 1) + (double)B * l.hout * l.wout * l.cout));
    HIPCHK(m, launch_conv_bf16(a, l.k, l.stride, mode, q.y == nullptr, bl.mw, bl.nw, bl.lds, nm, s));
  }
  if (gfuse) return PNVO_OK;
  PnvoTimed t(m, s, "bf16:gn_finalize", 0.0, 0.0);
  int rc = gn_finalize(M, B, li, &Bf16State::stats, a.slots, q.y_gn, s);
  // the riding downsample conv's GroupNorm (same geometry, its own sums and parameters)
  if (rc == PNVO_OK && q.ride >= 0) rc = gn_finalize(M, B, (size_t)q.ride, &Bf16State::stats_ds, a.slots, &Bf16State::ssD, s);
  return rc;
}

// What the block walk hands on: the buffer that holds (or, with a tail pending, will hold) the block output, and the tail of the last
// block where it is still to be applied — relu(GN2(rawB) + skip), the skip its block input or (skip_gn) its raw downsample conv.
struct WalkBf16 {
  Act cur = &Bf16State::bufY0, nxt = &Bf16State::bufY1;
  Act skip = nullptr;
  Gn skip_gn = nullptr;
};

// (a8) residual stages (BasicBlock: conv3x3(s) -> GN -> ReLU -> conv3x3 -> GN; + identity / conv1x1(s)+GN; ReLU).
// The tail of block k (GN2 + skip + ReLU) is not a pass of its own: conv1 of block k+1 (and the compression conv after
// the last block) computes it while staging its input patch and writes the block output for the later readers (the
// next skip branch / downsample conv).  PNVO_BF16_NOFUSE=1 keeps the separate residual kernel (A/B measurements).
int blocks_bf16(const Models &M, int B, WalkBf16 &w, hipStream_t s) {
  pnvo_handle m = M.hs[0];
  const int nm = M.nm;
  int rc;
  for (const Block &blk : m->blocks) {
    const size_t l1 = blk.conv[0], l2 = blk.conv[1];
    const bool ds = blk.ds >= 0;
    const Layer &c1 = m->convs[l1], &c2 = m->convs[l2];
    // the block's downsample conv rides on its first conv's launch (option ds_fuse); in the block-tail mode the block input is then
    // not written at all: both of its readers are that launch
    const bool ride_ok = ds && m->opt.ds_fuse && !w.skip_gn /* the stager would read rawD while the ride writes it */ &&
                         M.bs[0]->layers[l1].nw == 1 /* two N-tiles per wave: the second accumulator set does not fit (measured 56 -> 103 us) */ &&
                         c1.cinp != 32 /* 32 input channels: the resident-weight persistent form takes the head (140 + 39 us with the separate
                                          downsample conv against 235 us with the ride on the streaming form) */ &&
                         c1.k == 3 && c1.stride == 2 && m->convs[blk.ds].k == 1 && m->convs[blk.ds].stride == 2 &&
                         c1.cinp == m->convs[blk.ds].cinp && c1.coutp == m->convs[blk.ds].coutp && c1.hout == m->convs[blk.ds].hout &&
                         c1.wout == m->convs[blk.ds].wout && c1.groups == m->convs[blk.ds].groups;
    const long ride = ride_ok ? blk.ds : -1;
    if (w.skip) {                                // input = relu(GN2(rawB) + skip) of the previous block -> nxt
      rc = run_conv_bf16(M, B, l1, {.x = &Bf16State::rawB, .x_gn = &Bf16State::ssB, .skip = w.skip, .skip_gn = w.skip_gn,
                                    .xout = ride_ok ? nullptr : w.nxt, .y = &Bf16State::rawA, .y_gn = &Bf16State::ssA, .ride = ride}, s);
      std::swap(w.cur, w.nxt);
    } else {
      rc = run_conv_bf16(M, B, l1, {.x = w.cur, .y = &Bf16State::rawA, .y_gn = &Bf16State::ssA, .ride = ride}, s);
    }
    if (rc != PNVO_OK ||
        (rc = run_conv_bf16(M, B, l2, {.x = &Bf16State::rawA, .x_gn = &Bf16State::ssA, .y = &Bf16State::rawB, .y_gn = &Bf16State::ssB}, s)) != PNVO_OK)
      return rc;
    if (ds && !ride_ok && (rc = run_conv_bf16(M, B, blk.ds, {.x = w.cur, .y = &Bf16State::rawD, .y_gn = &Bf16State::ssD}, s)) != PNVO_OK) return rc;
    w.skip = ds ? &Bf16State::rawD : w.cur;
    w.skip_gn = ds ? &Bf16State::ssD : nullptr;
    if (m->opt.bf16_fuse) continue;
    const unsigned short *xa[2], *xb[2];
    const float *sa[2], *ta[2], *sb[2], *tb[2];
    unsigned short *y[2];
    for (int z = 0; z < 2; ++z) {
      const Bf16State *b = M.bs[M.k(z)];
      xa[z] = b->rawB, sa[z] = b->ssB[0], ta[z] = b->ssB[1], xb[z] = b->*w.skip, y[z] = b->*w.nxt;
      if (ds) sb[z] = b->ssD[0], tb[z] = b->ssD[1];
    }
    const long P = (long)c2.hout * c2.wout;
    PnvoTimed t(m, s, "bf16:residual", 0.0, 6.0 * nm * B * P * c2.coutp);
    HIPCHK(m, launch_residual_bf16(xa, sa, ta, xb, ds ? sb : nullptr, ds ? tb : nullptr, B, P, c2.coutp, y, nm, s));
    std::swap(w.cur, w.nxt);
    w.skip = nullptr, w.skip_gn = nullptr;
  }
  return PNVO_OK;
}

// (a11) Flatten + Linear + ReLU + output head: the fp32 split-K linear kernels on each model
int linears_bf16(const Models &M, int B, const FwdRequest &r, float *const *outs) {
  for (int z = 0; z < M.nm; ++z) {
    pnvo_handle h = M.hs[z];
    const pnvo_config &c = h->cfg;
    const Bf16State *b = M.bs[z];
    const int tm = h->timing;
    h->timing = 0;                                  // (their event records belong to the fp32 path's table)
    // (the output head rides on the hidden layer's split-K reduction when there is one: option head_fuse, as in the float32 forward)
    bool head_rode = false;
    const float *head_w = h->train != nullptr ? nullptr : h->head_w_plain;
    int rc = pnvo_run_conv(h, h->fc, B, {.x = b->comp_raw, .in_scale = b->ssC[0], .in_shift = b->ssC[1], .y = b->hid,
                                         .y_cstride = c.hidden, .bias = h->fc_bias, .bias_row = c.act_embed ? r.actions : nullptr, .relu_out = 1,
                                         .head_w = head_w, .head_out = (h->opt.head_fuse && c.out_dim <= 4 && head_w != nullptr) ? outs[z] : nullptr,
                                         .head_rode = &head_rode, .s = r.s});
    if (rc == PNVO_OK && !head_rode)
      rc = pnvo_run_conv(h, h->head, B, {.x = b->hid, .y = outs[z], .y_cstride = c.out_dim, .bias = h->head_bias, .s = r.s});
    h->timing = tm;
    if (rc != PNVO_OK) return z == 0 ? rc : pnvo_fail(M.hs[0], rc, h->err);
  }
  return PNVO_OK;
}

}  // namespace

int pnvo_forward_bf16(pnvo_handle *hs, int nm, int B, const FwdRequest &r, float *const *outs) {
  pnvo_handle m = hs[0];
  Models M{hs, {nullptr, nullptr}, nm};
  int rc;
  for (int z = 0; z < nm; ++z) {
    if ((rc = prepare(hs[z])) != PNVO_OK) return z == 0 ? rc : pnvo_fail(m, rc, hs[z]->err);
    M.bs[z] = static_cast<Bf16State *>(hs[z]->bf);
    if ((rc = ensure_ws(hs[z], B)) != PNVO_OK) return z == 0 ? rc : pnvo_fail(m, rc, hs[z]->err);
  }
  if (nm == 2 && (rc = dual_stem(hs[0], hs[1])) != PNVO_OK) return rc;
  WalkBf16 w;
  if ((rc = stem_bf16(M, B, r)) != PNVO_OK || (rc = blocks_bf16(M, B, w, r.s)) != PNVO_OK) return rc;
  // (a10) compression conv + GroupNorm(1, C): fp32 output for the Linear layers; a pending tail in its stager, the block output not written
  const ConvBRequest comp = w.skip ? ConvBRequest{.x = &Bf16State::rawB, .x_gn = &Bf16State::ssB, .skip = w.skip, .skip_gn = w.skip_gn, .y_gn = &Bf16State::ssC}
                                   : ConvBRequest{.x = w.cur, .y_gn = &Bf16State::ssC};
  if ((rc = run_conv_bf16(M, B, m->comp, comp, r.s)) != PNVO_OK) return rc;
  return linears_bf16(M, B, r, outs);
}
