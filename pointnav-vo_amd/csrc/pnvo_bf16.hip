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
  DevBuf<unsigned short> stem_raw, bufY[2], rawA, rawB, rawD;
  DevBuf<float> comp_raw, hid, stats, stats_ds;   // stats_ds: partial sums of a riding downsample conv
  DevPair<float> ssA, ssB, ssD, ssC;
};

// Before a regrow: the old workspace goes first (not old and new side by side), and a failed regrow leaves cap = 0.
void free_ws(Bf16State *b) {
  for (DevBuf<unsigned short> *q : {&b->stem_raw, &b->bufY[0], &b->bufY[1], &b->rawA, &b->rawB, &b->rawD}) q->reset();
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
  for (DevBuf<unsigned short> *q : {&b->bufY[0], &b->bufY[1], &b->rawA, &b->rawB, &b->rawD}) HIPCHK(m, q->alloc(act));
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

int pnvo_forward_bf16(pnvo_handle *hs, int nm, int B, const FwdRequest &r, float *const *outs) {
  pnvo_handle m = hs[0];
  hipStream_t s = r.s;
  Bf16State *bs[2] = {nullptr, nullptr};
  int rc;
  for (int z = 0; z < nm; ++z) {
    if ((rc = prepare(hs[z])) != PNVO_OK) return z == 0 ? rc : pnvo_fail(m, rc, hs[z]->err);
    bs[z] = static_cast<Bf16State *>(hs[z]->bf);
    if ((rc = ensure_ws(hs[z], B)) != PNVO_OK) return z == 0 ? rc : pnvo_fail(m, rc, hs[z]->err);
  }
  if (nm == 2 && (rc = dual_stem(hs[0], hs[1])) != PNVO_OK) return rc;
  const pnvo_config &c = m->cfg;
  const Layer &stem = m->convs[0];
  auto each = [&](auto f) {                       // per-model pointer arrays for the batched launches
    using T = decltype(f(0));
    struct R { T v[2]; } r;
    for (int z = 0; z < 2; ++z) r.v[z] = f(z < nm ? z : 0);
    return r;
  };

  // (a4-a6) fused stem, one N-tile per model
  {
    StemMXArgs a;
    std::memset(&a, 0, sizeof(a));
    pnvo_stem_mx_input(m, B, r.src, r.raw, a);                   // (pnvo_forward_raw: sensor frames instead of src[0..2])
    a.wpk = nm == 2 ? bs[0]->dual_stem : bs[0]->stem_wpk;
    for (int z = 0; z < nm; ++z) {
      a.y[z] = bs[z]->stem_raw;
      a.stats[z] = bs[z]->stats;
      a.y_coff[z] = 0;
    }
    a.y_cstride = 32;
    a.stats_cstride = 32;
    const double M = (double)B * m->Hs * m->Ws;
    {
      PnvoTimed t(m, s, "bf16:stem", 2.0 * nm * M * stem.cout * stem.cin * 49, pnvo_stem_in_bytes(m, B, r.raw) + 2.0 * nm * M * stem.cout);
      if ((rc = pnvo_launch_stem_mx(m, a, 1, nm, true, nullptr, s)) != PNVO_OK) return rc;
    }
    PnvoTimed t(m, s, "bf16:gn_finalize", 0.0, 0.0);
    auto st = each([&](int z) { return (const float *)bs[z]->stats; });
    auto ga = each([&](int z) { return (const float *)hs[z]->convs[0].gamma; });
    auto be = each([&](int z) { return (const float *)hs[z]->convs[0].beta; });
    auto sc = each([&](int z) { return bs[z]->ssA[0]; });
    auto sh = each([&](int z) { return bs[z]->ssA[1]; });
    HIPCHK(m, launch_gn_finalize2(st.v, B, a.slots, 32, 32, stem.groups, (long)m->Hs * m->Ws, ga.v, be.v, 1e-5f, sc.v, sh.v, nm, s));
  }
  // (a7) GN + ReLU + maxpool
  int cur = 0;
  {
    auto x = each([&](int z) { return (const unsigned short *)bs[z]->stem_raw; });
    auto sc = each([&](int z) { return (const float *)bs[z]->ssA[0]; });
    auto sh = each([&](int z) { return (const float *)bs[z]->ssA[1]; });
    auto o = each([&](int z) -> unsigned short * { return bs[z]->bufY[0]; });
    PnvoTimed t(m, s, "bf16:gn_relu_maxpool", 0.0, 2.0 * nm * B * ((double)m->Hs * m->Ws + (double)m->Hp * m->Wp) * 32);
    HIPCHK(m, launch_gn_relu_maxpool_bf16(x.v, sc.v, sh.v, B, m->Hs, m->Ws, 32, o.v, nm, s));
  }

  // one conv of the residual stages + its GroupNorm finalisation.  mode 0: plain input; 1: relu(GN(x)) of the producer
  // (ssA); 2: the fused BasicBlock tail relu(GN2(rawB) + skip) — computed while staging and written to `xout`
  struct Skip {
    bool on = false, affine = false;     // affine: the skip branch is the raw downsample conv (GN applied in the fetch)
    int buf = 0;                         // else: the block input bufY[buf]
  };
  const bool fuse = m->opt.bf16_fuse != 0;
  // ride (>= 0): the layer index of the block's 1x1 stride-2 downsample conv, computed by this launch (conv_bf16_kernel DSF): raw output ->
  // rawD, GroupNorm -> ssD
  auto conv = [&](size_t li, int mode, auto xin, auto yout, int ss_sel /*0 A, 1 B, 2 D, 3 C*/, bool f32out, const Skip &sk,
                  int out_buf, long ride = -1) -> int {
    const Layer &l = m->convs[li];
    ConvBArgs a = bs[0]->layers[li].plan;
    a.B = B;
    a.persist_wgs = m->opt.x3_persist ? 3 * m->num_cus : 0;
    for (int z = 0; z < 2; ++z) {
      const int k = z < nm ? z : 0;
      a.x[z] = xin(k);
      a.wpk[z] = bs[k]->layers[li].wpk;
      a.y[z] = yout(k);
      a.stats[z] = bs[k]->stats;
      a.in_scale[z] = mode == 1 ? bs[k]->ssA[0] : mode == 2 ? bs[k]->ssB[0] : nullptr;
      a.in_shift[z] = mode == 1 ? bs[k]->ssA[1] : mode == 2 ? bs[k]->ssB[1] : nullptr;
      a.x2[z] = mode == 2 ? (sk.affine ? bs[k]->rawD : bs[k]->bufY[sk.buf]) : nullptr;
      a.in_scale2[z] = mode == 2 && sk.affine ? bs[k]->ssD[0] : nullptr;
      a.in_shift2[z] = mode == 2 && sk.affine ? bs[k]->ssD[1] : nullptr;
      a.xout[z] = mode == 2 && out_buf >= 0 ? bs[k]->bufY[out_buf] : nullptr;
      if (ride >= 0) {
        a.ds_wpk[z] = bs[k]->layers[ride].wpk;
        a.ds_y[z] = bs[k]->rawD;
        a.ds_stats[z] = bs[k]->stats_ds;
      }
    }
    // one tile per sample (the 12 x 22 and 6 x 11 maps): the workgroup that sums a sample's channels finalises its GroupNorm too
    // (gn_finalize_lane: fp64, the butterfly order of the float32 path's fused finalisation) — one launch less per layer
    const int cpg = l.groups > 0 ? l.cout / l.groups : 0;
    const bool gfuse = m->opt.gn_fuse && a.slots == 1 && l.cout == l.coutp && cpg >= 1 && cpg <= 32 && 32 % cpg == 0 && l.cout % cpg == 0;
    auto ssof = [&](int z) -> float *const * { return ss_sel == 0 ? bs[z]->ssA : ss_sel == 1 ? bs[z]->ssB : ss_sel == 2 ? bs[z]->ssD : bs[z]->ssC; };
    for (int z = 0; z < 2; ++z) {
      const int k = z < nm ? z : 0;
      a.gn_gamma[z] = gfuse ? hs[k]->convs[li].gamma : nullptr;
      a.gn_beta[z] = gfuse ? hs[k]->convs[li].beta : nullptr;
      a.gn_scale[z] = gfuse ? ssof(k)[0] : nullptr;
      a.gn_shift[z] = gfuse ? ssof(k)[1] : nullptr;
      if (ride >= 0) {
        a.ds_gamma[z] = gfuse ? hs[k]->convs[ride].gamma : nullptr;
        a.ds_beta[z] = gfuse ? hs[k]->convs[ride].beta : nullptr;
        a.ds_scale[z] = gfuse ? bs[k]->ssD[0] : nullptr;
        a.ds_shift[z] = gfuse ? bs[k]->ssD[1] : nullptr;
      }
    }
    a.gn_cpg = cpg;
    a.gn_eps = 1e-5f;
    a.gn_P = (long)l.hout * l.wout;
    const double macs = (double)B * l.hout * l.wout * l.cout * l.cin * l.k * l.kw;
    {
      PnvoTimed t(m, s, "bf16:conv:" + l.name, 2.0 * nm * macs,
                  2.0 * nm * ((double)B * l.hin * l.win * l.cin * (mode == 2 ? 3 : 1) + (double)B * l.hout * l.wout * l.cout));
      HIPCHK(m, launch_conv_bf16(a, l.k, l.stride, mode, f32out, bs[0]->layers[li].mw, bs[0]->layers[li].nw, bs[0]->layers[li].lds,
                                 nm, s));
    }
    if (gfuse) return PNVO_OK;
    PnvoTimed t(m, s, "bf16:gn_finalize", 0.0, 0.0);
    auto st = each([&](int z) { return (const float *)bs[z]->stats; });
    auto ga = each([&](int z) { return (const float *)hs[z]->convs[li].gamma; });
    auto be = each([&](int z) { return (const float *)hs[z]->convs[li].beta; });
    auto sc = each([&](int z) { return ssof(z)[0]; });
    auto sh = each([&](int z) { return ssof(z)[1]; });
    HIPCHK(m, launch_gn_finalize2(st.v, B, a.slots, l.coutp, l.cout, l.groups, (long)l.hout * l.wout, ga.v, be.v, 1e-5f, sc.v, sh.v,
                                  nm, s));
    if (ride >= 0) {                     // the riding downsample conv's GroupNorm (same geometry, its own sums and parameters)
      auto std_ = each([&](int z) { return (const float *)bs[z]->stats_ds; });
      auto gad = each([&](int z) { return (const float *)hs[z]->convs[ride].gamma; });
      auto bed = each([&](int z) { return (const float *)hs[z]->convs[ride].beta; });
      auto scd = each([&](int z) { return bs[z]->ssD[0]; });
      auto shd = each([&](int z) { return bs[z]->ssD[1]; });
      HIPCHK(m, launch_gn_finalize2(std_.v, B, a.slots, l.coutp, l.cout, l.groups, (long)l.hout * l.wout, gad.v, bed.v, 1e-5f, scd.v, shd.v,
                                    nm, s));
    }
    return PNVO_OK;
  };

  // (a8) residual stages (BasicBlock: conv3x3(s) -> GN -> ReLU -> conv3x3 -> GN; + identity / conv1x1(s)+GN; ReLU).
  // The tail of block k (GN2 + skip + ReLU) is not a pass of its own: conv1 of block k+1 (and the compression conv after
  // the last block) computes it while staging its input patch and writes the block output for the later readers (the
  // next skip branch / downsample conv).  PNVO_BF16_NOFUSE=1 keeps the separate residual kernel (A/B measurements).
  Skip pend;                                       // tail of the previous block, still to be applied
  const Skip none;
  for (const Block &blk : m->blocks) {
    const size_t l1 = blk.conv[0], l2 = blk.conv[1];
    const bool ds = blk.ds >= 0;
    const Layer &c2 = m->convs[l2];
    // the block's downsample conv rides on its first conv's launch (option ds_fuse); in the block-tail mode the block input is then
    // not written at all: both of its readers are that launch
    const Layer &c1 = m->convs[l1];
    const bool ride_ok = ds && m->opt.ds_fuse && !(pend.on && pend.affine) /* the stager would read rawD while the ride writes it */ &&
                         bs[0]->layers[l1].nw == 1 /* two N-tiles per wave: the second accumulator set does not fit (measured 56 -> 103 us) */ &&
                         c1.cinp != 32 /* 32 input channels: the resident-weight persistent form takes the head (140 + 39 us with the separate
                                          downsample conv against 235 us with the ride on the streaming form) */ &&
                         c1.k == 3 && c1.stride == 2 && m->convs[blk.ds].k == 1 && m->convs[blk.ds].stride == 2 &&
                         c1.cinp == m->convs[blk.ds].cinp && c1.coutp == m->convs[blk.ds].coutp && c1.hout == m->convs[blk.ds].hout &&
                         c1.wout == m->convs[blk.ds].wout && c1.groups == m->convs[blk.ds].groups;
    const long ride = ride_ok ? blk.ds : -1;
    if (pend.on) {                               // input = relu(GN2(rawB) + skip) of the previous block -> bufY[cur ^ 1]
      if ((rc = conv(l1, 2, [&](int z) { return (const unsigned short *)bs[z]->rawB; }, [&](int z) { return (void *)bs[z]->rawA; }, 0,
                     false, pend, ride_ok ? -1 : (cur ^ 1), ride)) != PNVO_OK)
        return rc;
      cur ^= 1;
    } else if ((rc = conv(l1, 0, [&](int z) { return (const unsigned short *)bs[z]->bufY[cur]; },
                          [&](int z) { return (void *)bs[z]->rawA; }, 0, false, none, -1, ride)) != PNVO_OK) {
      return rc;
    }
    if ((rc = conv(l2, 1, [&](int z) { return (const unsigned short *)bs[z]->rawA; }, [&](int z) { return (void *)bs[z]->rawB; }, 1,
                   false, none, -1)) != PNVO_OK)
      return rc;
    const long P = (long)c2.hout * c2.wout;
    if (ds && !ride_ok && (rc = conv(blk.ds, 0, [&](int z) { return (const unsigned short *)bs[z]->bufY[cur]; },
                                     [&](int z) { return (void *)bs[z]->rawD; }, 2, false, none, -1)) != PNVO_OK)
      return rc;
    if (fuse) {
      pend.on = true;
      pend.affine = ds;
      pend.buf = cur;
      continue;
    }
    auto a_ = each([&](int z) { return (const unsigned short *)bs[z]->rawB; });
    auto sa = each([&](int z) { return (const float *)bs[z]->ssB[0]; });
    auto ta = each([&](int z) { return (const float *)bs[z]->ssB[1]; });
    auto y_ = each([&](int z) -> unsigned short * { return bs[z]->bufY[cur ^ 1]; });
    if (ds) {
      auto b_ = each([&](int z) { return (const unsigned short *)bs[z]->rawD; });
      auto sb = each([&](int z) { return (const float *)bs[z]->ssD[0]; });
      auto tb = each([&](int z) { return (const float *)bs[z]->ssD[1]; });
      PnvoTimed t(m, s, "bf16:residual", 0.0, 6.0 * nm * B * P * c2.coutp);
      HIPCHK(m, launch_residual_bf16(a_.v, sa.v, ta.v, b_.v, sb.v, tb.v, B, P, c2.coutp, y_.v, nm, s));
    } else {
      auto b_ = each([&](int z) { return (const unsigned short *)bs[z]->bufY[cur]; });
      PnvoTimed t(m, s, "bf16:residual", 0.0, 6.0 * nm * B * P * c2.coutp);
      HIPCHK(m, launch_residual_bf16(a_.v, sa.v, ta.v, b_.v, nullptr, nullptr, B, P, c2.coutp, y_.v, nm, s));
    }
    cur ^= 1;
  }
  // (a10) compression conv + GroupNorm(1, C): fp32 output for the Linear layers
  if (pend.on) {
    if ((rc = conv(m->comp, 2, [&](int z) { return (const unsigned short *)bs[z]->rawB; }, [&](int z) { return (void *)bs[z]->comp_raw; }, 3,
                   true, pend, -1)) != PNVO_OK)
      return rc;
  } else if ((rc = conv(m->comp, 0, [&](int z) { return (const unsigned short *)bs[z]->bufY[cur]; },
                        [&](int z) { return (void *)bs[z]->comp_raw; }, 3, true, none, -1)) != PNVO_OK) {
    return rc;
  }
  // (a11) Flatten + Linear + ReLU + output head: the fp32 split-K linear kernels on each model
  for (int z = 0; z < nm; ++z) {
    pnvo_handle h = hs[z];
    const int tm = h->timing;
    h->timing = 0;                                  // (their event records belong to the fp32 path's table)
    // (the output head rides on the hidden layer's split-K reduction when there is one: option head_fuse, as in the float32 forward)
    bool head_rode = false;
    const float *head_w = h->train != nullptr ? nullptr : h->head_w_plain;
    rc = pnvo_run_conv(h, h->fc, B, {.x = bs[z]->comp_raw, .in_scale = bs[z]->ssC[0], .in_shift = bs[z]->ssC[1], .y = bs[z]->hid,
                                     .y_cstride = c.hidden, .bias = h->fc_bias, .bias_row = c.act_embed ? r.actions : nullptr, .relu_out = 1,
                                     .head_w = head_w, .head_out = (h->opt.head_fuse && c.out_dim <= 4 && head_w != nullptr) ? outs[z] : nullptr,
                                     .head_rode = &head_rode, .s = s});
    if (rc == PNVO_OK && !head_rode)
      rc = pnvo_run_conv(h, h->head, B, {.x = bs[z]->hid, .y = outs[z], .y_cstride = c.out_dim, .bias = h->head_bias, .s = s});
    h->timing = tm;
    if (rc != PNVO_OK) return z == 0 ? rc : pnvo_fail(m, rc, h->err);
  }
  return PNVO_OK;
}
