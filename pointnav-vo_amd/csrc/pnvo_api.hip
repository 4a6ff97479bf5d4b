// pnvo_api.hip — the C ABI of include/pnvo.h: model construction, state_dict import, forward orchestration.
// Host-side only; every kernel lives in conv_mfma.hip / elementwise.hip.  gfx950 only, no fallbacks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <atomic>
#include <condition_variable>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "pnvo_model.h"

using namespace pnvo;

thread_local std::string g_err;

int pnvo_fail(pnvo_handle h, int code, const std::string &msg) {
  if (h) h->err = msg;
  g_err = msg;
  return code;
}

long long pnvo_device_bytes_live(void) { return g_device_bytes_live.load(); }

namespace {

inline int fail(pnvo_handle h, int code, const std::string &msg) { return pnvo_fail(h, code, msg); }


Layer make_layer(const std::string &name, const std::string &gn, int cin, int cout, int k, int stride, int pad,
                 int hin, int win, int groups) {
  Layer l;
  l.name = name;
  l.gn = gn;
  l.cin = cin;
  l.cinp = rup(cin, 8);
  l.cout = cout;
  l.coutp = rup(cout, 32);
  l.k = l.kw = k;
  l.stride = stride;
  l.pad = pad;
  l.hin = hin;
  l.win = win;
  l.hout = (hin + 2 * pad - k) / stride + 1;
  l.wout = (win + 2 * pad - k) / stride + 1;
  l.groups = groups;
  return l;
}

// Mirrors ResNet.__init__/_make_layer (resnet.py:153-212) and ResNetEncoder.__init__ (vo_cnn.py:70-101).
void build_plan(pnvo_model_s *m) {
  const pnvo_config &c = m->cfg;
  m->C = c.n_rgb + c.n_depth + c.n_dd + c.n_tdv;
  m->CP = rup(m->C, 8);
  m->CPL = rup(m->C, 16);
  m->Hs = halve(c.height);
  m->Ws = halve(c.width);
  m->Hp = halve(m->Hs);
  m->Wp = halve(m->Ws);
  {
    // reference order: [prev_rgb, prev_d, prev_dd, prev_tdv, cur_rgb, cur_d, cur_dd, cur_tdv]; tensor t holds
    // [prev half | cur half] on its channel axis (vo_cnn.py:114-174)
    const int n[4] = {c.n_rgb, c.n_depth, c.n_dd, c.n_tdv};
    int prev_off[4], half = 0;
    for (int t = 0; t < 4; ++t) {
      prev_off[t] = half;
      half += n[t] / 2;
    }
    m->stem_ref_of_new.clear();
    m->stem_tensor_of_new.clear();
    m->stem_ch_of_new.clear();
    for (int t = 0; t < 4; ++t)
      for (int ch = 0; ch < n[t]; ++ch) {
        const int hn = n[t] / 2;
        m->stem_ref_of_new.push_back(ch < hn ? prev_off[t] + ch : half + prev_off[t] + (ch - hn));
        m->stem_tensor_of_new.push_back(t);
        m->stem_ch_of_new.push_back(ch);
      }
    while ((int)m->stem_ref_of_new.size() < m->CP) {
      m->stem_ref_of_new.push_back(-1);
      m->stem_tensor_of_new.push_back(-1);
      m->stem_ch_of_new.push_back(0);
    }
  }
  const int g = c.baseplanes / 2;
  const std::string bb = "visual_encoder.backbone.";
  m->convs.clear();
  m->convs.push_back(make_layer(bb + "conv1.0", bb + "conv1.1", m->C, c.baseplanes, 7, 2, 3, c.height, c.width, g));
  int h = m->Hp, w = m->Wp, cin = c.baseplanes;
  const bool bott = c.backbone_depth == 50 || c.backbone_depth == 101;
  const int nblk[4] = {bott ? 3 : 2, bott ? 4 : 2, bott ? (c.backbone_depth == 101 ? 23 : 6) : 2, bott ? 3 : 2};
  // ResNeXtBottleneck / SEResNeXtBottleneck (resnet.py:143-150,172-173): expansion 2 on doubled stage planes, cardinality baseplanes / 2
  const bool resnext = bott && c.resnext != 0, se = bott && c.se != 0;
  const int expansion = resnext ? 2 : 4, cardinality = resnext ? c.baseplanes / 2 : 1;
  m->bottleneck = bott;
  m->grouped_se = resnext || se;
  m->blocks.clear();
  auto push = [&](Layer l) {                         // a conv of the block under construction
    l.block = (int)m->blocks.size();
    m->convs.push_back(std::move(l));
    return (int)m->convs.size() - 1;
  };
  for (int st = 1; st <= 4; ++st) {
    const int planes = (resnext ? 2 * c.baseplanes : c.baseplanes) << (st - 1), cout = bott ? planes * expansion : planes;
    for (int bi = 0; bi < nblk[st - 1]; ++bi) {
      Block b;
      b.stage = st;
      b.index = bi;
      b.tap = "layer" + std::to_string(st) + "." + std::to_string(bi);
      const std::string p = bb + b.tap + ".";
      const int stride = (st > 1 && bi == 0) ? 2 : 1;
      if (bott) {                                    // Bottleneck: 1x1 -> 3x3 (stride) -> 1x1 (x4), resnet.py:58-69
        Layer b2 = make_layer(p + "convs.3", p + "convs.4", planes, planes, 3, stride, 1, h, w, g);
        b.nconv = 3;
        b.conv[0] = push(make_layer(p + "convs.0", p + "convs.1", cin, planes, 1, 1, 0, h, w, g));
        if (bi == 0) b2.cgroups = cardinality;       // _make_layer hands the cardinality to the first block of a stage only (resnet.py:198-210)
        const int h2 = b2.hout, w2 = b2.wout;
        b.conv[1] = push(std::move(b2));
        if (se) b.se_r = cout / 16;                  // SE(planes * expansion, r = 16): int(planes / r), resnet.py:72-80
        b.conv[2] = push(make_layer(p + "convs.6", p + "convs.7", planes, cout, 1, 1, 0, h2, w2, g));
      } else {
        Layer c1 = make_layer(p + "convs.0", p + "convs.1", cin, planes, 3, stride, 1, h, w, g);
        b.nconv = 2;
        const int h1 = c1.hout, w1 = c1.wout;
        b.conv[0] = push(std::move(c1));
        b.conv[1] = push(make_layer(p + "convs.3", p + "convs.4", planes, planes, 3, 1, 1, h1, w1, g));
      }
      if (stride != 1 || cin != cout) b.ds = push(make_layer(p + "downsample.0", p + "downsample.1", cin, cout, 1, stride, 0, h, w, g));
      m->blocks.push_back(std::move(b));
      h = m->last(m->blocks.back()).hout;
      w = m->last(m->blocks.back()).wout;
      cin = cout;
    }
  }
  m->fh = h;
  m->fw = w;
  m->comp_c = (int)std::lround((double)c.flat_size / (double)(h * w));   // vo_cnn.py:82-84 (python round)
  {
    // python round() is banker's rounding; replicate for exact .5 cases
    const double q = (double)c.flat_size / (double)(h * w);
    const double fl = std::floor(q);
    if (q - fl == 0.5) m->comp_c = ((long)fl % 2 == 0) ? (int)fl : (int)fl + 1;
  }
  m->comp_cp = rup(m->comp_c, 32);
  m->comp = (int)m->convs.size();
  m->convs.push_back(make_layer("visual_encoder.compression.0", "visual_encoder.compression.1", cin, m->comp_c, 3, 1, 1,
                                h, w, 1));
  // Linear(flat -> hidden) as a valid (pad 0) fh x fw "conv" over the channel-padded compression map
  m->fc = make_layer(c.act_embed ? "hidden_generator.1" : "visual_fc.2", "", m->comp_c, c.hidden, 1, 1, 0, h, w, 1);
  m->fc.cinp = m->comp_cp;
  m->fc.k = h;
  m->fc.kw = w;
  m->fc.hout = m->fc.wout = 1;
  m->head = make_layer("output_head.1", "", c.hidden, c.out_dim, 1, 1, 0, 1, 1, 1);
}

struct Toc {
  std::map<std::string, const pnvo_tensor_desc *> by_name;
  const float *blob;
  size_t n;
};

const float *find_tensor(pnvo_handle h, const Toc &t, const std::string &name, std::vector<int64_t> shape, int *rc) {
  auto it = t.by_name.find(name);
  if (it == t.by_name.end()) {
    *rc = fail(h, PNVO_ERR_WEIGHTS, "state_dict is missing tensor '" + name + "'");
    return nullptr;
  }
  const pnvo_tensor_desc *d = it->second;
  size_t cnt = 1;
  bool ok = d->ndim == (int)shape.size();
  for (int k = 0; ok && k < d->ndim; ++k) {
    ok = d->shape[k] == shape[k];
    cnt *= (size_t)d->shape[k];
  }
  if (!ok || d->offset + cnt > t.n) {
    std::string s = "tensor '" + name + "' has the wrong shape (want [";
    for (auto v : shape) s += std::to_string(v) + ",";
    s += "])";
    *rc = fail(h, PNVO_ERR_WEIGHTS, s);
    return nullptr;
  }
  return t.blob + d->offset;
}

}  // namespace

// pack with an explicit padded input-channel count (the FC reads a channel-padded activation)
void pnvo_pack_conv_weight_cinp(const float *oihw, int cout, int cin, int cinp, int kh, int kw, std::vector<float> &out) {
  const int coutp = rup(cout, 32), J = cinp / 8, T = kh * kw, ntg_n = coutp / 32;
  out.assign((size_t)coutp * cinp * T, 0.f);
  for (int ntg = 0; ntg < ntg_n; ++ntg)
    for (int tap = 0; tap < T; ++tap)
      for (int j = 0; j < J; ++j)
        for (int hh = 0; hh < 2; ++hh)
          for (int n = 0; n < 32; ++n)
            for (int t = 0; t < 4; ++t) {
              const int co = ntg * 32 + n, ci = 8 * j + 4 * hh + t;
              if (co < cout && ci < cin)
                out[((((size_t)ntg * T + tap) * J + j) * 64 + hh * 32 + n) * 4 + t] =
                    oihw[((size_t)co * cin + ci) * T + tap];
            }
}

namespace {
inline void pack_conv_weight_cinp(const float *oihw, int cout, int cin, int cinp, int kh, int kw, std::vector<float> &out) {
  pnvo_pack_conv_weight_cinp(oihw, cout, cin, cinp, kh, kw, out);
}

int load_conv(pnvo_handle h, const Toc &t, Layer &l, bool has_gn) {
  int rc = PNVO_OK;
  const float *w = find_tensor(h, t, l.name + ".weight", {l.cout, l.cin / l.cgroups, l.k, l.kw}, &rc);
  if (!w) return rc;
  if (l.cgroups > 1) {                 // grouped conv [cout, cin / groups, 3, 3]: conv_group.hip's operand, and no other kernel's
    const int cg = l.cin / l.cgroups;
    if (l.cin != l.cout || !conv_group_supported(l.cout, cg, l.k, l.stride, l.pad))
      return fail(h, PNVO_ERR_ARG, "grouped conv " + l.name + ": unsupported geometry (" + std::to_string(l.cout) + " channels in groups of " +
                                       std::to_string(cg) + ")");
    std::vector<float> pk(conv_group_packed_floats(l.cout, cg));
    pack_conv_group_weight(w, l.cout, cg, pk.data());
    HIPCHK(h, l.wpk_grp.upload(pk.data(), pk.size()));
  } else {
    std::vector<float> pk;
    pack_conv_weight_cinp(w, l.cout, l.cin, l.cinp, l.k, l.kw, pk);
    HIPCHK(h, l.wpk.upload(pk.data(), pk.size()));
    l.host_w.assign(w, w + (size_t)l.cout * l.cin * l.k * l.kw);
  }
  if (has_gn) {
    const float *g = find_tensor(h, t, l.gn + ".weight", {l.cout}, &rc);
    if (!g) return rc;
    const float *b = find_tensor(h, t, l.gn + ".bias", {l.cout}, &rc);
    if (!b) return rc;
    HIPCHK(h, l.gamma.upload(g, l.cout));
    HIPCHK(h, l.beta.upload(b, l.cout));
  }
  return PNVO_OK;
}

// The input-contract flag of the fused stems and its host-mapped copy, lowered (pnvo_load_weights).
int reset_contract_flag(pnvo_handle h) {
  if (!h->dd_flag) HIPCHK(h, h->dd_flag.alloc_host(1, hipHostMallocMapped | hipHostMallocCoherent));
  if (!h->dd_flag_dev) HIPCHK(h, h->dd_flag_dev.alloc(1));
  *(volatile int *)h->dd_flag = 0;
  HIPCHK(h, hipMemset(h->dd_flag_dev, 0, sizeof(int)));
  return PNVO_OK;
}

// Before a regrow: the old workspace goes first (not old and new side by side), and a failed regrow leaves cap = 0.
void free_workspace(pnvo_model_s *m) {
  pnvo_drop_graphs(m);            // captured kernel arguments point into the workspace
  for (DevBuf<float> *b : {&m->xin, &m->stem_raw, &m->out_ws, &m->bufY[0], &m->bufY[1], &m->rawA, &m->rawB, &m->rawD, &m->rawC, &m->comp_raw,
                           &m->hid, &m->stats, &m->stats_ds, &m->tapbuf})
    b->reset();
  for (DevPair<float> *q : {&m->ssA, &m->ssB, &m->ssD, &m->ssC, &m->ssE}) q->reset();
  m->cap = 0;
}

// 3x3 (stride 1 or 2, pad 1) GroupNorm-ed convs run on conv_x3.hip unless option `conv` selects another kernel family
bool x3_layer(const PnvoOptions &o, const Layer &l) {
  const bool s2 = l.stride == 2 && o.x3_s2;
  const bool k3 = l.k == 3 && l.kw == 3 && l.pad == 1 && (l.stride == 1 || s2);
  const bool k1 = l.k == 1 && l.kw == 1 && l.pad == 0 && s2;      // the 1x1 stride-2 downsample convs (resnet.py:192-195)
  return (k3 || k1) && l.cgroups == 1 && !l.host_w.empty() && o.conv <= 1;
}
// operand pieces of conv_x3: two float16 pieces (three product terms) when the layer's input is provably inside float16's range and
// option pieces (train_pieces with a training step attached, whose device-side re-pack needs the weight's scale) asks for them;
// three bf16 pieces (six exact terms) otherwise
bool x3_two_pieces(pnvo_handle m, const Layer &l) {
  if (m->bottleneck || !(l.in_bound < 6.0e4f)) return false;
  if (m->train != nullptr)             // a training step is attached: operands are rebuilt on the device from the flat parameters
    return m->opt.train_pieces == 2 && pnvo_train_x2_scale(m, l) != nullptr;
  return m->opt.pieces == 2;
}
// Layer l at B samples as a problem of the float32-MFMA kernels under options o: the shape and the plan options — a plain conv with
// a dense output and nothing else asked; the caller states the rest.
ConvFp32Problem fp32_problem(pnvo_handle m, const PnvoOptions &o, const Layer &l, int B, int y_cstride) {
  ConvFp32Problem q{.B = B, .H = l.hin, .W = l.win, .CIN = l.cinp, .Ho = l.hout, .Wo = l.wout, .COUT = l.cout, .COUTP = l.coutp, .KH = l.k,
                    .KW = l.kw, .stride = l.stride, .pad = l.pad, .up = 1, .y_cstride = y_cstride};
  q.opt = pnvo_fp32_opts(o, m->num_cus);
  return q;
}

// launch timing of a conv of l at B samples: algorithmic flops and bytes
double conv_flops(const Layer &l, int B) { return 2.0 * ((double)((long)B * l.hout * l.wout) * l.cout * (l.cin / l.cgroups) * l.k * l.kw); }
double conv_bytes(const Layer &l, int B) {
  return 4.0 * ((double)B * l.hin * l.win * l.cin + (double)((long)B * l.hout * l.wout) * l.cout + (double)l.cout * l.cin * l.k * l.kw);
}

// The block's downsample conv cd rides on its first 3x3 conv c1 when both run on the float16-piece form of conv_x3_kernel and share the
// output geometry (they always do: resnet.py:189-212), in the inference and the training forward alike (the training forward still
// writes the block input: its backward pass reads it), and not while a tap wants the plain schedule.  (c1's side — 3x3, stride 2, two
// float16 pieces — is the plan's to refuse: conv_x3_plan.)
bool ride_fits(pnvo_handle m, const PnvoOptions &o, const Layer &c1, const Layer &cd) {
  if (!o.ds_fuse || m->tap_dst != nullptr || m->bottleneck || cd.k != 1 || cd.kw != 1 || cd.stride != 2 || cd.pad != 0) return false;
  if (c1.cinp != cd.cinp || c1.coutp != cd.coutp || c1.cout != cd.cout || c1.hout != cd.hout || c1.wout != cd.wout || c1.hin != cd.hin ||
      c1.win != cd.win || c1.cout != c1.coutp || c1.groups != cd.groups || cd.host_w.empty())
    return false;
  return x3_layer(o, cd) && x3_two_pieces(m, cd);
}

// Which kernel family runs conv l at B samples for this ask under options o, and what follows from that.  The one place that decides
// it: a forward asks with the handle's options (pnvo_conv_choice), the workspace with copies that select each family (stats_floats).
ConvChoice conv_choice(pnvo_handle m, const PnvoOptions &o, const Layer &l, int B, const ConvAsk &ask) {
  ConvChoice c;
  const int P = l.hout * l.wout;
  c.flops = conv_flops(l, B);
  if (l.cgroups > 1) {           // conv_group.hip: 32-pixel slots x slabs of max(cg, 16) channels, dense inside a slab
    c.family = ConvChoice::GROUP;
    c.slots = conv_group_slots(P);
    c.flops = 2.0 * B * c.slots * 32.0 * l.cout * (double)std::max(l.cin / l.cgroups, 16) * 9.0;
    return c;
  }
  // GroupNorm-ed 3x3 and 1x1 stride-2 convs: float32 results from the 16-bit matrix cores (conv_x3.hip) where its planner takes the
  // launch; option conv=fp32 keeps the fp32-MFMA kernels.
  const bool dense_gn = ask.gn && !ask.plain;
  if (dense_gn && l.groups > 0 && x3_layer(o, l) && (ask.ride == nullptr || ride_fits(m, o, l, *ask.ride))) {
    // The schedule's rule, kept as it stood before this value existed: forward_body, the training forward and pnvo_layer_kernel decide
    // tails, rides and the small-generic pre-pass per LAYER, before a stager mode is known, so they ask about the tile kernels on the
    // plain stager (a default ask: mode 0) with the rows form off.  Only the launch's own ask (conv_ask: rows_form) lets
    // conv_rows32_kernel take the tile plan's place — with fewer statistics slots than the tile plan the buffer is sized for.
    const bool tile_kernels_only = !ask.rows_form;
    // The conv_x3 problem: shape, operand pieces, stager mode and handle m's plan options.  (tail_scaled: the rows plan refuses a block
    // tail whose skip branch carries its own GroupNorm — a downsample skip, reachable with baseplanes 16: the rows kernel adds the raw skip tensor)
    ConvX3Problem q{.B = B, .H = l.hin, .W = l.win, .CIN = l.cinp, .Ho = l.hout, .Wo = l.wout, .COUTP = l.coutp, .ks = l.k, .stride = l.stride,
                    .np = x3_two_pieces(m, l) ? 2 : 3, .mode = ask.tail == ConvAsk::KEYS ? 3 : ask.tail != ConvAsk::NONE ? 2 : ask.affine ? 1 : 0,
                    .tail_scaled = ask.tail == ConvAsk::SKIP_SCALED, .ds = ask.ride != nullptr};
    q.opt = {.force = o.conv == 1, .strip = o.x3_strip, .fine = o.x3_fine, .w8 = o.x3_w8, .m16 = o.x3_m16,
             .ksw = o.x3_ksplit, .persist_wgs = o.x3_persist ? 3 * m->num_cus : 0, .rows = tile_kernels_only ? 0 : o.x3_rows,
             .num_cus = m->num_cus};
    if (const ConvX3Plan p = conv_x3_plan(q)) {
      c.family = ConvChoice::X3;
      c.x3q = q;
      c.x3p = p;
      c.slots = p.slots;
      // tiles x M-tiles x 32 pixels (the 16x16x32 flavour of x2: 16-row sub-tiles x 16) x padded outputs x K, six bf16 (x3) or three float16 (x2) MFMA terms per float32 product
      if (p.family != ConvX3Plan::ROWS)
        c.flops = (p.np == 2 ? 3.0 : 6.0) * 2.0 * (double)B * p.tiles_r * p.tiles_c * (double)p.m_rows * l.coutp * (double)l.cinp * l.k * l.kw;
      return c;
    }
  }
  // The float32-MFMA kernels: an LDS-staged 3x3 conv (slots = tiles x waves) where the ask allows one, else the generic implicit GEMM.
  // The problem is the layer's with the plain operand; conv_fp32_plan keeps family, wave tile and slots for the launch's real mode.
  c.fp32q = fp32_problem(m, o, l, B, l.coutp);
  c.fp32q.stats = ask.gn;
  c.fp32q.lds_ok = dense_gn && o.conv != 3;
  c.fp32p = conv_fp32_plan(c.fp32q);
  c.family = c.fp32p.family == ConvFp32Plan::LDS_TILE || c.fp32p.family == ConvFp32Plan::LDS_WAVE ? ConvChoice::FP32_LDS : ConvChoice::FP32_GENERIC;
  c.slots = c.fp32p.slots;
  return c;
}
}  // namespace

ConvChoice pnvo_conv_choice(pnvo_handle m, const Layer &l, int B, const ConvAsk &ask) { return conv_choice(m, m->opt, l, B, ask); }

// Does block b's downsample conv ride on the launch of its first conv at B samples?  Only a two-conv block carries a ride (ride_fits
// refuses Bottleneck models; said here for the walks that serve both block kinds); the rest is the conv choice's to say.
bool pnvo_ds_rides(pnvo_handle m, const Block &b, int B) {
  return b.ds >= 0 && b.nconv == 2 && pnvo_conv_choice(m, m->convs[b.conv[0]], B, {.ride = &m->convs[b.ds]}).family == ConvChoice::X3;
}

bool pnvo_conv_takes_tail(pnvo_handle m, const Layer &l, int B) {
  // taps want the block outputs of the plain schedule; option tail=separate: the pass of its own
  return m->tap_dst == nullptr && m->opt.tail && pnvo_conv_choice(m, l, B, {}).family == ConvChoice::X3;
}

namespace {
// GroupNorm partials of l at B samples: the most slots of the families an option change can select without the workspace regrowing
// (generic, LDS, the forced tile plan — stride 2 included —, group)
size_t stats_floats(pnvo_handle m, const Layer &l, int B) {
  PnvoOptions o = m->opt;
  int slots = 0;
  o.x3_s2 = 1;
  o.fp32_tile = 0;                                                     // (one 32-pixel tile per wave: the most slots of the generic kernel)
  for (o.conv = 1; o.conv <= 3; ++o.conv)                              // x3 | fp32 | generic
    for (o.fp32_form = 1; o.fp32_form <= 2; ++o.fp32_form)             // the LDS-staged convs: tile | wave
      slots = std::max(slots, conv_choice(m, o, l, B, {}).slots);
  return (size_t)B * (size_t)slots * l.coutp * 2;
}

// Statistics slots per sample a stem kernel leaves in m->stats: 8 x 16 tiles (MX, DD), 4 x 16 tiles (LDS).
int stem_slots(pnvo_handle m, StemPlan::Kernel k) {
  if (k == StemPlan::GENERIC) return 0;
  if (k == StemPlan::LDS) return stem_tiles_x(m->Ws) * stem_tiles_y(m->Hs);
  return k == StemPlan::MX ? stem_mx_slots(m->Hs, m->Ws) : stem_dd_slots(m->Hs, m->Ws);
}

int ensure_workspace(pnvo_handle m, int B) {   // (also exported as pnvo_ensure_workspace)
  if (B <= m->cap) return PNVO_OK;
  free_workspace(m);
  const pnvo_config &c = m->cfg;
  const size_t npix = (size_t)B * c.height * c.width;
  size_t act = (size_t)B * m->Hp * m->Wp * c.baseplanes;          // largest residual-stage tensor
  for (size_t k = 1; k < m->convs.size(); ++k) {
    const size_t need = (size_t)B * m->convs[k].hout * m->convs[k].wout * m->convs[k].coutp;
    if (need > act) act = need;
  }
  int maxc = m->comp_cp;
  size_t st = 0;                        // GroupNorm partials: whichever stem or conv leaves the most slots (option stem may change)
  for (StemPlan::Kernel k : {StemPlan::MX, StemPlan::DD, StemPlan::LDS}) st = std::max(st, (size_t)B * stem_slots(m, k) * m->convs[0].coutp * 2);
  for (const Layer &l : m->convs) {
    if (l.coutp > maxc) maxc = l.coutp;
    const size_t s = stats_floats(m, l, B);
    if (s > st) st = s;
  }
  (void)npix;   // the assembled [B,H,W,CP] input is only materialised for the "input" tap (allocated lazily)
  HIPCHK(m, m->stem_raw.alloc((size_t)B * m->Hs * m->Ws * c.baseplanes));
  HIPCHK(m, m->bufY[0].alloc(act));
  HIPCHK(m, m->bufY[1].alloc(act));
  HIPCHK(m, m->rawA.alloc(act));
  HIPCHK(m, m->rawB.alloc(act));
  HIPCHK(m, m->rawD.alloc(act));
  if (m->bottleneck) HIPCHK(m, m->rawC.alloc(act));
  HIPCHK(m, m->comp_raw.alloc((size_t)B * m->fh * m->fw * m->comp_cp));
  HIPCHK(m, m->hid.alloc((size_t)B * c.hidden));
  HIPCHK(m, m->out_ws.alloc((size_t)B * c.out_dim));
  HIPCHK(m, m->stats.alloc(st));
  HIPCHK(m, m->stats_ds.alloc(st));
  for (int k = 0; k < 2; ++k) {
    HIPCHK(m, m->ssA.alloc(k, (size_t)B * maxc));
    HIPCHK(m, m->ssB.alloc(k, (size_t)B * maxc));
    HIPCHK(m, m->ssD.alloc(k, (size_t)B * maxc));
    if (m->cfg.se) HIPCHK(m, m->ssE.alloc(k, (size_t)B * maxc));
    HIPCHK(m, m->ssC.alloc(k, (size_t)B * m->comp_cp));
    HIPCHK(m, hipMemset(m->ssC[k], 0, (size_t)B * m->comp_cp * sizeof(float)));   // pad channels stay (0, 0)
  }
  HIPCHK(m, m->tapbuf.alloc((size_t)B * m->fh * m->fw * m->comp_cp));
  HIPCHK(m, m->kpart.reserve((size_t)32 * B * (size_t)std::max(c.hidden, 32)));   // split-K partials of the linear layers: <= 32 slices of [B, hidden]
  m->cap = B;
  return PNVO_OK;
}

}  // namespace

PnvoTimed::PnvoTimed(pnvo_model_s *m_, hipStream_t s_, const std::string &name, double flops, double bytes) : m(m_), s(s_) {
  if (!m->timing) return;
  auto it = m->tindex.find(name);
  int idx;
  if (it == m->tindex.end()) {
    pnvo_kernel_time e;
    std::memset(&e, 0, sizeof(e));
    std::snprintf(e.name, sizeof(e.name), "%s", name.c_str());
    idx = (int)m->tentries.size();
    m->tentries.push_back(e);
    m->tindex[name] = idx;
  } else {
    idx = it->second;
  }
  m->tentries[idx].launches += 1;
  m->tentries[idx].flops += flops;
  m->tentries[idx].bytes += bytes;
  TimingRec r;
  auto get = [&]() {
    hipEvent_t e;
    if (!m->evpool.empty()) {
      e = m->evpool.back();
      m->evpool.pop_back();
    } else {
      (void)hipEventCreate(&e);
    }
    return e;
  };
  r.a = get();
  r.b = get();
  r.entry = idx;
  (void)hipEventRecord(r.a, s);
  m->trecs.push_back(r);
  rec = (int)m->trecs.size() - 1;
}

PnvoTimed::~PnvoTimed() {
  if (rec >= 0) (void)hipEventRecord(m->trecs[rec].b, s);
}

namespace {
typedef PnvoTimed Timed;

int maybe_tap(pnvo_handle m, const char *name, const float *src, size_t n, hipStream_t s) {
  if (m->tap_dst == nullptr || m->tap_name != name) return PNVO_OK;
  if (n > m->tap_cap) return fail(m, PNVO_ERR_ARG, std::string("tap buffer too small for '") + name + "'");
  HIPCHK(m, hipMemcpyAsync(m->tap_dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  return PNVO_OK;
}

}  // namespace

void pnvo_drop_graphs(pnvo_handle m) {
  for (auto &g : m->graphs) {
    (void)hipGraphExecDestroy(g.exec);
    (void)hipGraphDestroy(g.graph);
  }
  m->graphs.clear();
  m->seen.clear();
}

// Upper bound of |activation| entering each conv of the residual stages from per-layer GroupNorm bounds gn_bound(l) =
// max_c (|gamma_c| sqrt(N) + |beta_c|): a block output adds its skip branch (resnet.py:47-55).  Used at load (host copy of the
// parameters) and by the training step (bounds tracked on the device after every optimiser step, pnvo_train_api.hip).
void pnvo_chain_in_bounds(pnvo_handle h, const std::function<float(const Layer &)> &gn_bound) {
  if (h->bottleneck || h->convs.empty()) return;
  float bin = gn_bound(h->convs[0]);                         // pooled stem output
  for (const Block &b : h->blocks) {
    Layer &c1 = h->convs[b.conv[0]], &c2 = h->convs[b.conv[1]];
    c1.in_bound = bin;
    c2.in_bound = gn_bound(c1);
    float skip = bin;
    if (b.ds >= 0) {
      h->convs[b.ds].in_bound = bin;
      skip = gn_bound(h->convs[b.ds]);
    }
    bin = gn_bound(c2) + skip;
  }
  h->convs[h->comp].in_bound = bin;                          // the compression conv reads the last block's output
}

namespace {
// The conv_x3 weight operand of layer q of handle h in `pieces` pieces (2: float16 and the inverse of their scale, 3: bf16), rebuilt
// when h's weights moved since it was made: re-packed on the device from the flat parameters of an attached training step (weight
// and float16 scale live there: pnvo_train_refresh), else packed on the host and uploaded.
int x3_operand(pnvo_handle h, Layer &q, int pieces, hipStream_t s) {
  DevBuf<unsigned short> &wpk = pieces == 2 ? q.wpk_x2 : q.wpk_x3;
  unsigned long long &gen = pieces == 2 ? q.x2_gen : q.x3_gen;
  if (wpk && gen == h->weights_gen) return PNVO_OK;
  const size_t nel = (size_t)q.k * q.kw * q.cinp * q.coutp * pieces;
  if (!wpk) HIPCHK(h, wpk.alloc(nel));
  const float *dev_w = h->train ? pnvo_train_weight_ptr(h, q) : nullptr;
  if (dev_w != nullptr && pieces == 2) {
    HIPCHK(h, launch_conv_x2_repack(dev_w, q.cout, q.cin, q.cinp, q.coutp, q.k, q.kw, pnvo_train_x2_scale(h, q), wpk, s));
  } else if (dev_w != nullptr) {
    HIPCHK(h, launch_conv_x3_repack(dev_w, q.cout, q.cin, q.cinp, q.coutp, q.k, q.kw, 0, wpk, s));
  } else {
    std::vector<unsigned short> pk(nel);
    if (pieces == 2)
      q.x2_oscale = pack_conv_x2_weight(q.host_w.data(), q.cout, q.cin, q.cinp, q.coutp, q.k, q.kw, pk.data());
    else
      pack_conv_x3_weight(q.host_w.data(), q.cout, q.cin, q.cinp, q.coutp, q.k, q.kw, pk.data());
    HIPCHK(h, hipMemcpyAsync(wpk, pk.data(), nel * 2, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));
  }
  gen = h->weights_gen;
  return PNVO_OK;
}

// The GroupNorm finalisation behind a conv (or stem) of l that left `slots` partials per sample in m->stats — wave_rows > 0: the generic
// kernel's flattened wave tiles of that many pixels.
int finalize_gn(pnvo_handle m, const Layer &l, int B, int slots, int wave_rows, float *const *ss, float *mu, float *rstd, hipStream_t s,
                const GnGroup *gg = nullptr) {
  Timed t(m, s, "gn_finalize", 0.0, 0.0);
  HIPCHK(m, launch_gn_finalize(m->stats, B, slots, l.coutp, l.cout, l.groups, (long)l.hout * l.wout, wave_rows ? wave_rows : 1, l.gamma, l.beta, 1e-5f,
                               ss[0], ss[1], s, wave_rows ? 0 : slots, mu, rstd, gg));
  return PNVO_OK;
}

// conv_x3_kernel / conv_x3p_kernel, or conv_rows32_kernel (rows), on the choice's plan, + the GroupNorm finalisation unless the conv does it.
int run_conv_x3(pnvo_handle m, const Layer &l, int B, const ConvRequest &r, const ConvChoice &c) {
  const ConvX3Problem &q = c.x3q;
  const ConvX3Plan &p = c.x3p;
  hipStream_t s = r.s;
  const DsRide *ride = r.ride;
  const bool two = q.np == 2, rows = p.family == ConvX3Plan::ROWS;
  ConvX3Args xa = conv_x3_args(q, p);
  Layer &lm = const_cast<Layer &>(l);
  if (int rc = x3_operand(m, lm, q.np, s)) return rc;
  if (ride != nullptr) {             // the block's downsample conv on this launch (the schedule's choice for this ride said X3; the plan carries it: q.ds)
    Layer &dm = const_cast<Layer &>(*ride->cd);
    if (int rc = x3_operand(m, dm, 2, s)) return rc;
    xa.ds_wpk = dm.wpk_x2;
    xa.ds_oscale = dm.x2_oscale;
    if (m->train != nullptr) {
      const float *sp = pnvo_train_x2_scale(m, dm);
      xa.ds_oscale_ptr = sp ? sp + 1 : nullptr;
    }
    xa.ds_y = ride->y;
    xa.ds_stats = m->stats_ds;
  }
  GnGroup gg{0x7fffffff, 0x7fffffff, {nullptr, nullptr}, {nullptr, nullptr}}, ggd = gg;   // grouped forward: models 1 / 2 of this layer
  if (r.grp != nullptr) {
    const GroupedFwd &g = *r.grp;
    if (!two || rows) return fail(m, PNVO_ERR_STATE, "grouped forward: layer " + l.name + " is not on the float16-piece tile kernel");
    const size_t idx = (size_t)(&l - m->convs.data());
    if (idx >= m->convs.size()) return fail(m, PNVO_ERR_STATE, "grouped forward: layer outside the conv list");
    xa.grp_end0 = g.end[0];
    xa.grp_end1 = g.n > 2 ? g.end[1] : 0;
    gg.end0 = ggd.end0 = g.end[0];
    if (g.n > 2) gg.end1 = ggd.end1 = g.end[1];
    for (int k = 1; k < g.n; ++k) {
      pnvo_handle hk = g.h[k];
      Layer &lk = hk->convs[idx];
      if (!x3_two_pieces(hk, lk)) return fail(m, PNVO_ERR_STATE, "grouped forward: a model's " + l.name + " left the float16-piece form");
      if (int rc = x3_operand(hk, lk, 2, s)) return fail(m, rc, hk->err);
      xa.wpk_g[k - 1] = lk.wpk_x2;
      xa.oscale_g[k - 1] = lk.x2_oscale;
      xa.gn_gamma_g[k - 1] = gg.gamma[k - 1] = lk.gamma;
      xa.gn_beta_g[k - 1] = gg.beta[k - 1] = lk.beta;
      if (ride != nullptr) {
        const size_t idd = (size_t)(ride->cd - m->convs.data());
        Layer &dk = hk->convs[idd];
        if (!x3_two_pieces(hk, dk)) return fail(m, PNVO_ERR_STATE, "grouped forward: a model's downsample conv left the float16-piece form");
        if (int rc = x3_operand(hk, dk, 2, s)) return fail(m, rc, hk->err);
        xa.ds_wpk_g[k - 1] = dk.wpk_x2;
        xa.ds_oscale_g[k - 1] = dk.x2_oscale;
        xa.ds_gamma_g[k - 1] = ggd.gamma[k - 1] = dk.gamma;
        xa.ds_beta_g[k - 1] = ggd.beta[k - 1] = dk.beta;
      }
    }
  }
  xa.x = r.x;
  xa.wpk = two ? lm.wpk_x2 : lm.wpk_x3;
  xa.oscale = lm.x2_oscale;
  if (two && m->train != nullptr) {
    const float *sp = pnvo_train_x2_scale(m, l);
    xa.oscale_ptr = sp ? sp + 1 : nullptr;
  }
  xa.y = r.y;
  xa.in_scale = r.in_scale;
  xa.in_shift = r.in_shift;
  xa.stats = m->stats;
  if (r.tail != nullptr) {
    if (r.in_scale == nullptr) return fail(m, PNVO_ERR_STATE, "block tail without the conv's GroupNorm scale/shift");
    xa.res = r.tail->res;
    xa.res_scale = r.tail->res_scale;
    xa.res_shift = r.tail->res_shift;
    xa.xout = r.tail->out;
  }
  // one tile per sample (the 12 x 22 and 6 x 11 maps): the workgroup that sums a sample's channels also turns the sums into the
  // GroupNorm scale / shift — the same fp64 arithmetic as gn_finalize_kernel, bit for bit, one launch less (option gn_fuse)
  const long P = (long)l.hout * l.wout;
  const int cpg = l.groups > 0 ? l.cout / l.groups : 0;
  const bool fuse = m->opt.gn_fuse && xa.slots == 1 && l.cout == l.coutp && cpg >= 1 && cpg <= 32 &&
                    32 % cpg == 0 && l.cout % cpg == 0 && (rows || !(q.opt.persist_wgs > 0 && l.cin == 32 && l.coutp == 32));
  if (fuse && ride != nullptr) {
    xa.ds_gamma = ride->cd->gamma;
    xa.ds_beta = ride->cd->beta;
    xa.ds_scale = ride->ss[0];
    xa.ds_shift = ride->ss[1];
    xa.ds_mu = ride->mu;
    xa.ds_rstd = ride->rstd;
  }
  if (fuse) {
    xa.gn_gamma = l.gamma;
    xa.gn_beta = l.beta;
    xa.gn_scale = r.ss[0];
    xa.gn_shift = r.ss[1];
    xa.gn_mu = r.mu;
    xa.gn_rstd = r.rstd;
    xa.gn_cpg = cpg;
    xa.gn_eps = 1e-5f;
    xa.gn_P = P;
  }
  {
    Timed t(m, s, "conv:" + l.name, conv_flops(l, B), conv_bytes(l, B) + (r.tail ? 8.0 * B * l.hin * l.win * l.cin : 0.0));
    if (rows)
      HIPCHK(m, launch_conv_rows32(xa, p, s));
    else
      HIPCHK(m, launch_conv_x3(xa, p, s));
  }
  if (fuse) return PNVO_OK;
  if (ride != nullptr) {             // the conv's GroupNorm and the riding downsample conv's in one launch
    Timed t(m, s, "gn_finalize", 0.0, 0.0);
    const float *st2[2] = {m->stats, m->stats_ds}, *ga2[2] = {l.gamma, ride->cd->gamma}, *be2[2] = {l.beta, ride->cd->beta};
    float *sc2[2] = {r.ss[0], ride->ss[0]}, *sh2[2] = {r.ss[1], ride->ss[1]};
    float *mu2[2] = {r.mu, ride->mu}, *rs2[2] = {r.rstd, ride->rstd};
    HIPCHK(m, launch_gn_finalize_pair(st2, B, xa.slots, l.coutp, l.cout, l.groups, P, ga2, be2, 1e-5f, sc2, sh2, mu2, rs2, s,
                                      r.grp ? &gg : nullptr, r.grp ? &ggd : nullptr));
    return PNVO_OK;
  }
  return finalize_gn(m, l, B, xa.slots, 0, r.ss, r.mu, r.rstd, s, r.grp ? &gg : nullptr);
}

// The float32-MFMA kernels: the LDS-staged 3x3 conv, else the generic implicit GEMM — linear layers split the reduction when the
// output tiles alone cannot fill the chip, and the output head may ride on that reduction.
int run_conv_fp32(pnvo_handle m, const Layer &l, int B, const ConvRequest &r, const ConvChoice &c) {
  hipStream_t s = r.s;
  // the choice's problem with what the request adds: output stride, operand mode, epilogue, and what this handle can provide
  ConvFp32Problem q = c.fp32q;
  q.y_cstride = r.y_cstride;
  q.mode = r.src != nullptr ? 2 : r.in_scale != nullptr ? 1 : 0;
  q.linear = r.bias != nullptr || r.relu_out != 0;
  q.stats = r.ss != nullptr;
  q.ksplit_ok = r.bias != nullptr && !r.ss;          // linear layer: the reduction may be split (scratch: m->kpart, grown below)
  q.head = r.head_out != nullptr ? m->cfg.out_dim : 0;
  const ConvFp32Plan p = conv_fp32_plan(q);
  if (!p) return fail(m, PNVO_ERR_STATE, "conv " + l.name + ": no float32-MFMA kernel is instantiated for this launch (check options fp32_tile, fp32_form)");
  if (p.family != c.fp32p.family || (r.ss && p.slots != c.slots))
    return fail(m, PNVO_ERR_STATE, "conv " + l.name + ": the launch's plan left the schedule's choice");
  ConvArgs a = conv_fp32_args(q, p);
  if (q.mode == 2) {             // fused stem: gather A from the observation tensors
    const int nsrc[4] = {m->cfg.n_rgb, m->cfg.n_depth, m->cfg.n_dd, m->cfg.n_tdv};
    a.zero_page = m->zero_page;
    for (int j = 0; j < m->CP / 8; ++j)
      for (int hh = 0; hh < 2; ++hh)
        for (int k = 0; k < 2; ++k) {
          const int nc = 8 * j + 4 * hh + 2 * k;
          const int tn = m->stem_tensor_of_new[nc];
          SrcPiece &pc = a.pieces[j][hh][k];
          pc.base = tn >= 0 ? r.src[tn] : nullptr;
          pc.nch = tn >= 0 ? nsrc[tn] : 0;
          pc.choff = m->stem_ch_of_new[nc];
        }
  }
  a.x = r.x;
  a.wpk = l.wpk;
  a.y = r.y;
  a.in_scale = r.in_scale;
  a.in_shift = r.in_shift;
  a.stats = r.ss ? m->stats : nullptr;
  a.bias = r.bias;
  a.bias_row = r.bias_row;
  a.relu_out = r.relu_out;
  if (p.scratch_floats > 0) {
    if (p.scratch_floats > m->kpart.size()) {
      pnvo_drop_graphs(m);                           // captured launches point into the old scratch
      HIPCHK(m, m->kpart.alloc(p.scratch_floats));
    }
    a.kpart = m->kpart;
  }
  {
    Timed t(m, s, "conv:" + l.name, conv_flops(l, B), conv_bytes(l, B));
    const ConvFp32Head head{.w = r.head_w, .b = m->head_bias, .out_dim = m->cfg.out_dim, .out = r.head_out};
    HIPCHK(m, launch_conv_fp32(a, p, s, &head));     // ... with the split-K reduction, the output head on it where the plan says so
    if (p.reduce == ConvFp32Plan::HEAD && r.head_rode != nullptr) *r.head_rode = true;
  }
  return r.ss ? finalize_gn(m, l, B, p.slots, p.wave_rows, r.ss, r.mu, r.rstd, s) : PNVO_OK;
}

// The grouped 3x3 conv of a ResNeXt block (conv_group.hip) + the GroupNorm finalisation that follows it.
int run_conv_group(pnvo_handle m, const Layer &l, int B, const ConvRequest &r, const ConvChoice &c) {
  if (!r.ss || r.src != nullptr || r.bias != nullptr || r.relu_out || r.y_cstride != l.coutp || r.tail != nullptr || r.ride != nullptr ||
      r.grp != nullptr || l.cout != l.coutp || l.cin != l.cinp || !l.wpk_grp)
    return fail(m, PNVO_ERR_STATE, "grouped conv " + l.name + " asked for something only the dense kernels do");
  ConvGroupArgs a{.x = r.x, .wpk = l.wpk_grp, .in_scale = r.in_scale, .in_shift = r.in_shift, .y = r.y, .stats = m->stats, .B = B, .H = l.hin,
                  .W = l.win, .Ho = l.hout, .Wo = l.wout, .C = l.cout, .cg = l.cin / l.cgroups, .stride = l.stride, .slots = c.slots};
  {
    Timed t(m, r.s, "conv:" + l.name, conv_flops(l, B), conv_bytes(l, B));
    HIPCHK(m, launch_conv_group(a, r.s));
  }
  return finalize_gn(m, l, B, a.slots, 0, r.ss, r.mu, r.rstd, r.s);
}

// What request r asks of its conv's kernel (the launch's own ask: the rows form may take it).
ConvAsk conv_ask(const Layer &l, const ConvRequest &r) {
  const ConvAsk::Tail tail = !r.tail ? ConvAsk::NONE : !r.tail->res ? ConvAsk::KEYS : r.tail->res_scale ? ConvAsk::SKIP_SCALED : ConvAsk::SKIP;
  return {.gn = r.ss != nullptr, .plain = r.src != nullptr || r.bias != nullptr || r.relu_out != 0 || r.y_cstride != l.coutp,
          .affine = r.in_scale != nullptr, .tail = tail, .ride = r.ride ? r.ride->cd : nullptr, .rows_form = true};
}
}  // namespace

int pnvo_run_conv(pnvo_handle m, const Layer &l, int B, const ConvRequest &r) {
  const ConvChoice c = pnvo_conv_choice(m, l, B, conv_ask(l, r));
  // (a choice and the workspace's sizing that drifted apart would be an out-of-bounds device write)
  if (r.ss != nullptr && ((size_t)B * c.slots * l.coutp * 2 > m->stats.size() ||
                          (r.ride != nullptr && (size_t)B * c.slots * r.ride->cd->coutp * 2 > m->stats_ds.size())))
    return fail(m, PNVO_ERR_STATE, "conv " + l.name + ": the launch's GroupNorm partials do not fit the workspace");
  if (c.family == ConvChoice::GROUP) return run_conv_group(m, l, B, r, c);
  if (c.family == ConvChoice::X3) return run_conv_x3(m, l, B, r, c);
  if (r.ride != nullptr) return fail(m, PNVO_ERR_STATE, "downsample ride on a conv that cannot carry it (" + l.name + ")");
  if (r.tail != nullptr) return fail(m, PNVO_ERR_STATE, "block tail handed to a conv that cannot take it (" + l.name + ")");
  if (r.grp != nullptr && r.ss != nullptr) return fail(m, PNVO_ERR_STATE, "grouped forward: layer " + l.name + " fell off the float16-piece tile kernel");
  return run_conv_fp32(m, l, B, r, c);
}

// The stem's place in the forward is the 16-bit-matrix-core stems' (8 x 16-tile slots, pooled keys, raw entry) or the one-hot-aware
// stem's.  Once the input fallback engaged (dense_sticky) that place is kept and the float32 stem stands in (stem_lds_kernel<.., PAIRED>)
// wherever it serves the model; elsewhere, and in the training forward, the handle leaves the fused stems for stem_lds.hip / the
// generic kernel.
StemPlan pnvo_stem_plan(pnvo_handle m, bool train_fwd, const RawFrames &raw) {
  const Layer &stem = m->convs[0];
  StemPlan p;
  p.lds_serves = (m->CPL <= 32) && (stem.coutp == 32 || stem.coutp == 64) && stem.cout == stem.coutp;
  const bool keeps_place = !m->dense_sticky || (!train_fwd && p.lds_serves);
  if (keeps_place && m->mx_ok && (!train_fwd || m->train_mx) && m->opt.stem <= 1)
    p.kernel = StemPlan::MX;
  else if (keeps_place && m->dd_ok && m->opt.stem != 3)
    p.kernel = StemPlan::DD;       // (in training its operands are rebuilt on the device every step: refresh_stem_dd)
  else
    p.kernel = p.lds_serves ? StemPlan::LDS : StemPlan::GENERIC;
  const bool fused = p.kernel == StemPlan::MX || p.kernel == StemPlan::DD;
  p.standin = fused && m->dense_sticky;
  p.slots = stem_slots(m, p.kernel);
  // Inference forwards decide on the DEVICE whether the stem is redone on float32 operands (a stand-in predicated on the contract
  // flag); the training forward keeps the host-side event (its backward has to know, too).  Sensor frames are inside the contract
  // by construction: nothing to repair, nothing to mark.
  const bool on_device = m->opt.input_fallback && m->dd_flag != nullptr && !train_fwd && p.lds_serves;
  p.repairs = fused && !p.standin && raw.depth == nullptr && on_device;
  p.marks = m->dd_flag != nullptr && !m->dense_sticky && raw.depth == nullptr && !on_device;
  // two float16 weight pieces at inference (5 MFMAs per tap); three bf16 pieces (7, every product exact) on request and while the
  // float16 operand is stale: with a training step attached it is current when the step's device-side re-pack wrote it, or — eval
  // forwards only — when a pnvo_load_weights followed the last optimiser step
  const bool loaded_current = m->train == nullptr || m->weights_gen == m->weights_gen_at_load;
  const bool h2_current = m->mx_wpk2_dev || (train_fwd ? m->train == nullptr : loaded_current);
  const bool want2 = train_fwd ? m->opt.train_pieces == 2 : m->opt.pieces == 2;
  p.pieces = (want2 && h2_current && m->mx_wpk2 != nullptr) ? 2 : 3;
  p.h2_from_host = m->opt.pieces == 2 && m->mx_wpk2 != nullptr && loaded_current;
  return p;
}

double pnvo_stem_in_bytes(pnvo_handle m, int B, const RawFrames &raw) {
  const pnvo_config &c = m->cfg;
  // the observation tensors (or, RAW: 6 B of rgb + 8 B of depth + 8 B of top-down view per pixel) once
  return (double)B * c.height * c.width * (raw.depth ? (c.n_rgb ? 6.0 : 0.0) + 8.0 + (c.n_tdv ? 8.0 : 0.0) : 4.0 * m->convs[0].cin);
}

void pnvo_stem_mx_input(pnvo_handle m, int B, const float *const *src, const RawFrames &raw, StemMXArgs &a) {
  for (int k = 0; k < 4; ++k) a.src[k] = src[k];
  a.zero_page = m->mx_pages;
  a.B = B;
  a.H = m->cfg.height;
  a.W = m->cfg.width;
  a.Ho = m->Hs;
  a.Wo = m->Ws;
  a.slots = stem_slots(m, StemPlan::MX);
  if (raw.depth == nullptr) return;
  a.raw_rgb = raw.rgb;
  a.raw_depth = raw.depth;
  a.raw_flags = (m->cfg.n_depth > 0 ? 1 : 0) | (m->cfg.n_dd > 0 ? 2 : 0);
  a.raw_err = raw.err;
  const int bins = 10;                                             // the mx stem's K-slot layout (n_dd == 20)
  for (int i = 0; i < bins; ++i) a.edges[i] = (float)((double)i * 1.0 / (double)bins);   // base_trainer_with_vo.py:105-115
  a.edges[bins] = 1.0f;
  if (raw.edges != nullptr)                                        // the caller's (pnvo_train_forward_raw: the dataset's float16-rounded edges)
    for (int i = 0; i <= bins; ++i) a.edges[i] = raw.edges[i];
  a.edges[bins + 1] = 1.0f;
  a.src[0] = a.src[1] = a.src[2] = nullptr;
}

// Forms of the 16-bit-matrix-core stem (option stem_form: auto | fast | resident | tiles):
//   fast (auto when every workgroup gets >= 4 tiles): one 4-wave workgroup per CU for the whole launch, the weights in its
//     registers, staging of the next tile and epilogue of the previous one between the MFMAs (stem_rs.hip), the remainder MFMAs
//     of four taps in one K chunk and tap 48 split over the waves — 0.78 ms at 256 pairs, float32-grade equal to the others;
//   resident: the same kernel in the tile kernel's summation order — 0.81 ms, bit-identical to tiles (the bf16 path's dual stem
//     with its 196 KB of weight fragments takes this one);
//   tiles (auto otherwise, and every grouped forward): one tile per workgroup, two workgroups per CU — 0.99 ms, bound by the CU's
//     vector-memory pipe (245 KB of weight fragments + 93 KB of patch per 128-pixel tile);
//   (round 4's role-specialised persistent form — stem_ps_kernel, as fast as tiles — was retired in round 5: HISTORY.md.)
int pnvo_launch_stem_mx(pnvo_handle m, const StemMXArgs &a, int pieces, int ntiles, bool bf16_out, const GroupedFwd *grp, hipStream_t s) {
  const int form = m->opt.stem_form;
  const bool resident = grp == nullptr && (form == 3 || form == 4 || form == 0) && stem_rs_takes(a, pieces, ntiles, bf16_out, m->num_cus);
  if (!bf16_out) m->mx_prof_rs = resident;         // (the bf16 path's launches carry no profile buffer)
  if (resident)
    HIPCHK(m, launch_stem_rs(a, pieces, !bf16_out && (form == 4 || form == 0), m->num_cus, s));
  else
    HIPCHK(m, launch_stem_mx(a, pieces, ntiles, bf16_out, s));
  return PNVO_OK;
}

// The operands of stem_lds.hip: the dense stem, or (`slots` of an 8 x 16-tile stem, paired) the stand-in for one.
static void stem_lds_args(pnvo_handle m, int B, const StemRequest &r, int slots, StemArgs &a) {
  const pnvo_config &c = m->cfg;
  const int nsrc[4] = {c.n_rgb, c.n_depth, c.n_dd, c.n_tdv};
  std::memset(&a, 0, sizeof(a));
  for (int j = 0; j < m->CPL / 8; ++j)
    for (int hh = 0; hh < 2; ++hh)
      for (int q = 0; q < 2; ++q) {
        const int nc = 8 * j + 4 * hh + 2 * q;
        const int tn = nc < m->CP ? m->stem_tensor_of_new[nc] : -1;
        a.pieces[j][hh][q].base = tn >= 0 ? r.src[tn] : nullptr;
        a.pieces[j][hh][q].nch = tn >= 0 ? nsrc[tn] : 0;
        a.pieces[j][hh][q].choff = tn >= 0 ? m->stem_ch_of_new[nc] : 0;
      }
  a.sc = m->stem_sc;
  a.sh = m->stem_sh;
  a.wpk = m->stem_wpk16;
  a.zero_page = m->zero_page;
  a.y = r.y;
  a.stats = m->stats;
  a.B = B;
  a.H = c.height;
  a.W = c.width;
  a.Ho = m->Hs;
  a.Wo = m->Ws;
  a.CPL = m->CPL;
  a.slots = slots;
}

// The stem's entry of the timing table; the stand-in predicated on the contract flag is a "stem_repair" without figures.
static Timed stem_timed(pnvo_handle m, int B, const StemRequest &r, bool repair) {
  const Layer &stem = m->convs[0];
  if (repair) return Timed(m, r.s, "stem_repair", 0.0, 0.0);
  const double M = (double)B * m->Hs * m->Ws, wts = (double)stem.cout * stem.cin * 49;
  return Timed(m, r.s, "conv:" + stem.name, 2.0 * M * wts, pnvo_stem_in_bytes(m, B, r.raw) + 4.0 * (M * stem.cout + wts));
}

// The float32 stem in the place of an 8 x 16-tile stem: raw output + that stem's GroupNorm slot layout (+ pooled keys).  `only_if`
// (device-readable flag) makes both launches no-ops while it is zero.
static int pnvo_stem_standin(pnvo_handle m, int B, const StemRequest &r, int slots, const int *only_if) {
  const Layer &stem = m->convs[0];
  StemArgs a;
  stem_lds_args(m, B, r, slots, a);
  a.paired = 1;
  a.only_if = only_if;
  a.publish = only_if ? m->dd_flag : nullptr;     // a raised flag reaches the host-mapped copy from this launch
  {
    Timed t = stem_timed(m, B, r, only_if != nullptr);
    HIPCHK(m, launch_stem_lds(a, stem.coutp, r.s));
  }
  if (r.pool_keys != nullptr) {
    Timed t(m, r.s, only_if ? "stem_repair" : "pool_keys", 0.0, only_if ? 0.0 : 4.0 * B * ((double)m->Hs * m->Ws + (double)m->Hp * m->Wp) * stem.coutp);
    HIPCHK(m, launch_pool_keys_from_raw(r.y, stem.gamma, B, m->Hs, m->Ws, stem.coutp, r.pool_keys, only_if, r.s));
  }
  return PNVO_OK;
}

// Behind a contract-checking stem launch whose repair is NOT decided on the device: the flag's host copy, and an event the caller
// waits for (pnvo_input_fallback); no event while a stream capture is under way (an event recorded into a graph cannot be waited
// for: such forwards keep the deferred check of pnvo_check_inputs).
int pnvo_mark_stem(pnvo_handle m, hipStream_t s, const StemPlan &p) {
  if (!p.marks) return PNVO_OK;
  HIPCHK(m, launch_flag_publish(m->dd_flag_dev, m->dd_flag, s));   // the host-side decisions below / pnvo_check_inputs read the host copy
  if (!m->opt.input_fallback) return PNVO_OK;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return PNVO_OK;
  if (!m->stem_ev) HIPCHK(m, hipEventCreateWithFlags(&m->stem_ev, hipEventDisableTiming));
  HIPCHK(m, hipEventRecord(m->stem_ev, s));
  m->stem_ev_pending = true;
  return PNVO_OK;
}

// bf16 / float16 matrix cores, exact weight pieces: float32 results (stem_mx.hip, stem_rs.hip)
static int stem_launch_mx(pnvo_handle m, int B, const StemRequest &r, const StemPlan &p, GnGroup &sgg) {
  const Layer &stem = m->convs[0];
  StemMXArgs a;
  std::memset(&a, 0, sizeof(a));
  pnvo_stem_mx_input(m, B, r.src, r.raw, a);
  a.wpk = p.pieces == 2 ? m->mx_wpk2 : m->mx_wpk3;
  a.oscale = m->mx_oscale;
  // (after a device-side re-pack the scale lives on the device; a later pnvo_load_weights re-packs on the host with its own)
  a.oscale_ptr = m->mx_wpk2_dev ? m->mx_scale2_dev + 1 : nullptr;
  a.bad_input = m->dd_flag_dev;
  const int ntn = stem.cout / 32;
  for (int g = 0; g < ntn; ++g) {
    a.y[g] = r.y;
    a.stats[g] = m->stats;
    a.y_coff[g] = 32 * g;
  }
  a.y_cstride = stem.coutp;
  a.stats_cstride = stem.coutp;
  a.pool = r.pool_keys;
  a.pool_gamma = stem.gamma;
  a.Hp = m->Hp;
  a.Wp = m->Wp;
  if (r.grp != nullptr) {               // grouped forward: the other models' stem operands (tile kernel only)
    if (p.pieces != 2 || r.pool_keys == nullptr) return fail(m, PNVO_ERR_STATE, "grouped forward needs the float16-piece stem with pooled keys");
    a.grp_end0 = sgg.end0 = r.grp->end[0];
    if (r.grp->n > 2) a.grp_end1 = sgg.end1 = r.grp->end[1];
    for (int k = 1; k < r.grp->n; ++k) {
      pnvo_handle hk = r.grp->h[k];
      if (hk->mx_wpk2 == nullptr || hk->mx_wpk2_dev) return fail(m, PNVO_ERR_STATE, "grouped forward: a model has no host-packed float16 stem operand");
      a.wpk_g[k - 1] = hk->mx_wpk2;
      a.oscale_g[k - 1] = hk->mx_oscale;
      a.pool_gamma_g[k - 1] = sgg.gamma[k - 1] = hk->convs[0].gamma;
      sgg.beta[k - 1] = hk->convs[0].beta;
    }
  }
  a.dbg = m->opt.stem_dbg >= 16 ? m->opt.stem_dbg - 16 : 0;
  if (m->opt.stem_dbg == 9 || m->opt.stem_dbg >= 16) {
    if (!m->mx_prof) {
      HIPCHK(m, m->mx_prof.alloc(256));
      HIPCHK(m, hipMemset(m->mx_prof, 0, 2048));
    }
    a.prof = m->mx_prof;
  }
  // the input fallback engaged: the float32 stem stands in (same place in the forward, same slot layout, pooled keys)
  if (p.standin) return pnvo_stem_standin(m, B, r, p.slots, nullptr);
  Timed t = stem_timed(m, B, r, false);
  return pnvo_launch_stem_mx(m, a, p.pieces, ntn, false, r.grp, r.s);
}

// one-hot-aware stem (stem_dd.hip)
static int stem_launch_dd(pnvo_handle m, int B, const StemRequest &r, const StemPlan &p) {
  const pnvo_config &c = m->cfg;
  if (p.standin) return pnvo_stem_standin(m, B, r, p.slots, nullptr);   // the input fallback engaged: in this stem's slot layout
  const int nsrc[4] = {c.n_rgb, c.n_depth, c.n_dd, c.n_tdv};
  StemDDArgs a;
  std::memset(&a, 0, sizeof(a));
  for (int j = 0; j < 3; ++j)
    for (int q = 0; q < 2; ++q) {
      const int d = 4 * j + 2 * q;
      const int tn = m->dd_dense_tensor[d];
      a.pieces[j][0][q].base = tn >= 0 ? r.src[tn] : nullptr;
      a.pieces[j][0][q].nch = tn >= 0 ? nsrc[tn] : 0;
      a.pieces[j][0][q].choff = tn >= 0 ? m->dd_dense_ch[d] : 0;
    }
  a.sc = m->dd_sc;
  a.sh = m->dd_sh;
  a.wpk = m->dd_wpk;
  a.table = m->dd_table;
  a.dd = r.src[2];
  a.zero_page = m->zero_page;
  a.bad_onehot = m->dd_flag_dev;
  a.y = r.y;
  a.stats = m->stats;
  a.B = B;
  a.H = c.height;
  a.W = c.width;
  a.Ho = m->Hs;
  a.Wo = m->Ws;
  a.bins = m->dd_bins;
  a.slots = p.slots;
  a.dbg = m->opt.stem_dbg;
  if (a.dbg == 9) {
    if (!m->dd_prof) {
      HIPCHK(m, m->dd_prof.alloc(8));
      HIPCHK(m, hipMemset(m->dd_prof, 0, 64));
    }
    a.prof = m->dd_prof;
  }
  Timed t = stem_timed(m, B, r, false);
  HIPCHK(m, launch_stem_dd(a, r.s));
  return PNVO_OK;
}

// The fused stem: input assembly + /255 + whitening gathered in the operand fetch, raw output + GroupNorm scale / shift (+ optional
// mean / rstd).
int pnvo_run_stem(pnvo_handle m, int B, const StemRequest &r) {
  const Layer &stem = m->convs[0];
  const StemPlan p = pnvo_stem_plan(m, r.train_fwd, r.raw);
  int rc = PNVO_OK;
  if (r.pool_keys != nullptr && !p.pools()) return fail(m, PNVO_ERR_STATE, "pooled stem output asked of a stem kernel without it");
  GnGroup sgg{0x7fffffff, 0x7fffffff, {nullptr, nullptr}, {nullptr, nullptr}};
  switch (p.kernel) {
    case StemPlan::MX: rc = stem_launch_mx(m, B, r, p, sgg); break;
    case StemPlan::DD: rc = stem_launch_dd(m, B, r, p); break;
    case StemPlan::LDS: {
      StemArgs a;
      stem_lds_args(m, B, r, p.slots, a);
      a.dbg = m->opt.stem_dbg;
      a.lds_pad = m->opt.stem_dbg_pad;
      Timed t = stem_timed(m, B, r, false);
      HIPCHK(m, launch_stem_lds(a, stem.coutp, r.s));
      break;
    }
    case StemPlan::GENERIC:             // MODE 2 of the generic kernel; pnvo_run_conv finalises the GroupNorm itself
      return pnvo_run_conv(m, stem, B, {.in_scale = m->stem_sc, .in_shift = m->stem_sh, .y = r.y, .y_cstride = stem.coutp, .ss = r.ss,
                                        .mu = r.mu, .rstd = r.rstd, .src = r.src, .grp = r.grp, .s = r.s});
  }
  if (rc != PNVO_OK) return rc;
  if (p.kernel != StemPlan::LDS) {
    // a value outside the observation contract (the flag the stager raised): redone on float32 operands, decided on the DEVICE —
    // two launches that return at once while the flag is down; the host never waits (it reads the flag at its next entry and
    // moves the handle to the stand-in for good: pnvo_check_inputs)
    if (p.repairs && (rc = pnvo_stem_standin(m, B, r, p.slots, m->dd_flag_dev)) != PNVO_OK) return rc;
    if ((rc = pnvo_mark_stem(m, r.s, p)) != PNVO_OK) return rc;
  }
  if (r.slots_out != nullptr) *r.slots_out = p.slots;
  return r.skip_finalize ? PNVO_OK : finalize_gn(m, stem, B, p.slots, 0, r.ss, r.mu, r.rstd, r.s, r.grp ? &sgg : nullptr);
}

int pnvo_ensure_workspace(pnvo_handle m, int B) { return ensure_workspace(m, B); }

namespace {
// option table: key -> (member, accepted spellings).  The PNVO_* environment variables of earlier rounds are the DEFAULTS of
// these options, read once per handle in pnvo_create; nothing on the forward path reads the environment.
struct OptChoice {
  const char *word;
  int value;
};
struct OptDef {
  const char *key, *env;
  int PnvoOptions::*field;
  bool numeric;                 // value = atoi(word) instead of a choice
  OptChoice choices[7];
};
const OptDef kOptions[] = {
    {"stem", "PNVO_STEM", &PnvoOptions::stem, false, {{"auto", 0}, {"mx", 1}, {"dd", 2}, {"dense", 3}, {nullptr, 0}}},
    {"conv", "PNVO_CONV", &PnvoOptions::conv, false, {{"auto", 0}, {"x3", 1}, {"fp32", 2}, {"generic", 3}, {nullptr, 0}}},
    {"pieces", "PNVO_PIECES", &PnvoOptions::pieces, false, {{"2", 2}, {"3", 3}, {nullptr, 0}}},
    {"stem_form", "PNVO_STEM_FORM", &PnvoOptions::stem_form, false, {{"auto", 0}, {"tiles", 2}, {"resident", 3}, {"fast", 4}, {nullptr, 0}}},
    {"train_pieces", "PNVO_TRAIN_PIECES", &PnvoOptions::train_pieces, false, {{"2", 2}, {"3", 3}, {nullptr, 0}}},
    {"x3_persist", "PNVO_X3_PERSIST", &PnvoOptions::x3_persist, false, {{"on", 1}, {"off", 0}, {nullptr, 0}}},
    {"x3_rows", "PNVO_X3_ROWS", &PnvoOptions::x3_rows, false, {{"on", 1}, {"off", 0}, {nullptr, 0}}},
    {"x3_strip", "PNVO_X3_STRIP", &PnvoOptions::x3_strip, false, {{"on", 1}, {"off", 0}, {nullptr, 0}}},
    {"x3_fine", "PNVO_X3_FINE", &PnvoOptions::x3_fine, false, {{"on", 1}, {"off", 0}, {nullptr, 0}}},
    {"x3_w8", "PNVO_X3_W8", &PnvoOptions::x3_w8, false, {{"on", 1}, {"off", 0}, {nullptr, 0}}},
    {"x3_m16", "PNVO_X3_M16", &PnvoOptions::x3_m16, false, {{"on", 1}, {"off", 0}, {nullptr, 0}}},
    {"x3_ksplit", "PNVO_X3_KSPLIT", &PnvoOptions::x3_ksplit, false, {{"on", 1}, {"off", 0}, {nullptr, 0}}},
    // the float32-MFMA kernels' plan options (ConvFp32Opts); the environment spells the wave split 1 / 0
    {"fp32_tile", "PNVO_CONV_TILE", &PnvoOptions::fp32_tile, true, {{nullptr, 0}}},
    {"fp32_wsplit", "PNVO_CONV_WSPLIT", &PnvoOptions::fp32_wsplit, false, {{"auto", -1}, {"on", 1}, {"off", 0}, {"1", 1}, {"0", 0}, {nullptr, 0}}},
    {"fp32_form", "PNVO_CONV3", &PnvoOptions::fp32_form, false, {{"auto", 0}, {"tile", 1}, {"wave", 2}, {nullptr, 0}}},
    {"wave_wgs", "PNVO_WAVE_WGS", &PnvoOptions::wave_wgs, true, {{nullptr, 0}}},
    {"wave_nt", "PNVO_WAVE_NT", &PnvoOptions::wave_nt, true, {{nullptr, 0}}},
    {"fc_rows", "PNVO_FC_ROWS", &PnvoOptions::fc_rows, true, {{nullptr, 0}}},
    {"head_fuse", "PNVO_HEAD_FUSE", &PnvoOptions::head_fuse, false, {{"on", 1}, {"off", 0}, {nullptr, 0}}},
    {"ds_fuse", "PNVO_DS_FUSE", &PnvoOptions::ds_fuse, false, {{"on", 1}, {"off", 0}, {nullptr, 0}}},
    {"gn_fuse", "PNVO_GN_FUSE", &PnvoOptions::gn_fuse, false, {{"on", 1}, {"off", 0}, {nullptr, 0}}},
    {"x3_s2", nullptr, &PnvoOptions::x3_s2, false, {{"on", 1}, {"off", 0}, {nullptr, 0}}},
    {"tail", "PNVO_TAIL", &PnvoOptions::tail, false, {{"fused", 1}, {"separate", 0}, {nullptr, 0}}},
    {"pool", "PNVO_POOL", &PnvoOptions::pool, false, {{"fused", 1}, {"separate", 0}, {nullptr, 0}}},
    {"graph", "PNVO_GRAPH", &PnvoOptions::graph, true, {{nullptr, 0}}},
    {"stem_dbg", nullptr, &PnvoOptions::stem_dbg, true, {{nullptr, 0}}},
    {"stem_dbg_pad", nullptr, &PnvoOptions::stem_dbg_pad, true, {{nullptr, 0}}},
    {"wgrad_stem", "PNVO_WGRAD_STEM", &PnvoOptions::wgrad_stem, false, {{"mx", 0}, {"fp32", 1}, {nullptr, 0}}},
    {"wgrad3", "PNVO_WGRAD3", &PnvoOptions::wgrad3, false, {{"x3", 1}, {"fp32", 0}, {nullptr, 0}}},
    {"wgrad", "PNVO_WGRAD", &PnvoOptions::wgrad, false, {{"auto", 0}, {"lds9", 1}, {"generic", 2}, {nullptr, 0}}},
    {"pool_bwd", "PNVO_POOL_BWD", &PnvoOptions::pool_bwd, false, {{"fused", 1}, {"separate", 0}, {nullptr, 0}}},
    {"dgrad", "PNVO_DGRAD", &PnvoOptions::dgrad, false, {{"phase", 1}, {"masked", 0}, {nullptr, 0}}},
    {"bf16_fuse", nullptr, &PnvoOptions::bf16_fuse, false, {{"on", 1}, {"off", 0}, {nullptr, 0}}},
    {"input_fallback", "PNVO_INPUT_FALLBACK", &PnvoOptions::input_fallback, false, {{"on", 1}, {"off", 0}, {nullptr, 0}}},
    {"small_net", "PNVO_SMALL_NET", &PnvoOptions::small_net, false, {{"on", 1}, {"off", 0}, {nullptr, 0}}},
    {"small_max", "PNVO_SMALL_MAX", &PnvoOptions::small_max, true, {{nullptr, 0}}},
    {"small_coop", "PNVO_SMALL_COOP", &PnvoOptions::small_coop, true, {{nullptr, 0}}},
    {"small_prof", "PNVO_SMALL_PROF", &PnvoOptions::small_prof, true, {{nullptr, 0}}},
};

const OptDef *find_option(const char *key) {
  for (const OptDef &d : kOptions)
    if (std::strcmp(d.key, key) == 0) return &d;
  return nullptr;
}

bool parse_option(const OptDef &d, const char *word, int *out) {
  if (d.numeric) {
    char *end = nullptr;
    const long v = std::strtol(word, &end, 10);
    if (end == word || *end != 0) return false;
    *out = (int)v;
    return true;
  }
  for (const OptChoice *c = d.choices; c->word != nullptr; ++c)
    if (std::strcmp(c->word, word) == 0) {
      *out = c->value;
      return true;
    }
  return false;
}

void env_defaults(pnvo_model_s *m) {
  for (const OptDef &d : kOptions) {
    const char *e = d.env ? std::getenv(d.env) : nullptr;
    int v;
    if (e && parse_option(d, e, &v)) m->opt.*(d.field) = v;
  }
  // spellings of earlier rounds that do not fit the table
  if (std::getenv("PNVO_X3_S2_OFF")) m->opt.x3_s2 = 0;
  if (std::getenv("PNVO_BF16_NOFUSE")) m->opt.bf16_fuse = 0;
  if (const char *e = std::getenv("PNVO_STEM_DBG")) std::sscanf(e, "%d,%d", &m->opt.stem_dbg, &m->opt.stem_dbg_pad);
}
}  // namespace


// The stems that exploit the observation contract (uint8-valued rgb, one-hot depth: stem_mx.hip, stem_dd.hip) raise a
// host-mapped flag when a value breaks it.  pnvo_run_stem records an event behind such a stem; once the rest of the forward
// is enqueued the caller waits for THAT event (the stem is the first kernel of ~55: it has normally finished by then, and the
// GPU keeps the rest of the queue), and a raised flag re-runs the forward on the dense fp32 stem — which takes any float
// input, as the reference model does (vo_cnn.py:110-176) — and keeps the handle on it.
int pnvo_input_fallback(pnvo_handle m, hipStream_t s, bool *rerun) {
  *rerun = false;
  if (!m->stem_ev_pending) return PNVO_OK;
  m->stem_ev_pending = false;
  HIPCHK(m, hipEventSynchronize(m->stem_ev));
  if (!m->dd_flag || *(volatile int *)m->dd_flag == 0) return PNVO_OK;
  *(volatile int *)m->dd_flag = 0;
  HIPCHK(m, hipMemsetAsync(m->dd_flag_dev, 0, sizeof(int), s));
  m->dense_sticky = true;
  m->fallback_count += 1;
  pnvo_drop_graphs(m);
  m->note = "note: observation values outside the fused stems' contract (fractional rgb or depth codes that are not one-hot) — "
           "the forward was re-run on the dense fp32 stem and this handle stays on it";
  *rerun = true;
  return PNVO_OK;
}

namespace {
int forward_dispatch(pnvo_handle m, int B, const FwdRequest &r);
int forward_body(pnvo_handle m, int B, const FwdRequest &r);

// Do the pair tensors / the sensor frames a caller handed over match the model's observation space?
bool pairs_match(const pnvo_config &c, const float *rgb, const float *depth, const float *dd, const float *tdv) {
  return (c.n_rgb > 0) == (rgb != nullptr) && (c.n_depth > 0) == (depth != nullptr) && (c.n_dd > 0) == (dd != nullptr) &&
         (c.n_tdv > 0) == (tdv != nullptr);
}
bool frames_match(const pnvo_config &c, const uint8_t *rgb_frames, const float *depth_frames, const float *tdv) {
  return (c.n_rgb > 0) == (rgb_frames != nullptr) && !((c.n_depth > 0 || c.n_dd > 0) && depth_frames == nullptr) &&
         (c.n_tdv > 0) == (tdv != nullptr);
}
// The entry checks of a single-handle forward in their order: handle, weights, batch / output, then what `inputs_match` says of the inputs
int check_entry(pnvo_handle m, const char *entry, int B, const void *out, bool inputs_match, const char *inputs) {
  if (!m) return fail(m, PNVO_ERR_ARG, "null handle");
  if (!m->loaded) return fail(m, PNVO_ERR_STATE, std::string(entry) + " before pnvo_load_weights");
  if (B <= 0 || !out) return fail(m, PNVO_ERR_ARG, "bad batch / null output");
  if (!inputs_match) return fail(m, PNVO_ERR_ARG, std::string(inputs) + " do not match the model's observation_space");
  return PNVO_OK;
}
int check_pairs(pnvo_handle m, const char *entry, const float *rgb, const float *depth, const float *dd, const float *tdv, int B, const void *out) {
  return check_entry(m, entry, B, out, !m || pairs_match(m->cfg, rgb, depth, dd, tdv), "observation tensors");
}
int check_frames(pnvo_handle m, const char *entry, const uint8_t *rgb_frames, const float *depth_frames, const float *tdv, int B, const void *out) {
  return check_entry(m, entry, B, out, !m || frames_match(m->cfg, rgb_frames, depth_frames, tdv), "sensor frames");
}

// ... of the two handles of a dual forward, up to the inputs
int check_dual(pnvo_handle ha, pnvo_handle hb, const char *entry, int B, const void *out_a, const void *out_b) {
  if (!ha || !hb) return fail(ha, PNVO_ERR_ARG, "null handle");
  if (!ha->loaded || !hb->loaded) return fail(ha, PNVO_ERR_STATE, std::string(entry) + " before pnvo_load_weights");
  if (B <= 0 || !out_a || !out_b) return fail(ha, PNVO_ERR_ARG, "bad batch / null output");
  if (ha->precision != 1 || hb->precision != 1)
    return fail(ha, PNVO_ERR_STATE, std::string(entry) + " runs the bfloat16 path: call pnvo_set_precision(h, 1) on both models");
  if (std::memcmp(&ha->cfg, &hb->cfg, sizeof(pnvo_config)) != 0 || ha->device != hb->device)
    return fail(ha, PNVO_ERR_ARG, "the two models of a dual forward must share architecture and device");
  return PNVO_OK;
}

// precision == 1: one model on the bfloat16 path
int forward_bf16_one(pnvo_handle m, int B, const FwdRequest &r) {
  float *outs[1] = {r.out};
  return pnvo_forward_bf16(&m, 1, B, r, outs);
}

// Size the workspace, run the forward (through the graph cache where the entry allows it) and, where a stem left its contract event
// pending, wait for it and run again on the dense stem when the input broke the contract.
int run_forward(pnvo_handle m, int B, const FwdRequest &r, bool graphs_allowed) {
  int (*const run)(pnvo_handle, int, const FwdRequest &) = graphs_allowed ? forward_dispatch : forward_body;
  int rc = ensure_workspace(m, B);
  if (rc != PNVO_OK || (rc = run(m, B, r)) != PNVO_OK) return rc;
  bool rerun = false;
  if ((rc = pnvo_input_fallback(m, r.s, &rerun)) != PNVO_OK) return rc;
  return rerun ? run(m, B, r) : PNVO_OK;
}
}


// ==================================================================================================================
extern "C" {

// "pnvo 0.3 (gfx950) src:<sha256[:16] of the tracked sources this library was built from>": the Makefile writes src_hash.h from
// csrc/*.hip, csrc/*.h and include/pnvo.h (sorted by name), tests/test_abi.py recomputes it — a loaded .so that does not match the
// tree it sits in is caught by the round-end GPU test, not by a reader of the numbers.
#include "src_hash.h"
const char *pnvo_version(void) { return "pnvo 0.3 (gfx950: fp32 + f16/bf16 MFMA) src:" PNVO_SRC_HASH; }

const char *pnvo_last_error(pnvo_handle h) { return h ? h->err.c_str() : g_err.c_str(); }

const char *pnvo_last_note(pnvo_handle h) {
  if (h && h->loaded && h->opt.input_fallback && pnvo_stem_plan(h, false, {}).lds_serves) (void)pnvo_check_inputs(h);     // a raised input-contract flag (host-mapped, no wait) is noted here at the latest
  return h ? h->note.c_str() : "";
}

int pnvo_create(const pnvo_config *cfg, int device, pnvo_handle *out) {
  if (!cfg || !out) return fail(nullptr, PNVO_ERR_ARG, "null argument");
  const int C = cfg->n_rgb + cfg->n_depth + cfg->n_dd + cfg->n_tdv;
  if (C <= 0) return fail(nullptr, PNVO_ERR_ARG, "visual odometry must not be blind (no input modality)");   // vo_cnn.py:68
  if (C > 64 || (cfg->n_rgb % 2) || (cfg->n_depth % 2) || (cfg->n_dd % 2) || (cfg->n_tdv % 2))
    return fail(nullptr, PNVO_ERR_ARG, "unsupported input channel configuration");
  if (cfg->width < 32 || cfg->height < 32) return fail(nullptr, PNVO_ERR_ARG, "observation_size must be >= 32x32");
  if (cfg->baseplanes < 32 || cfg->baseplanes % 32 || cfg->hidden % 8 || cfg->hidden <= 0 || cfg->out_dim <= 0)
    return fail(nullptr, PNVO_ERR_ARG, "unsupported baseplanes / hidden_size / output_dim");
  if ((cfg->resnext != 0 && cfg->resnext != 1) || (cfg->se != 0 && cfg->se != 1) ||
      ((cfg->resnext || cfg->se) && cfg->backbone_depth != 50 && cfg->backbone_depth != 101))
    return fail(nullptr, PNVO_ERR_ARG, "unsupported backbone: resnext / se are 0 or 1 and need backbone_depth 50 or 101");
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return fail(nullptr, PNVO_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) return fail(nullptr, PNVO_ERR_HIP, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
    return fail(nullptr, PNVO_ERR_ARG, std::string("libpnvo is built for gfx950 only, device is ") + prop.gcnArchName);
  pnvo_model_s *m = new pnvo_model_s();
  static std::atomic<unsigned long long> next_uid{1};
  m->uid = next_uid.fetch_add(1);
  m->cfg = *cfg;
  m->device = device;
  m->num_cus = prop.multiProcessorCount;
  if (m->cfg.flat_size <= 0) m->cfg.flat_size = 2048;
  if (m->cfg.n_acts <= 0) m->cfg.n_acts = 4;
  env_defaults(m);                 // the ONLY place the PNVO_* environment is read for this handle
  build_plan(m);
  *out = m;
  return PNVO_OK;
}

int pnvo_load_weights(pnvo_handle h, const float *blob, size_t n_floats, const pnvo_tensor_desc *toc, int ntoc) {
  if (!h || !blob || !toc) return fail(h, PNVO_ERR_ARG, "null argument");
  HIPCHK(h, hipSetDevice(h->device));
  pnvo_drop_graphs(h);            // weight buffers may be re-allocated
  Toc t;
  t.blob = blob;
  t.n = n_floats;
  for (int k = 0; k < ntoc; ++k) t.by_name[toc[k].name] = &toc[k];
  int rc = PNVO_OK;
  const pnvo_config &c = h->cfg;
  h->mean.assign(h->C, 0.f);
  h->stdev.assign(h->C, 1.f);
  if (c.normalize) {
    const std::string pre = "visual_encoder.running_mean_and_var.";
    const float *mu = find_tensor(h, t, pre + "_mean", {1, h->C, 1, 1}, &rc);
    if (!mu) return rc;
    const float *var = find_tensor(h, t, pre + "_var", {1, h->C, 1, 1}, &rc);
    if (!var) return rc;
    for (int k = 0; k < h->C; ++k) {
      h->mean[k] = mu[k];
      h->stdev[k] = std::sqrt(std::fmax(var[k], 1e-2f));   // running_mean_and_var.py:62, float32
    }
  }
  for (Layer &l : h->convs)
    if ((rc = load_conv(h, t, l, true)) != PNVO_OK) return rc;
  for (Block &b : h->blocks) {         // SE(planes * expansion).excite: Linear(C, C / 16), ReLU, Linear(C / 16, C), Sigmoid (resnet.py:75-80)
    if (b.se_r == 0) continue;
    const std::string pre = "visual_encoder.backbone." + b.tap + ".se.excite.";
    const int C = h->last(b).cout, R = b.se_r;
    if (!se_gate_supported(C, R)) return fail(h, PNVO_ERR_ARG, "SE branch of " + b.tap + ": unsupported width " + std::to_string(C));
    const float *w1 = find_tensor(h, t, pre + "0.weight", {R, C}, &rc);
    if (!w1) return rc;
    const float *b1 = find_tensor(h, t, pre + "0.bias", {R}, &rc);
    if (!b1) return rc;
    const float *w2 = find_tensor(h, t, pre + "2.weight", {C, R}, &rc);
    if (!w2) return rc;
    const float *b2 = find_tensor(h, t, pre + "2.bias", {C}, &rc);
    if (!b2) return rc;
    HIPCHK(h, b.se_w1.upload(w1, (size_t)R * C));
    HIPCHK(h, b.se_b1.upload(b1, R));
    HIPCHK(h, b.se_w2.upload(w2, (size_t)C * R));
    HIPCHK(h, b.se_b2.upload(b2, C));
  }
  if (!h->bottleneck) {
    // Upper bounds of |activation| entering each conv of the residual stages, from the GroupNorm parameters alone: a group of N
    // elements normalised to unit variance has |x^| <= sqrt(N), so |relu(GN(x))| <= max_c (|gamma_c| sqrt(N) + |beta_c|); a block
    // output adds its skip branch.  The two-piece float16 operands of conv_x3 need the bound below 65504 (pnvo_run_conv).
    auto gn_bound = [&](const Layer &l) {
      const float *g = find_tensor(h, t, l.gn + ".weight", {l.cout}, &rc), *b = find_tensor(h, t, l.gn + ".bias", {l.cout}, &rc);
      if (!g || !b) return 3.0e38f;
      const double rootn = std::sqrt((double)(l.cout / l.groups) * l.hout * l.wout);
      double mx = 0.0;
      for (int c2 = 0; c2 < l.cout; ++c2) mx = std::fmax(mx, std::fabs((double)g[c2]) * rootn + std::fabs((double)b[c2]));
      return (float)std::fmin(mx, 3.0e38);
    };
    pnvo_chain_in_bounds(h, gn_bound);
  }
  {
    // fused stem: re-pack conv1 with its input channels in observation-tensor order, and fold /255 and the
    // RunningMeanAndVar whitening into x*sc+sh:  (x/255 - mean)/std = x * 1/(255 std) - mean/std
    Layer &st = h->convs[0];
    const float *w = find_tensor(h, t, st.name + ".weight", {st.cout, st.cin, st.k, st.kw}, &rc);
    if (!w) return rc;
    const int T = st.k * st.kw;
    std::vector<float> wp((size_t)st.cout * h->CP * T, 0.f), sc(h->CPL, 0.f), sh(h->CPL, 0.f);
    for (int nc = 0; nc < h->CP; ++nc) {
      const int rc_ = h->stem_ref_of_new[nc];
      if (rc_ < 0) continue;
      for (int o = 0; o < st.cout; ++o)
        std::memcpy(&wp[((size_t)o * h->CP + nc) * T], &w[((size_t)o * st.cin + rc_) * T], sizeof(float) * T);
      const double sd = (double)h->stdev[rc_], mu = (double)h->mean[rc_];
      const double div = (h->stem_tensor_of_new[nc] == 0) ? 255.0 : 1.0;
      sc[nc] = (float)(1.0 / (div * sd));
      sh[nc] = (float)(-mu / sd);
    }
    std::vector<float> pk;
    pack_conv_weight_cinp(wp.data(), st.cout, h->CP, h->CP, st.k, st.kw, pk);
    HIPCHK(h, st.wpk.upload(pk.data(), pk.size()));
    HIPCHK(h, h->stem_sc.upload(sc.data(), sc.size()));
    HIPCHK(h, h->stem_sh.upload(sh.data(), sh.size()));
    std::vector<float> z(64, 0.f);
    HIPCHK(h, h->zero_page.upload(z.data(), z.size()));
    std::vector<float> pk16((size_t)49 * h->CPL * st.cout);
    pack_stem_weight(wp.data(), st.cout, h->CP, h->CPL, pk16.data());
    HIPCHK(h, h->stem_wpk16.upload(pk16.data(), pk16.size()));
    // ---- one-hot-aware stem: split the input channels into dense (matrix cores) and one-hot depth bins (table gather)
    h->dd_ok = false;
    const int bins = c.n_dd / 2;
    if (c.n_dd > 0 && stem_dd_supported(bins) && st.cout == 32 && c.normalize) {
      h->dd_dense_tensor.clear();
      h->dd_dense_ch.clear();
      std::vector<int> dense_ref;
      for (int nc = 0; nc < h->CP; ++nc)
        if (h->stem_ref_of_new[nc] >= 0 && h->stem_tensor_of_new[nc] != 2) {
          h->dd_dense_tensor.push_back(h->stem_tensor_of_new[nc]);
          h->dd_dense_ch.push_back(h->stem_ch_of_new[nc]);
          dense_ref.push_back(h->stem_ref_of_new[nc]);
        }
      const int nd = (int)dense_ref.size();
      if (nd % 2 == 0 && nd + 1 <= 12) {
        std::vector<float> wd((size_t)st.cout * 12 * T, 0.f), sc16(12, 0.f), sh16(12, 0.f);
        for (int d = 0; d < nd; ++d) {
          const int r = dense_ref[d];
          for (int o = 0; o < st.cout; ++o)
            std::memcpy(&wd[((size_t)o * 12 + d) * T], &w[((size_t)o * st.cin + r) * T], sizeof(float) * T);
          const double sd = (double)h->stdev[r], mu = (double)h->mean[r];
          const double div = (h->dd_dense_tensor[d] == 0) ? 255.0 : 1.0;
          sc16[d] = (float)(1.0 / (div * sd));
          sh16[d] = (float)(-mu / sd);
        }
        sh16[nd] = 1.0f;                                   // indicator channel: 1 inside the image (x = 0, sc = 0)
        while ((int)h->dd_dense_tensor.size() < 12) {
          h->dd_dense_tensor.push_back(-1);
          h->dd_dense_ch.push_back(0);
        }
        // reference channel of one-hot entry (frame f, bin b)
        std::vector<int> ddref(2 * bins, -1);
        for (int nc = 0; nc < h->CP; ++nc)
          if (h->stem_ref_of_new[nc] >= 0 && h->stem_tensor_of_new[nc] == 2) ddref[h->stem_ch_of_new[nc]] = h->stem_ref_of_new[nc];
        const int slice = stem_dd_slice_floats(bins), brows = bins + 1;
        std::vector<float> tab((size_t)7 * slice, 0.f);
        for (int kh = 0; kh < 7; ++kh)
          for (int kw = 0; kw < 7; ++kw) {
            const int tap = kh * 7 + kw;
            for (int o = 0; o < st.cout; ++o) {
              double ind = 0.0;
              for (int f = 0; f < 2; ++f)
                for (int b = 0; b < bins; ++b) {
                  const int r = ddref[f * bins + b];
                  const double wv = (double)w[((size_t)o * st.cin + r) * T + tap];
                  const double sd = (double)h->stdev[r], mu = (double)h->mean[r];
                  tab[(size_t)kh * slice + (((size_t)kw * brows + b) * 2 + f) * 32 + o] = (float)(wv / sd);
                  ind -= wv * mu / sd;
                }
              wd[((size_t)o * 12 + nd) * T + tap] = (float)ind;   // weight of the "inside the image" indicator
            }
          }
        std::vector<float> pkd((size_t)49 * 12 * st.cout);
        pack_stem_dd_weight(wd.data(), st.cout, pkd.data());
        HIPCHK(h, h->dd_wpk.upload(pkd.data(), pkd.size()));
        HIPCHK(h, h->dd_table.upload(tab.data(), tab.size()));
        HIPCHK(h, h->dd_sc.upload(sc16.data(), 12));
        HIPCHK(h, h->dd_sh.upload(sh16.data(), 12));
        if ((rc = reset_contract_flag(h)) != PNVO_OK) return rc;
        h->dd_bins = bins;
        h->dd_ok = true;
      }
    }
  }
  {
    // ---- stem on the bf16 matrix cores (stem_mx.hip)
    Layer &st = h->convs[0];
    const float *w = find_tensor(h, t, st.name + ".weight", {st.cout, st.cin, st.k, st.kw}, &rc);
    if (!w) return rc;
    h->mx_ok = false;
    const int nsrc[4] = {c.n_rgb, c.n_depth, c.n_dd, c.n_tdv};
    // fixed K-slot layout of stem_mx.hip: 0-19 discretised depth | 20-25 rgb | 26-27 depth | 28-29 top-down view | 30 indicator
    const bool shape_ok = (c.n_rgb == 0 || c.n_rgb == 6) && (c.n_depth == 0 || c.n_depth == 2) && (c.n_dd == 0 || c.n_dd == 20) &&
                          (c.n_tdv == 0 || c.n_tdv == 2);
    if (shape_ok && (st.cout == 32 || st.cout == 64) && st.k == 7) {
      std::vector<int> slot_ref(32, -1), slot_ref_sw(32, -1), slot_tensor(32, -1), slot_new(32, -1);
      const int first_slot[4] = {20, 26, 0, 28};           // rgb, depth, dd, tdv
      for (int x = 0; x < 4; ++x) h->mx_xslot[x] = -1;
      if (c.n_depth) h->mx_xslot[0] = 26, h->mx_xslot[1] = 27;
      if (c.n_tdv) h->mx_xslot[2] = 28, h->mx_xslot[3] = 29;
      for (int tn = 0; tn < 4; ++tn)
        for (int ch = 0; ch < nsrc[tn]; ++ch) {
          int nc = -1, ncs = -1;                            // position in the stem's "new" (tensor-major) channel order
          for (int k = 0; k < h->CP; ++k) {
            if (h->stem_tensor_of_new[k] != tn) continue;
            if (h->stem_ch_of_new[k] == ch) nc = k;
            if (h->stem_ch_of_new[k] == (ch + nsrc[tn] / 2) % nsrc[tn]) ncs = k;   // the frame-swapped twin
          }
          slot_ref[first_slot[tn] + ch] = h->stem_ref_of_new[nc];
          slot_new[first_slot[tn] + ch] = nc;
          slot_ref_sw[first_slot[tn] + ch] = h->stem_ref_of_new[ncs];
          slot_tensor[first_slot[tn] + ch] = tn;
        }
      const int T = 49;
      auto fold = [&](const std::vector<int> &ref, std::vector<float> &wk) {
        wk.assign((size_t)st.cout * 32 * T, 0.f);
        for (int o = 0; o < st.cout; ++o)
          for (int tap = 0; tap < T; ++tap) {
            double ind = 0.0;
            for (int k = 0; k < 30; ++k) {
              const int r = ref[k];
              if (r < 0) continue;
              const double wv = (double)w[((size_t)o * st.cin + r) * T + tap];
              const double sd = (double)h->stdev[r], mu = (double)h->mean[r];
              const double div = slot_tensor[k] == 0 ? 255.0 : 1.0;
              wk[((size_t)o * 32 + k) * T + tap] = (float)(wv / (div * sd));
              ind -= wv * mu / sd;
            }
            wk[((size_t)o * 32 + 30) * T + tap] = (float)ind;      // "inside the image" indicator
          }
      };
      fold(slot_ref, h->mx_wk);
      fold(slot_ref_sw, h->mx_wk_swapped);
      h->mx_slot_ref = slot_ref;
      h->mx_slot_new = slot_new;
      std::vector<unsigned short> pk(stem_mx_packed_u16(3, st.cout / 32));
      pack_stem_mx_weight(h->mx_wk.data(), st.cout, 3, h->mx_xslot, pk.data());
      HIPCHK(h, h->mx_wpk3.upload(pk.data(), pk.size()));
      {
        std::vector<unsigned short> pk2(stem_mx_packed_u16(2, st.cout / 32));
        h->mx_oscale = pack_stem_mx_weight_h(h->mx_wk.data(), st.cout, h->mx_xslot, pk2.data());
        h->mx_wpk2_dev = false;
        HIPCHK(h, h->mx_wpk2.upload(pk2.data(), pk2.size()));
      }
      {
        std::vector<float> pages(64, 0.f);
        HIPCHK(h, h->mx_pages.upload(pages.data(), pages.size()));
      }
      if ((rc = reset_contract_flag(h)) != PNVO_OK) return rc;
      h->mx_ok = true;
    }
  }
  // Linear(flat[+embed] -> hidden): visual columns become the fh x fw "conv"; the embedding columns fold into a
  // per-action bias row:  bias[a][o] = b[o] + sum_e W[o][flat+e] * emb[a][e]   (vo_cnn_act_embed.py:63-72)
  const int flat = h->comp_c * h->fh * h->fw;
  const int fc_in = flat + (c.act_embed ? 32 : 0);
  const float *w1 = find_tensor(h, t, h->fc.name + ".weight", {c.hidden, fc_in}, &rc);
  if (!w1) return rc;
  const float *b1 = find_tensor(h, t, h->fc.name + ".bias", {c.hidden}, &rc);
  if (!b1) return rc;
  {
    std::vector<float> vis((size_t)c.hidden * flat);
    for (int o = 0; o < c.hidden; ++o) std::memcpy(&vis[(size_t)o * flat], w1 + (size_t)o * fc_in, sizeof(float) * flat);
    std::vector<float> pk;
    h->fc.host_w = vis;                                    // (smallnet.hip packs its own layout from these)
    {                                                      // fc_rows.hip: plain rows in the activation's (h, w, padded channel) order
      const int hw = h->fh * h->fw, kp = hw * h->comp_cp;
      std::vector<float> rows((size_t)c.hidden * kp, 0.f);
      for (int o = 0; o < c.hidden; ++o)
        for (int ch = 0; ch < h->comp_c; ++ch)
          for (int q = 0; q < hw; ++q) rows[(size_t)o * kp + (size_t)q * h->comp_cp + ch] = vis[(size_t)o * flat + (size_t)ch * hw + q];
      HIPCHK(h, h->fc_rows_w.upload(rows.data(), rows.size()));
    }
    pack_conv_weight_cinp(vis.data(), c.hidden, h->comp_c, h->comp_cp, h->fh, h->fw, pk);
    HIPCHK(h, h->fc.wpk.upload(pk.data(), pk.size()));
    const int rows = c.act_embed ? c.n_acts + 1 : 1;
    std::vector<float> bias((size_t)rows * c.hidden);
    const float *emb = nullptr;
    if (c.act_embed) {
      emb = find_tensor(h, t, "action_embedding.weight", {c.n_acts + 1, 32}, &rc);
      if (!emb) return rc;
    }
    for (int a = 0; a < rows; ++a)
      for (int o = 0; o < c.hidden; ++o) {
        double acc = 0.0;
        if (emb)
          for (int e = 0; e < 32; ++e) acc += (double)w1[(size_t)o * fc_in + flat + e] * (double)emb[a * 32 + e];
        bias[(size_t)a * c.hidden + o] = (float)(acc + (double)b1[o]);
      }
    HIPCHK(h, h->fc_bias.upload(bias.data(), bias.size()));
  }
  const float *w2 = find_tensor(h, t, "output_head.1.weight", {c.out_dim, c.hidden}, &rc);
  if (!w2) return rc;
  const float *b2 = find_tensor(h, t, "output_head.1.bias", {c.out_dim}, &rc);
  if (!b2) return rc;
  {
    std::vector<float> pk;
    h->head.host_w.assign(w2, w2 + (size_t)c.out_dim * c.hidden);
    pack_conv_weight_cinp(w2, c.out_dim, c.hidden, c.hidden, 1, 1, pk);
    HIPCHK(h, h->head.wpk.upload(pk.data(), pk.size()));
    HIPCHK(h, h->head_bias.upload(b2, c.out_dim));
    HIPCHK(h, h->head_w_plain.upload(w2, (size_t)c.out_dim * c.hidden));
  }
  h->loaded = true;
  h->load_gen += 1;
  h->weights_gen += 1;
  h->weights_gen_at_load = h->weights_gen;
  return PNVO_OK;
}

int pnvo_set_option(pnvo_handle h, const char *key, const char *value) {
  if (!h || !key || !value) return fail(h, PNVO_ERR_ARG, "null argument");
  const OptDef *d = find_option(key);
  if (!d) return fail(h, PNVO_ERR_ARG, std::string("unknown option '") + key + "'");
  int v;
  if (!parse_option(*d, value, &v)) {
    std::string msg = std::string("option '") + key + "' does not take '" + value + "' (";
    if (d->numeric) msg += "an integer";
    for (const OptChoice *c = d->choices; !d->numeric && c->word != nullptr; ++c) msg += std::string(c == d->choices ? "" : " | ") + c->word;
    return fail(h, PNVO_ERR_ARG, msg + ")");
  }
  const bool lift = d->field == &PnvoOptions::stem && h->dense_sticky;   // an explicit stem choice lifts the fallback
  if (h->opt.*(d->field) == v && !lift) return PNVO_OK;
  h->opt.*(d->field) = v;
  pnvo_drop_graphs(h);                       // captured launches encode the kernel selection
  if (lift) {
    // repairs of forwards still in flight read the flag on the device: wait for them before it is lowered (a rare, explicit call)
    if (h->dd_flag && *(volatile int *)h->dd_flag != 0) {
      HIPCHK(h, hipSetDevice(h->device));
      HIPCHK(h, hipDeviceSynchronize());
      *(volatile int *)h->dd_flag = 0;
      HIPCHK(h, hipMemset(h->dd_flag_dev, 0, sizeof(int)));
    }
    h->dense_sticky = false;
  }
  return PNVO_OK;
}

int pnvo_get_option(pnvo_handle h, const char *key, char *buf, size_t cap) {
  if (!h || !key || !buf || cap == 0) return fail(h, PNVO_ERR_ARG, "null argument");
  const OptDef *d = find_option(key);
  if (!d) return fail(h, PNVO_ERR_ARG, std::string("unknown option '") + key + "'");
  const int v = h->opt.*(d->field);
  std::string word = std::to_string(v);
  for (const OptChoice *c = d->choices; !d->numeric && c->word != nullptr; ++c)
    if (c->value == v) {
      word = c->word;
      break;
    }
  if (d->field == &PnvoOptions::stem && h->loaded && h->opt.input_fallback && pnvo_stem_plan(h, false, {}).lds_serves) (void)pnvo_check_inputs(h);   // see pnvo_last_note
  if (d->field == &PnvoOptions::stem && h->dense_sticky) word = "dense (fallback)";
  std::snprintf(buf, cap, "%s", word.c_str());
  return PNVO_OK;
}

int pnvo_set_precision(pnvo_handle h, int precision) {
  if (!h) return fail(h, PNVO_ERR_ARG, "null handle");
  if (precision != 0 && precision != 1) return fail(h, PNVO_ERR_ARG, "precision must be 0 (float32) or 1 (bfloat16)");
  if (precision == 1 && h->grouped_se)
    return fail(h, PNVO_ERR_ARG, "bfloat16 precision: SE / ResNeXt backbones run in float32 only (their grouped conv and gate have no bf16 form)");
  h->precision = precision;
  return PNVO_OK;
}

int pnvo_forward_dual(pnvo_handle ha, pnvo_handle hb, const float *rgb, const float *depth, const float *dd, const float *tdv,
                      int B, float *out_a, float *out_b, void *stream) {
  if (int rc0 = check_dual(ha, hb, "pnvo_forward_dual", B, out_a, out_b)) return rc0;
  if (ha->cfg.act_embed)
    return fail(ha, PNVO_ERR_ARG, "pnvo_forward_dual covers the separate-action models (act_left_right_inv_joint); act-embed "
                                  "models take their actions through pnvo_forward");
  if (!pairs_match(ha->cfg, rgb, depth, dd, tdv)) return fail(ha, PNVO_ERR_ARG, "observation tensors do not match the model's observation_space");
  if (int rc0 = pnvo_check_inputs(ha)) return rc0;
  HIPCHK(ha, hipSetDevice(ha->device));
  pnvo_handle hs[2] = {ha, hb};
  float *outs[2] = {out_a, out_b};
  return pnvo_forward_bf16(hs, 2, B, {.src = {rgb, depth, dd, tdv}, .s = (hipStream_t)stream}, outs);
}

int pnvo_check_inputs(pnvo_handle m) {
  if (!m) return fail(m, PNVO_ERR_ARG, "null handle");
  if (m->dd_flag && *(volatile int *)m->dd_flag != 0) {
    // already repaired: the handle runs the float32 stand-in since an earlier check; the flag only stays up for forwards still in
    // flight (turning input_fallback off afterwards must not turn every later forward into an error)
    if (m->dense_sticky) return PNVO_OK;
    if (m->opt.input_fallback && pnvo_stem_plan(m, false, {}).lds_serves) {
      // The flag is host-mapped: read without waiting for anything.  The forward that raised it repaired itself on the device
      // (pnvo_stem_standin behind its stem); from here on this handle launches the float32 stand-in directly.  The flag stays up
      // — repairs of forwards still in flight read it — until pnvo_set_option(h, "stem", ..) lifts the fallback.
      if (!m->dense_sticky) {
        m->dense_sticky = true;
        m->fallback_count += 1;
        pnvo_drop_graphs(m);
        m->note = "note: observation values outside the fused stems' contract (fractional rgb or depth codes that are not one-hot) — "
                  "the forward redid its stem on float32 operands (decided on the device) and this handle stays on the dense float32 stem";
      }
      return PNVO_OK;
    }
    return fail(m, PNVO_ERR_INPUT,
                "an earlier forward met observation values outside the reference's contract — a discretised-depth pixel "
                "that is not one-hot (base_trainer_with_vo.py:163) or an rgb value that is not an integer 0..255 — so its "
                "outputs are invalid (this handle runs with input_fallback=off, is inside a training forward, or its model is one the "
                "float32 stand-in stem does not serve — e.g. a forward that was stream-captured on such a model).  Feed "
                "contract inputs, keep option input_fallback on, or select the dense stem: pnvo_set_option(h, \"stem\", \"dense\")");
  }
  return PNVO_OK;
}

int pnvo_forward(pnvo_handle m, const float *rgb, const float *depth, const float *dd, const float *tdv,
                 const int64_t *actions, int B, float *out, void *stream) {
  if (int rc0 = check_pairs(m, "pnvo_forward", rgb, depth, dd, tdv, B, out)) return rc0;
  if (m->cfg.act_embed && !actions) return fail(m, PNVO_ERR_ARG, "act_embed model needs actions");
  if (int rc0 = pnvo_check_inputs(m)) return rc0;
  HIPCHK(m, hipSetDevice(m->device));
  const FwdRequest r{.src = {rgb, depth, dd, tdv}, .actions = actions, .out = out, .s = (hipStream_t)stream};
  return m->precision == 1 ? forward_bf16_one(m, B, r) /* before any float32 workspace is sized */ : run_forward(m, B, r, true);
}

namespace {
int forward_dispatch(pnvo_handle m, int B, const FwdRequest &r) {
  const pnvo_config &c = m->cfg;
  hipStream_t s = r.s;
  int rc = PNVO_OK;
  {
    // Opt-in (option graph=1).  Measured on ROCm 7.2 / MI355X: replaying the ~60-node graph is no faster than the plain
    // asynchronous launches — 6.32 vs 6.22 ms at B = 256 (the GPU is never starved) and 0.77 vs 0.80 ms at B = 1 (the
    // dependent-kernel latency of the chain, not the host launches, is what a batch-1 call pays).
    m->graph_mode = m->opt.graph;
  }
  const bool plain = !m->graph_mode || m->timing || m->tap_dst != nullptr || m->train != nullptr || m->opt.stem_dbg != 0;
  if (plain) return forward_body(m, B, r);

  // ---- graph replay: key = everything the captured kernel arguments depend on
  const void *key[8] = {r.src[0], r.src[1], r.src[2], r.src[3], r.actions, r.raw.rgb, r.raw.depth, r.raw.err};   // (pnvo_set_option drops the captured graphs)
  const StemPlan sp = pnvo_stem_plan(m, false, r.raw);
  const size_t out_bytes = (size_t)B * c.out_dim * sizeof(float);
  auto find = [&](std::vector<pnvo_model_s::GraphEntry> &v) {
    return std::find_if(v.begin(), v.end(), [&](const pnvo_model_s::GraphEntry &g) { return g.B == B && std::memcmp(g.key, key, sizeof(key)) == 0; });
  };
  if (auto g = find(m->graphs); g != m->graphs.end()) {
    g->stamp = ++m->graph_clock;
    HIPCHK(m, hipGraphLaunch(g->exec, s));
    HIPCHK(m, hipMemcpyAsync(r.out, m->out_ws, out_bytes, hipMemcpyDeviceToDevice, s));
    return pnvo_mark_stem(m, s, sp);
  }
  if (find(m->seen) == m->seen.end()) {            // capture only call shapes that come back
    pnvo_model_s::GraphEntry sn;
    std::memset(&sn, 0, sizeof(sn));
    std::memcpy(sn.key, key, sizeof(key));
    sn.B = B;
    if (m->seen.size() >= 16) m->seen.erase(m->seen.begin());
    m->seen.push_back(sn);
    return forward_body(m, B, r);
  }
  if (!m->cap_stream) HIPCHK(m, hipStreamCreateWithFlags(&m->cap_stream, hipStreamNonBlocking));
  pnvo_model_s::GraphEntry g;
  std::memcpy(g.key, key, sizeof(key));
  g.B = B;
  g.stamp = ++m->graph_clock;
  HIPCHK(m, hipStreamBeginCapture(m->cap_stream, hipStreamCaptureModeRelaxed));
  FwdRequest rcap = r;                              // the captured forward writes the handle's own output buffer
  rcap.out = m->out_ws;
  rcap.s = m->cap_stream;
  rc = forward_body(m, B, rcap);
  const hipError_t ce = hipStreamEndCapture(m->cap_stream, &g.graph);
  if (rc != PNVO_OK) {
    if (ce == hipSuccess && g.graph) (void)hipGraphDestroy(g.graph);
    return rc;
  }
  HIPCHK(m, ce);
  HIPCHK(m, hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
  if (m->graphs.size() >= 8) {                     // keep the 8 most recently used call shapes
    size_t old = 0;
    for (size_t k = 1; k < m->graphs.size(); ++k)
      if (m->graphs[k].stamp < m->graphs[old].stamp) old = k;
    (void)hipGraphExecDestroy(m->graphs[old].exec);
    (void)hipGraphDestroy(m->graphs[old].graph);
    m->graphs.erase(m->graphs.begin() + (long)old);
  }
  m->graphs.push_back(g);
  HIPCHK(m, hipGraphLaunch(g.exec, s));
  HIPCHK(m, hipMemcpyAsync(r.out, m->out_ws, out_bytes, hipMemcpyDeviceToDevice, s));
  return pnvo_mark_stem(m, s, sp);
}
}  // namespace

namespace {
// (r.actions, r.out, r.features_only, r.s of the request; the rows of `comp_raw` are the caller's to say)
int run_fc_head(pnvo_handle m, int B, const float *comp_raw, const float *sc, const float *sh, const FwdRequest &r);
bool fc_rows_usable(pnvo_handle m, int B, const FwdRequest &r);
int run_fc_rows(pnvo_handle m, pnvo_handle const *grp, const int *end, int ng, int B, const float *comp_raw, const float *sc, const float *sh,
                const FwdRequest &r);

// A raw conv output and the scale / shift pair of the GroupNorm that follows it: what the next conv, the gate or the block tail reads.
struct RawGn {
  float *x;
  float *const *ss;
};

// What the steps of a float32 forward hand on.
struct FwdState {
  float *cur, *nxt;          // the block input / where the next block output goes
  bool have_keys = false;    // `nxt` holds pooled stem keys: the first conv of the first block decodes them and writes `cur`
  bool have_tail = false;    // the last block's tail relu(GN(rawB) + skip) is still to be applied, by the stager of the next conv
  BlockTail tail{};
  bool done = false;         // the persistent small-batch launch ran everything behind the stem
};

// (a4-a7) stem + max-pool.  Input assembly, /255 and whitening are fused into the stem kernel's operand fetch (pnvo_run_stem): the
// [B,H,W,30] tensor of the reference (vo_cnn.py:174-176) is only materialised for the "input" tap.
int forward_stem(pnvo_handle m, int B, const FwdRequest &r, FwdState &st) {
  const pnvo_config &c = m->cfg;
  hipStream_t s = r.s;
  int rc = PNVO_OK;
  if (m->tap_dst != nullptr && m->tap_name == "input") {
    AssembleArgs a;
    for (int k = 0; k < 4; ++k) a.src[k] = r.src[k];
    a.nsrc[0] = c.n_rgb;
    a.nsrc[1] = c.n_depth;
    a.nsrc[2] = c.n_dd;
    a.nsrc[3] = c.n_tdv;
    a.mean = c.normalize ? m->mean.data() : nullptr;
    a.stdev = m->stdev.data();
    a.C = m->C;
    a.CP = m->CP;
    a.npix = (long)B * c.height * c.width;
    HIPCHK(m, m->xin.alloc((size_t)a.npix * m->CP));
    a.out = m->xin;
    HIPCHK(m, launch_assemble(a, s));
    if ((rc = maybe_tap(m, "input", m->xin, (size_t)B * c.height * c.width * m->CP, s)) != PNVO_OK) return rc;
  }
  const Layer &stem = m->convs[0];
  // GN + ReLU + maxpool.  Default: no pass at all — the stem writes pooled order-preserving keys (stem_mx.hip POOL), the first block's
  // first conv decodes / normalises them while staging and writes the pooled activations the skip branch needs (conv_x3 MODE 3).
  // PNVO_POOL=separate, taps, Bottleneck models and the other stem kernels keep the pass.
  const StemPlan sp = pnvo_stem_plan(m, false, r.raw);
  st.have_keys = !m->bottleneck && sp.pools() && m->opt.pool && stem.coutp == stem.cout &&
                 pnvo_conv_takes_tail(m, m->convs[m->blocks[0].conv[0]], B);
  StemRequest sr{.src = {r.src[0], r.src[1], r.src[2], r.src[3]}, .raw = r.raw, .y = m->stem_raw, .ss = m->ssA, .grp = r.grp, .s = s};
  // Batches of the navigation loop (one or two pairs): everything behind the stem conv is ONE persistent launch (smallnet.hip),
  // which also reduces the stem's GroupNorm statistics itself.
  if (!st.have_keys && sp.writes_slots() && !r.stop_after_compression && pnvo_small_usable(m, B)) {
    int stem_slots = 0;
    sr.slots_out = &stem_slots;
    sr.skip_finalize = true;
    st.done = true;
    if ((rc = pnvo_run_stem(m, B, sr)) != PNVO_OK) return rc;
    return pnvo_small_forward(m, B, r, stem_slots);
  }
  if (st.have_keys) {
    Timed t(m, s, "pool_init", 0.0, 4.0 * B * m->Hp * m->Wp * stem.coutp);
    HIPCHK(m, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(st.nxt), STEM_POOL_INIT, (size_t)B * m->Hp * m->Wp * stem.coutp, s));
    sr.pool_keys = reinterpret_cast<int *>(st.nxt);
  }
  if ((rc = pnvo_run_stem(m, B, sr)) != PNVO_OK) return rc;
  if ((rc = maybe_tap(m, "stem_conv", m->stem_raw, (size_t)B * m->Hs * m->Ws * stem.coutp, s)) != PNVO_OK) return rc;
  if (!st.have_keys) {
    Timed t(m, s, "gn_relu_maxpool", 0.0, 4.0 * B * ((double)m->Hs * m->Ws + (double)m->Hp * m->Wp) * stem.coutp);
    HIPCHK(m, launch_gn_relu_maxpool(m->stem_raw, m->ssA[0], m->ssA[1], B, m->Hs, m->Ws, stem.coutp, st.cur, s));
  }
  return maybe_tap(m, "maxpool", st.cur, (size_t)B * m->Hp * m->Wp * stem.coutp, s);
}

// (a8) residual stages: per block a chain of nconv convs (BasicBlock 2, resnet.py:29-55; Bottleneck 3, :58-117), each reading the raw
// output of the one before through its GroupNorm pair, then the SE gate, the skip branch and the tail.  Raw outputs: rawA, (rawC,) rawB
// in chain order, pairs ssA / ssB in turn; the downsample conv's in rawD / ssD.
int forward_blocks(pnvo_handle m, int B, const FwdRequest &r, FwdState &st) {
  hipStream_t s = r.s;
  int rc = PNVO_OK;
  for (size_t bk = 0; bk < m->blocks.size(); ++bk) {
    const Block &b = m->blocks[bk];
    const int K = b.nconv;
    const bool ds = b.ds >= 0;
    // The block's downsample conv rides on its first conv's launch (conv_x3_kernel DSF): no launch, no finalisation of its own.  Not
    // while pooled keys are pending: the key-decoding stager has no riding form.
    const bool ds_ride = !st.have_keys && pnvo_ds_rides(m, b, B);
    const DsRide ride{ds_ride ? &m->convs[b.ds] : nullptr, m->rawD, m->ssD, nullptr, nullptr};
    const BlockTail ktail{nullptr, nullptr, nullptr, st.cur};
    RawGn last{nullptr, nullptr};
    for (int k = 0; k < K; ++k) {
      const Layer &ck = m->convs[b.conv[k]];
      const RawGn out{k == K - 1 ? m->rawB : k == 0 ? m->rawA : m->rawC, k % 2 ? m->ssB : m->ssA};
      ConvRequest q{.y = out.x, .y_cstride = ck.coutp, .ss = out.ss, .grp = r.grp, .s = s};
      const long P = (long)ck.hout * ck.wout;
      if (k == 0 && st.have_keys) {     // pooled stem keys in `nxt`: decoded + normalised by this conv's stager, activations -> `cur`
        q.x = st.nxt, q.in_scale = m->ssA[0], q.in_shift = m->ssA[1], q.tail = &ktail;
      } else if (k == 0 && st.have_tail) {   // the previous block's tail rides on this conv's stager, which also writes the block output
        // with a ride in tail mode the block input is not written to HBM at all: this conv and the downsample conv are its only readers
        if (ds_ride) st.tail.out = nullptr;
        q.x = m->rawB, q.in_scale = m->ssB[0], q.in_shift = m->ssB[1], q.tail = &st.tail, q.ride = ds_ride ? &ride : nullptr;
      } else if (k == 0) {
        q.x = st.cur, q.ride = ds_ride ? &ride : nullptr;
      } else if (K == 2 && pnvo_conv_choice(m, ck, B, {}).family == ConvChoice::FP32_GENERIC && (size_t)B * P * ck.cinp * 4 <= ((size_t)48 << 20)) {
        // Second conv of a BasicBlock, small deep stage on the generic kernel: its per-tap GroupNorm+ReLU prologue costs more than one
        // streaming pass over the (L2-sized) tensor, so normalise once and run the conv on final activations.  Scratch: rawD — unless
        // the downsample conv rode and its output already sits there; `nxt` is free until the block tail.
        float *napp = ds_ride ? st.nxt : m->rawD;
        Timed t(m, s, "gn_relu_apply", 0.0, 8.0 * B * P * ck.cinp);
        HIPCHK(m, launch_apply_ss_relu(last.x, last.ss[0], last.ss[1], B, P, ck.cinp, napp, s));
        q.x = napp;
      } else {
        q.x = last.x, q.in_scale = last.ss[0], q.in_shift = last.ss[1];
      }
      if ((rc = pnvo_run_conv(m, ck, B, q)) != PNVO_OK) return rc;
      if (k == 0 && st.have_tail) std::swap(st.cur, st.nxt);
      if (k == 0) st.have_keys = st.have_tail = false;
      last = out;
    }
    const Layer &cl = m->last(b);
    const long P = (long)cl.hout * cl.wout;
    // SE block: out = se(out) * out (resnet.py:131-140) — the gate scales the last GroupNorm's scale / shift pair, the tail is unchanged
    if (b.se_r > 0) {
      if (cl.cout != cl.coutp) return fail(m, PNVO_ERR_STATE, "SE block " + b.tap + " on a channel-padded map");
      Timed t(m, s, "se_gate:" + b.tap, 2.0 * B * (2.0 * b.se_r + (double)P) * cl.cout, 4.0 * B * P * cl.cout);
      HIPCHK(m, launch_se_gate({.x = last.x, .scale = last.ss[0], .shift = last.ss[1], .w1 = b.se_w1, .b1 = b.se_b1, .w2 = b.se_w2,
                                .b2 = b.se_b2, .out_scale = m->ssE[0], .out_shift = m->ssE[1], .B = B, .P = (int)P, .C = cl.cout, .R = b.se_r}, s));
      last.ss = m->ssE;
    }
    if (ds && !ds_ride) {                                            // (riding: rawD / ssD came out of the first conv's launch)
      const Layer &cd = m->convs[b.ds];
      if ((rc = pnvo_run_conv(m, cd, B, {.x = st.cur, .y = m->rawD, .y_cstride = cd.coutp, .ss = m->ssD, .grp = r.grp, .s = s})) != PNVO_OK)
        return rc;
    }
    st.tail = BlockTail{ds ? m->rawD : st.cur, ds ? m->ssD[0] : nullptr, ds ? m->ssD[1] : nullptr, st.nxt};
    // relu(GN(last) + skip) is computed by the next conv's stager where that conv takes a tail (the compression conv behind the last
    // block: nobody else reads that block output) — of a two-conv block only: a Bottleneck block always runs its own pass and is tapped,
    // whatever pnvo_conv_takes_tail says of the conv behind it.
    if (K == 2 && pnvo_conv_takes_tail(m, m->convs[m->next_conv_after(bk)], B)) {
      st.have_tail = true;
      continue;
    }
    {
      Timed t(m, s, "residual", 0.0, 12.0 * B * P * cl.coutp);
      HIPCHK(m, launch_residual(last.x, last.ss[0], last.ss[1], st.tail.res, st.tail.res_scale, st.tail.res_shift, B, P, cl.coutp, st.nxt, s));
    }
    std::swap(st.cur, st.nxt);
    if ((rc = maybe_tap(m, b.tap.c_str(), st.cur, (size_t)B * P * cl.coutp, s)) != PNVO_OK) return rc;
  }
  return PNVO_OK;
}

// (a10) compression conv + GroupNorm(1, C); a pending tail of the last block in its stager, that block's output not materialised
int forward_compression(pnvo_handle m, int B, const FwdRequest &r, FwdState &st) {
  const Layer &comp = m->convs[m->comp];
  hipStream_t s = r.s;
  int rc = PNVO_OK;
  ConvRequest q{.x = st.cur, .y = m->comp_raw, .y_cstride = comp.coutp, .ss = m->ssC, .grp = r.grp, .s = s};
  if (st.have_tail) {
    st.tail.out = nullptr;
    q.x = m->rawB, q.in_scale = m->ssB[0], q.in_shift = m->ssB[1], q.tail = &st.tail;
  }
  if ((rc = pnvo_run_conv(m, comp, B, q)) != PNVO_OK) return rc;
  st.have_tail = false;
  if (m->tap_dst != nullptr && m->tap_name == "compression") {
    HIPCHK(m, launch_apply_ss_relu(m->comp_raw, m->ssC[0], m->ssC[1], B, (long)m->fh * m->fw, m->comp_cp, m->tapbuf, s));
    if ((rc = maybe_tap(m, "compression", m->tapbuf, (size_t)B * m->fh * m->fw * m->comp_cp, s)) != PNVO_OK) return rc;
  }
  return PNVO_OK;
}

// (a11) Flatten + Linear + ReLU, then the output head — per action model in a grouped forward (each on its own handle: its weights, bias
// rows and split-K scratch; the sample ranges are contiguous)
int forward_linears(pnvo_handle m, int B, const FwdRequest &r) {
  const pnvo_config &c = m->cfg;
  const GroupedFwd *grp = r.grp;
  if (grp == nullptr) return run_fc_head(m, B, m->comp_raw, m->ssC[0], m->ssC[1], r);
  int rc = PNVO_OK;
  bool rows_ok = !c.act_embed;
  FwdRequest rk = r;                   // model k's rows of the output; no act-embed models in a grouped forward
  rk.actions = nullptr;
  for (int k = 0; k < grp->n; ++k) rows_ok = rows_ok && fc_rows_usable(grp->h[k], B, rk);
  if (rows_ok) return run_fc_rows(m, grp->h, grp->end, grp->n, B, m->comp_raw, m->ssC[0], m->ssC[1], rk);
  const size_t crow = (size_t)m->fh * m->fw * m->comp_cp;
  for (int k = 0, start = 0; k < grp->n; start = grp->end[k++]) {
    const int Bk = grp->end[k] - start;
    pnvo_handle hk = grp->h[k];
    if (k > 0 && (rc = ensure_workspace(hk, Bk)) != PNVO_OK) return fail(m, rc, std::string("grouped forward: ") + pnvo_last_error(hk));
    rk.out = r.out + (size_t)start * c.out_dim;
    rc = run_fc_head(hk, Bk, m->comp_raw + start * crow, m->ssC[0] + (size_t)start * m->comp_cp, m->ssC[1] + (size_t)start * m->comp_cp, rk);
    if (rc != PNVO_OK) return k > 0 ? fail(m, rc, std::string("grouped forward: ") + pnvo_last_error(hk)) : rc;
  }
  return PNVO_OK;
}

int forward_body(pnvo_handle m, int B, const FwdRequest &r) {
  FwdState st{.cur = m->bufY[0], .nxt = m->bufY[1]};
  int rc;
  if ((rc = forward_stem(m, B, r, st)) != PNVO_OK || st.done) return rc;
  if ((rc = forward_blocks(m, B, r, st)) != PNVO_OK || (rc = forward_compression(m, B, r, st)) != PNVO_OK) return rc;
  return r.stop_after_compression ? PNVO_OK : forward_linears(m, B, r);   // (pnvo_forward_compression: the caller reads m->comp_raw and m->ssC)
}

// fc_rows.hip takes the two Linear layers of this handle at B samples (inference handles on float32, default kernels)
bool fc_rows_usable(pnvo_handle m, int B, const FwdRequest &r) {
  const long kp = (long)m->fh * m->fw * m->comp_cp;
  return m->opt.fc_rows >= B && B >= 1 && m->fc_rows_w != nullptr && m->train == nullptr && m->precision == 0 && m->opt.conv == 0 &&
         m->comp_cp > 0 && 256 % m->comp_cp == 0 && kp % 4 == 0 && kp / 4 <= 64L * FC_ROWS_MAXV && m->cfg.hidden % 4 == 0 &&
         (r.features_only || m->head_w_plain != nullptr);
}

// ... of up to three handles (a grouped forward: grp[k] serves the samples up to end[k]) in one launch each
int run_fc_rows(pnvo_handle m, pnvo_handle const *grp, const int *end, int ng, int B, const float *comp_raw, const float *sc, const float *sh,
                const FwdRequest &r) {
  const pnvo_config &c = m->cfg;
  FcRowsArgs a;
  std::memset(&a, 0, sizeof(a));
  a.x = comp_raw;
  a.sc = sc;
  a.sh = sh;
  a.hid = r.features_only ? r.out : m->hid;
  a.out = r.out;
  a.actions = c.act_embed ? r.actions : nullptr;
  a.B = B;
  a.Kp = m->fh * m->fw * m->comp_cp;
  a.cp = m->comp_cp;
  a.hidden = c.hidden;
  a.out_dim = c.out_dim;
  a.ngroups = ng;
  for (int k = 0; k < ng; ++k) {
    a.end[k] = end[k];
    a.w[k] = grp[k]->fc_rows_w;
    a.bias[k] = grp[k]->fc_bias;
    a.head_w[k] = grp[k]->head_w_plain;
    a.head_b[k] = grp[k]->head_bias;
  }
  Timed t(m, r.s, "conv:" + m->fc.name, 2.0 * B * (double)a.Kp * c.hidden, 4.0 * ng * (double)a.Kp * c.hidden);
  HIPCHK(m, launch_fc_rows(a, !r.features_only, r.s));
  return PNVO_OK;
}

// The hidden layer and the output head of handle m on B rows of the compression output.
int run_fc_head(pnvo_handle m, int B, const float *comp_raw, const float *sc, const float *sh, const FwdRequest &r) {
  const pnvo_config &c = m->cfg;
  float *out = r.out;
  hipStream_t s = r.s;
  int rc = PNVO_OK;
  if (fc_rows_usable(m, B, r)) {
    pnvo_handle one[1] = {m};
    const int end[1] = {B};
    if ((rc = run_fc_rows(m, one, end, 1, B, comp_raw, sc, sh, r)) != PNVO_OK) return rc;
    return r.features_only ? PNVO_OK : maybe_tap(m, "hidden", m->hid, (size_t)B * c.hidden, s);
  }
  // the output head rides on the hidden layer's split-K reduction when there is one (option head_fuse); with a training step attached
  // the head's weight is read where the optimiser keeps it (the flat parameter buffer), the bias from its re-packed copy
  bool head_rode = false;
  const float *head_w = m->train != nullptr ? pnvo_train_weight_ptr(m, m->head) : m->head_w_plain;   // (OIHW of a 1x1 conv = [out_dim][hidden])
  float *head_out = (m->opt.head_fuse && !r.features_only && c.out_dim <= 4 && head_w != nullptr) ? out : nullptr;
  if ((rc = pnvo_run_conv(m, m->fc, B, {.x = comp_raw, .in_scale = sc, .in_shift = sh, .y = m->hid, .y_cstride = c.hidden, .bias = m->fc_bias,
                                        .bias_row = c.act_embed ? r.actions : nullptr, .relu_out = 1, .head_w = head_w, .head_out = head_out,
                                        .head_rode = &head_rode, .s = s})) != PNVO_OK)
    return rc;
  if ((rc = maybe_tap(m, "hidden", m->hid, (size_t)B * c.hidden, s)) != PNVO_OK) return rc;
  if (head_rode) return PNVO_OK;
  if (r.features_only) {                           // pnvo_forward_features: `out` receives the hidden vector
    HIPCHK(m, hipMemcpyAsync(out, m->hid, (size_t)B * c.hidden * sizeof(float), hipMemcpyDeviceToDevice, s));
    return PNVO_OK;
  }
  return pnvo_run_conv(m, m->head, B, {.x = m->hid, .y = out, .y_cstride = c.out_dim, .bias = m->head_bias, .s = s});
}
}  // namespace

namespace {
// Can this call run on the RAW stager (frames straight into the stem)?  Else the raw entry materialises the observation pairs
// (pnvo_build_obs_pairs into a workspace of the handle) and takes the ordinary path: same results, the old cost.
bool raw_direct(pnvo_handle m, const float *depth_frames) {
  const StemPlan sp = pnvo_stem_plan(m, false, {});
  if (depth_frames == nullptr || !sp.raw_stager() || m->tap_dst != nullptr) return false;
  if (m->precision == 1) return true;                                // bf16 path: its stem is the mx kernel (PIECES = 1)
  return sp.h2_from_host;     // (not sp.pieces == 2: the RAW stager is not built for the training step's device-side re-pack)
}

int raw_materialise(pnvo_handle m, const uint8_t *rgb_frames, const float *depth_frames, int B, int32_t *err_flag, hipStream_t s) {
  return pnvo_raw_materialise(m, rgb_frames, depth_frames, B, nullptr, err_flag, s);
}
}  // namespace

extern "C++" {
int pnvo_check_frames(pnvo_handle m, const char *entry, const uint8_t *rgb_frames, const float *depth_frames, const float *tdv, int B,
                      const void *out) {
  return check_frames(m, entry, rgb_frames, depth_frames, tdv, B, out);
}

int pnvo_raw_materialise(pnvo_handle m, const uint8_t *rgb_frames, const float *depth_frames, int B, const float *edges, int32_t *err_flag,
                         hipStream_t s, DevBuf<float> *ws, int *cap) {
  const pnvo_config &c = m->cfg;
  if (ws == nullptr) {
    ws = m->rawws;
    cap = &m->rawws_cap;
  }
  if (B > *cap) {
    for (int k = 0; k < 3; ++k) ws[k].reset();
    *cap = 0;
    const size_t px = (size_t)B * c.height * c.width;
    if (c.n_rgb) HIPCHK(m, ws[0].alloc(px * 6));
    HIPCHK(m, ws[1].alloc(px * 2));
    if (c.n_dd) HIPCHK(m, ws[2].alloc(px * (size_t)c.n_dd));
    *cap = B;
  }
  HIPCHK(m, launch_frame_pairs(c.n_rgb ? rgb_frames : nullptr, depth_frames, B, c.height, c.width, c.n_dd / 2, ws[0], ws[1], ws[2], err_flag,
                               s, edges));
  return PNVO_OK;
}
}  // extern "C++"

int pnvo_forward_raw(pnvo_handle m, const uint8_t *rgb_frames, const float *depth_frames, const float *tdv, const int64_t *actions, int B,
                     float *out, int32_t *err_flag, void *stream) {
  if (int rc0 = check_frames(m, "pnvo_forward_raw", rgb_frames, depth_frames, tdv, B, out)) return rc0;
  const pnvo_config &c = m->cfg;
  if (c.act_embed && !actions) return fail(m, PNVO_ERR_ARG, "act_embed model needs actions");
  if (int rc0 = pnvo_check_inputs(m)) return rc0;
  HIPCHK(m, hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  if (!raw_direct(m, depth_frames)) {
    int rc = raw_materialise(m, rgb_frames, depth_frames, B, err_flag, s);
    if (rc != PNVO_OK) return rc;
    return pnvo_forward(m, c.n_rgb ? m->rawws[0] : nullptr, c.n_depth ? m->rawws[1] : nullptr, c.n_dd ? m->rawws[2] : nullptr, tdv,
                        actions, B, out, stream);
  }
  const FwdRequest r{.src = {nullptr, nullptr, nullptr, tdv}, .raw = {rgb_frames, depth_frames, err_flag}, .actions = actions, .out = out, .s = s};
  if (m->precision == 1) return forward_bf16_one(m, B, r);
  int rc = ensure_workspace(m, B);
  // (frames are uint8 / the one-hot is derived in the stager: nothing for the input-contract check to find — no stem event; one
  //  left pending by an earlier forward that failed between its stem and its wait is dropped here)
  if (rc == PNVO_OK) rc = forward_dispatch(m, B, r);
  m->stem_ev_pending = false;
  return rc;
}

// Can these handles share a grouped forward?  PNVO_OK, or the error pnvo_forward_grouped_raw would return (reason in pnvo_last_error
// of the first handle) — the caller's dispatch between one grouped and several per-model forwards asks here, no exception-driven retry.
int pnvo_grouped_supported(const pnvo_handle *hs, int n) {
  if (!hs || n < 1 || n > 3 || !hs[0]) return fail(nullptr, PNVO_ERR_ARG, "bad handle list");
  pnvo_handle m = hs[0];
  const pnvo_config &c = m->cfg;
  for (int k = 0; k < n; ++k) {
    pnvo_handle h = hs[k];
    if (!h) return fail(m, PNVO_ERR_ARG, "grouped forward: null handle");
    for (int j = 0; j < k; ++j)
      if (hs[j] == h) return fail(m, PNVO_ERR_ARG, "grouped forward: a handle appears twice");
    if (!h->loaded) return fail(m, PNVO_ERR_STATE, "grouped forward before pnvo_load_weights");
    if (std::memcmp(&h->cfg, &c, sizeof(pnvo_config)) != 0 || h->device != m->device)
      return fail(m, PNVO_ERR_ARG, "the models of a grouped forward must share architecture and device");
    const StemPlan sp = pnvo_stem_plan(h, false, {});
    if (h->precision != 0 || h->train != nullptr || h->bottleneck || c.act_embed || !sp.raw_stager() || !sp.h2_from_host ||
        h->tap_dst != nullptr || !h->opt.pool || !h->opt.tail || h->opt.conv > 1)
      return fail(m, PNVO_ERR_STATE, "grouped forward needs float32 inference handles on the default float16-piece kernels (no training step, "
                                     "no tap, no act-embed, options pieces=2 / stem=auto / conv=auto / pool / tail at their defaults)");
    for (size_t li = 1; li < h->convs.size(); ++li)
      if (h->convs[li].groups > 0 && !x3_two_pieces(h, h->convs[li]))
        return fail(m, PNVO_ERR_STATE, "grouped forward: layer " + h->convs[li].name + " of a model is range-guarded off the float16-piece form");
  }
  return PNVO_OK;
}

// One launch chain for the pairs of up to three action models (round 6; the navigation loop's call shape: 8-32 pairs per simulator
// step split over the forward / left / right models, base_trainer_with_vo.py:277-294 — three small forwards of ~58 dependent launches
// each are bound by launch latency, not work).  Pairs are sorted by model: handles[k] serves counts[k] consecutive pairs.  Every
// conv runs on conv_x3_kernel (forced; fine plan for small launches) and the tile stem, which pick a sample's weights, weight scale
// and GroupNorm affine by its model; the hidden layer and head run per model on its rows.  Same arithmetic per pair as a forward
// of its model that selects these kernels (options conv=x3, x3_rows=off, stem_form=tiles): float32-grade equal to the default
// forward of the same pairs, whose kernel choice depends on the batch size.
int pnvo_forward_grouped_raw(const pnvo_handle *handles, const int32_t *counts, int n_models, const uint8_t *rgb_frames,
                             const float *depth_frames, const float *tdv, int B, float *out, int32_t *err_flag, void *stream) {
  if (!handles || !counts || n_models < 1 || n_models > 3 || !handles[0]) return fail(nullptr, PNVO_ERR_ARG, "bad handle list");
  pnvo_handle hs[3] = {nullptr, nullptr, nullptr};
  int cnt[3] = {0, 0, 0}, ng = 0, total = 0;
  for (int k = 0; k < n_models; ++k) {
    if (counts[k] < 0 || (counts[k] > 0 && !handles[k])) return fail(handles[0], PNVO_ERR_ARG, "bad pair count / null handle");
    total += counts[k];
    if (counts[k] > 0) {
      hs[ng] = handles[k];
      cnt[ng++] = counts[k];
    }
  }
  pnvo_handle m = hs[0];
  if (ng == 0 || total != B || B <= 0 || !out) return fail(handles[0], PNVO_ERR_ARG, "pair counts do not add up to the batch / null output");
  if (ng == 1) return pnvo_forward_raw(m, rgb_frames, depth_frames, tdv, nullptr, B, out, err_flag, stream);
  const pnvo_config &c = m->cfg;
  if (int rcs = pnvo_grouped_supported(hs, ng)) return rcs;
  for (int k = 0; k < ng; ++k)
    if (int rc0 = pnvo_check_inputs(hs[k])) return rc0;
  if (!frames_match(c, rgb_frames, depth_frames, tdv)) return fail(m, PNVO_ERR_ARG, "sensor frames do not match the models' observation_space");
  if (!raw_direct(m, depth_frames)) return fail(m, PNVO_ERR_STATE, "grouped forward needs the sensor-frame stager of the float16-piece stem");
  HIPCHK(m, hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  int rc = ensure_workspace(m, B);
  if (rc != PNVO_OK) return rc;
  const PnvoOptions saved = m->opt;
  m->opt.conv = 1;                 // every GroupNorm-ed conv on conv_x3_kernel (its fine plan for small launches)
  m->opt.x3_rows = 0;              // (the row-streaming and resident-weight kernels hold ONE model's weights per workgroup)
  m->opt.x3_persist = 0;
  GroupedFwd grp{ng, {hs[0], hs[1], hs[2]}, {0, 0, 0}};
  for (int k = 0, acc = 0; k < ng; ++k) grp.end[k] = acc += cnt[k];
  rc = forward_body(m, B, {.src = {nullptr, nullptr, nullptr, tdv}, .raw = {rgb_frames, depth_frames, err_flag}, .out = out, .grp = &grp, .s = s});
  m->stem_ev_pending = false;            // (as in pnvo_forward_raw)
  m->opt = saved;
  return rc;
}

int pnvo_forward_dual_raw(pnvo_handle ha, pnvo_handle hb, const uint8_t *rgb_frames, const float *depth_frames, const float *tdv, int B,
                          float *out_a, float *out_b, int32_t *err_flag, void *stream) {
  if (int rc0 = check_dual(ha, hb, "pnvo_forward_dual_raw", B, out_a, out_b)) return rc0;
  const pnvo_config &c = ha->cfg;
  if (c.act_embed) return fail(ha, PNVO_ERR_ARG, "pnvo_forward_dual_raw covers the separate-action models");
  if (!frames_match(c, rgb_frames, depth_frames, tdv)) return fail(ha, PNVO_ERR_ARG, "sensor frames do not match the model's observation_space");
  HIPCHK(ha, hipSetDevice(ha->device));
  hipStream_t s = (hipStream_t)stream;
  if (!raw_direct(ha, depth_frames)) {
    int rc = raw_materialise(ha, rgb_frames, depth_frames, B, err_flag, s);
    if (rc != PNVO_OK) return rc;
    return pnvo_forward_dual(ha, hb, c.n_rgb ? ha->rawws[0] : nullptr, c.n_depth ? ha->rawws[1] : nullptr,
                             c.n_dd ? ha->rawws[2] : nullptr, tdv, B, out_a, out_b, stream);
  }
  pnvo_handle hs[2] = {ha, hb};
  float *outs[2] = {out_a, out_b};
  return pnvo_forward_bf16(hs, 2, B, {.src = {nullptr, nullptr, nullptr, tdv}, .raw = {rgb_frames, depth_frames, err_flag}, .s = s}, outs);
}

int pnvo_forward_features(pnvo_handle m, const float *rgb, const float *depth, const float *dd, const float *tdv,
                          const int64_t *actions, int B, float *hidden_out, void *stream) {
  if (int rc0 = check_pairs(m, "pnvo_forward_features", rgb, depth, dd, tdv, B, hidden_out)) return rc0;
  if (int rc0 = pnvo_check_inputs(m)) return rc0;
  HIPCHK(m, hipSetDevice(m->device));
  return run_forward(m, B, {.src = {rgb, depth, dd, tdv}, .actions = actions, .out = hidden_out, .features_only = true, .s = (hipStream_t)stream},
                     false);
}

extern "C++" int pnvo_forward_compression(pnvo_handle m, const float *depth, int B, void *stream) {
  if (!m) return fail(m, PNVO_ERR_ARG, "null handle");
  if (!m->loaded) return fail(m, PNVO_ERR_STATE, "pnvo_forward_compression before pnvo_load_weights");
  const pnvo_config &c = m->cfg;
  if (B <= 0 || !depth || c.n_rgb > 0 || c.n_dd > 0 || c.n_tdv > 0 || c.n_depth <= 0)
    return fail(m, PNVO_ERR_ARG, "pnvo_forward_compression takes a depth-only model and a positive batch");
  if (m->precision != 0) return fail(m, PNVO_ERR_STATE, "pnvo_forward_compression runs on the float32 path");
  if (int rc0 = pnvo_check_inputs(m)) return rc0;
  HIPCHK(m, hipSetDevice(m->device));
  return run_forward(m, B, {.src = {nullptr, depth, nullptr, nullptr}, .stop_after_compression = true, .s = (hipStream_t)stream}, false);
}

int pnvo_discretize_depth(const float *depth, int64_t n, int64_t in_stride, int bins, float *onehot,
                          int64_t out_stride, int32_t *err_flag, void *stream) {
  if (!depth || !onehot || n < 0 || bins < 1 || bins > 64) return fail(nullptr, PNVO_ERR_ARG, "bad argument");
  if (n == 0) return PNVO_OK;
  HIPCHK(nullptr, launch_discretize_depth(depth, n, in_stride, bins, onehot, out_stride, err_flag, (hipStream_t)stream));
  return PNVO_OK;
}

size_t pnvo_topdown_workspace_bytes(int N, int H, int W) { return topdown_workspace_bytes(N, H, W); }

int pnvo_topdown_view(const float *depth, int N, int H, int W, int64_t in_fstride, int64_t in_pstride,
                      const float *consts, int rows_around_center, float *out, int64_t out_fstride,
                      int64_t out_pstride, void *work, void *stream) {
  if (!depth || !out || !consts || !work || N < 0 || H <= 0 || W <= 0)
    return fail(nullptr, PNVO_ERR_ARG, "bad argument");
  if (N == 0) return PNVO_OK;
  HIPCHK(nullptr, launch_topdown(depth, N, H, W, in_fstride, in_pstride, consts, rows_around_center, out, out_fstride,
                                 out_pstride, work, (hipStream_t)stream));
  return PNVO_OK;
}

int pnvo_topdown_view_pairs(const float *depth_frames, int n_pairs, int H, int W, const float *consts, int rows_around_center,
                            float *tdv_pairs, void *work, void *stream) {
  if (!depth_frames || !tdv_pairs || !consts || !work || n_pairs < 0 || H <= 0 || W <= 0)
    return fail(nullptr, PNVO_ERR_ARG, "bad argument");
  if (n_pairs == 0) return PNVO_OK;
  const int64_t hw = (int64_t)H * W;
  HIPCHK(nullptr, launch_topdown(depth_frames, 2 * n_pairs, H, W, hw, 1, consts, rows_around_center, tdv_pairs, 2 * hw, 2, work,
                                 (hipStream_t)stream, 1));
  return PNVO_OK;
}

int pnvo_topdown_view_f64(const float *depth, int N, int H, int W, int64_t in_fstride, int64_t in_pstride,
                          const double *consts, int rows_around_center, float *out, int64_t out_fstride,
                          int64_t out_pstride, void *work, void *stream) {
  if (!depth || !out || !consts || !work || N < 0 || H <= 0 || W <= 0)
    return fail(nullptr, PNVO_ERR_ARG, "bad argument");
  if (N == 0) return PNVO_OK;
  HIPCHK(nullptr, launch_topdown_f64(depth, N, H, W, in_fstride, in_pstride, consts, rows_around_center, out, out_fstride,
                                     out_pstride, work, (hipStream_t)stream));
  return PNVO_OK;
}

int pnvo_half_to_float(const uint16_t *src, int64_t n, float *dst, void *stream) {
  if (!src || !dst || n < 0) return fail(nullptr, PNVO_ERR_ARG, "bad argument");
  if (n == 0) return PNVO_OK;
  HIPCHK(nullptr, launch_half_to_float(src, (long)n, dst, (hipStream_t)stream));
  return PNVO_OK;
}

int pnvo_dataset_pairs(const uint8_t *prev_rgb, const uint8_t *cur_rgb, const uint16_t *prev_depth, const uint16_t *cur_depth,
                       const float *tdv_frames, const int32_t *src, const int32_t *swap, int N, int M, int H, int W, int bins,
                       const float *edges, float *rgb_pairs, float *depth_pairs, float *dd_pairs, float *tdv_pairs,
                       int32_t *err_flag, void *stream) {
  if (!prev_depth || !cur_depth || !src || !swap || N <= 0 || M < 0 || H <= 0 || W <= 0 || bins < 0 || bins > 64)
    return fail(nullptr, PNVO_ERR_ARG, "bad argument");
  if (rgb_pairs && (!prev_rgb || !cur_rgb)) return fail(nullptr, PNVO_ERR_ARG, "rgb pairs requested without rgb frames");
  if (M == 0) return PNVO_OK;
  HIPCHK(nullptr, launch_dataset_pairs(prev_rgb, cur_rgb, prev_depth, cur_depth, tdv_frames, src, swap, N, M, H, W, bins, edges,
                                       rgb_pairs, depth_pairs, dd_pairs, tdv_pairs, err_flag, (hipStream_t)stream));
  return PNVO_OK;
}

int pnvo_dataset_frames(const uint8_t *prev_rgb, const uint8_t *cur_rgb, const uint16_t *prev_depth, const uint16_t *cur_depth,
                        const int32_t *src, const int32_t *swap, int N, int M, int H, int W, uint8_t *rgb_frames, float *depth_frames,
                        int32_t *err_flag, void *stream) {
  if (!prev_depth || !cur_depth || !src || !swap || N <= 0 || M < 0 || H <= 0 || W <= 0) return fail(nullptr, PNVO_ERR_ARG, "bad argument");
  if (rgb_frames && (!prev_rgb || !cur_rgb)) return fail(nullptr, PNVO_ERR_ARG, "rgb frames requested without rgb frames of the chunk");
  if (!rgb_frames && !depth_frames) return fail(nullptr, PNVO_ERR_ARG, "no output requested");
  if (M == 0) return PNVO_OK;
  HIPCHK(nullptr, launch_dataset_frames(prev_rgb, cur_rgb, prev_depth, cur_depth, src, swap, N, M, H, W, rgb_frames, depth_frames, err_flag,
                                        (hipStream_t)stream));
  return PNVO_OK;
}

namespace {
// Persistent copy workers of pnvo_stage_frames: a per-call std::thread spawn costs more than the copy of a small chunk, and the
// gather of 2N simulator frames into pinned staging is the host-side critical path of the batched boundary call (59 MB at 64
// pairs).  Heap-allocated and never destroyed: workers may still be parked on the condition variable at process exit.
struct StagePool {
  std::mutex mu;
  std::condition_variable cv_work, cv_done;
  std::vector<std::thread> workers;
  // current job: items [0, n) of array 0 then items [0, n) of array 1 (rgb frames and depth frames of a chunk in ONE wake-up)
  const void *const *src[2] = {nullptr, nullptr};
  char *dst[2] = {nullptr, nullptr};
  size_t bytes[2] = {0, 0};
  int n = 0, narr = 1;
  std::atomic<int> next{0};
  int active = 0;            // workers still inside the current job
  int want = 0;              // workers the current job admits
  unsigned long long gen = 0;
  void run(int nworkers, int narr_, const void *const *s0, size_t b0, void *d0, const void *const *s1, size_t b1, void *d1, int n_) {
    std::unique_lock<std::mutex> lk(mu);
    while ((int)workers.size() < nworkers) {
      const int id = (int)workers.size();
      workers.emplace_back([this, id] { loop(id); });
      workers.back().detach();
    }
    src[0] = s0;
    dst[0] = static_cast<char *>(d0);
    bytes[0] = b0;
    src[1] = s1;
    dst[1] = static_cast<char *>(d1);
    bytes[1] = b1;
    narr = narr_;
    n = n_;
    next.store(0);
    want = nworkers;
    active = nworkers;
    ++gen;
    cv_work.notify_all();
    lk.unlock();
    copy_items();                                   // the caller works too
    lk.lock();
    cv_done.wait(lk, [this] { return active == 0; });
  }
  void copy_items() {
    for (;;) {
      const int i = next.fetch_add(1);
      if (i >= n * narr) return;
      const int a = i / n, k = i - a * n;
      std::memcpy(dst[a] + (size_t)k * bytes[a], src[a][k], bytes[a]);
    }
  }
  void loop(int id) {
    unsigned long long seen = 0;
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv_work.wait(lk, [&] { return gen != seen; });
      seen = gen;
      if (id >= want) continue;                     // this job runs on fewer workers
      lk.unlock();
      copy_items();
      lk.lock();
      if (--active == 0) cv_done.notify_all();
    }
  }
};
StagePool *stage_pool() {
  static StagePool *p = new StagePool();
  return p;
}
std::mutex g_stage_call;                            // one gather at a time (the pool holds one job)
}  // namespace

int pnvo_stage_frames(const void *const *src, int n, size_t bytes_each, void *dst, int threads) {
  if (!src || !dst || n < 0) return fail(nullptr, PNVO_ERR_ARG, "bad argument");
  if (threads < 1) threads = 1;
  if (threads > 32) threads = 32;
  if (threads > n) threads = n > 0 ? n : 1;
  if (threads == 1 || (size_t)n * bytes_each < ((size_t)1 << 20)) {      // small jobs: a wake-up would dominate
    for (int i = 0; i < n; ++i) std::memcpy(static_cast<char *>(dst) + (size_t)i * bytes_each, src[i], bytes_each);
    return PNVO_OK;
  }
  std::lock_guard<std::mutex> lk(g_stage_call);
  stage_pool()->run(threads - 1, 1, src, bytes_each, dst, nullptr, 0, nullptr, n);   // threads - 1 workers + the caller
  return PNVO_OK;
}

int pnvo_stage_frames2(const void *const *src_a, size_t bytes_a, void *dst_a, const void *const *src_b, size_t bytes_b, void *dst_b, int n,
                       int threads) {
  if (!src_a || !dst_a || !src_b || !dst_b || n < 0) return fail(nullptr, PNVO_ERR_ARG, "bad argument");
  if (threads < 1) threads = 1;
  if (threads > 32) threads = 32;
  if (threads > 2 * n) threads = n > 0 ? 2 * n : 1;
  if (threads == 1 || (size_t)n * (bytes_a + bytes_b) < ((size_t)1 << 20)) {
    for (int i = 0; i < n; ++i) std::memcpy(static_cast<char *>(dst_a) + (size_t)i * bytes_a, src_a[i], bytes_a);
    for (int i = 0; i < n; ++i) std::memcpy(static_cast<char *>(dst_b) + (size_t)i * bytes_b, src_b[i], bytes_b);
    return PNVO_OK;
  }
  std::lock_guard<std::mutex> lk(g_stage_call);
  stage_pool()->run(threads - 1, 2, src_a, bytes_a, dst_a, src_b, bytes_b, dst_b, n);
  return PNVO_OK;
}

int pnvo_build_obs_pairs(const uint8_t *rgb_frames, const float *depth_frames, int n, int H, int W, int bins,
                         const float *tdv_consts, int rows_around_center, void *tdv_work, float *rgb_pairs, float *depth_pairs,
                         float *dd_pairs, float *tdv_pairs, int32_t *err_flag, void *stream) {
  if (!depth_frames || !depth_pairs || n < 0 || H <= 0 || W <= 0 || bins < 0 || bins > 64)
    return fail(nullptr, PNVO_ERR_ARG, "bad argument");
  if ((bins > 0) != (dd_pairs != nullptr)) return fail(nullptr, PNVO_ERR_ARG, "dd_pairs must be given exactly when bins > 0");
  if (tdv_pairs && (!tdv_consts || !tdv_work)) return fail(nullptr, PNVO_ERR_ARG, "top-down view requested without constants / workspace");
  if (n == 0) return PNVO_OK;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(nullptr, launch_frame_pairs(rgb_frames, depth_frames, n, H, W, bins, rgb_pairs, depth_pairs, dd_pairs, err_flag, s));
  if (tdv_pairs) {
    const int64_t hw = (int64_t)H * W;
    for (int k = 0; k < 2; ++k)        // prev frames then cur frames (base_trainer_with_vo.py:239-249), written into channel k
      HIPCHK(nullptr, launch_topdown(depth_frames + k * hw, n, H, W, 2 * hw, 1, tdv_consts, rows_around_center, tdv_pairs + k, 2 * hw,
                                     2, tdv_work, s));
  }
  return PNVO_OK;
}

int pnvo_ring_assemble(const uint8_t *up_rgb, const float *up_depth, const float *up_tdv, uint8_t *ring_rgb, float *ring_depth,
                       float *ring_tdv, const int32_t *idx, int n, int H, int W, uint8_t *rgb_frames, float *depth_frames, float *tdv_pairs,
                       void *stream) {
  if (!up_depth || !ring_depth || !idx || !depth_frames || n < 0 || H <= 0 || W <= 0) return fail(nullptr, PNVO_ERR_ARG, "bad argument");
  if ((up_rgb != nullptr) != (rgb_frames != nullptr) || (up_rgb != nullptr) != (ring_rgb != nullptr))
    return fail(nullptr, PNVO_ERR_ARG, "rgb buffers must be given together");
  if ((up_tdv != nullptr) != (tdv_pairs != nullptr) || (up_tdv != nullptr) != (ring_tdv != nullptr))
    return fail(nullptr, PNVO_ERR_ARG, "top-down buffers must be given together");
  if (n == 0) return PNVO_OK;
  HIPCHK(nullptr, launch_ring_assemble(up_rgb, up_depth, up_tdv, ring_rgb, ring_depth, ring_tdv, idx, n, H, W, rgb_frames, depth_frames,
                                       tdv_pairs, (hipStream_t)stream));
  return PNVO_OK;
}

int pnvo_destroy(pnvo_handle m) {
  if (!m) return PNVO_OK;
  (void)hipSetDevice(m->device);
  pnvo_train_free(m);
  pnvo_bf16_free(m);
  pnvo_small_free(m);
  pnvo_drop_graphs(m);
  if (m->cap_stream) (void)hipStreamDestroy(m->cap_stream);
  if (m->stem_ev) (void)hipEventDestroy(m->stem_ev);
  if (m->mx_prof && m->mx_prof_rs) {
    unsigned long long pr[256];
    (void)hipMemcpy(pr, m->mx_prof, 2048, hipMemcpyDeviceToHost);
    for (int w = 0; w < 12; ++w) {
      const unsigned long long *q = pr + 16 * w;
      if (q[5] == 0) continue;
      const double nt_ = (double)q[5];
      std::fprintf(stderr, "[pnvo] stem_rs wave %d (cycles per tile): k-loop with the next patch's staging %.0f  wait others %.0f  "
                   "exchange + epilogue %.0f  (%llu tiles)\n", w, q[0] / nt_, q[1] / nt_, q[2] / nt_, q[5]);
    }
  } else if (m->mx_prof) {
    unsigned long long pr[32];
    (void)hipMemcpy(pr, m->mx_prof, 256, hipMemcpyDeviceToHost);
    for (int w = 0; w < 4; ++w) {
      const double nt_ = (double)(pr[8 * w + 4] ? pr[8 * w + 4] : 1);
      std::fprintf(stderr, "[pnvo] stem_mx wave %d (cycles per tile): staging %.0f  barrier %.0f  k-loop %.0f  reduce+epilogue %.0f  "
                   "(%llu tiles)\n", w, pr[8 * w] / nt_, pr[8 * w + 1] / nt_, pr[8 * w + 2] / nt_, pr[8 * w + 3] / nt_, pr[8 * w + 4]);
    }
  }
  if (m->dd_prof) {
    unsigned long long pr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    (void)hipMemcpy(pr, m->dd_prof, 64, hipMemcpyDeviceToHost);
    const double nt_ = (double)(pr[3] ? pr[3] : 1);
    std::fprintf(stderr, "[pnvo] stem_dd phases (cycles per tile, workgroup thread 0): staging %.0f  k-loop %.0f (of which "
                 "row barriers %.0f)  epilogue %.0f  (%llu tiles)\n", (double)pr[0] / nt_, (double)pr[1] / nt_,
                 (double)pr[4] / nt_, (double)pr[2] / nt_, pr[3]);
  }
  for (auto &r : m->trecs) {
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  for (auto e : m->evpool) (void)hipEventDestroy(e);
  delete m;
  return PNVO_OK;
}

int pnvo_set_tap(pnvo_handle h, const char *name, float *dst, size_t capacity) {
  if (!h) return fail(h, PNVO_ERR_ARG, "null handle");
  h->tap_name = name ? name : "";
  h->tap_dst = name ? dst : nullptr;
  h->tap_cap = capacity;
  return PNVO_OK;
}

int pnvo_tap_shape(pnvo_handle h, const char *name, int B, int64_t shape[4]) {
  if (!h || !name || !shape) return fail(h, PNVO_ERR_ARG, "null argument");
  const pnvo_config &c = h->cfg;
  const std::string n = name;
  auto set = [&](int64_t a, int64_t b, int64_t cc, int64_t d) {
    shape[0] = a;
    shape[1] = b;
    shape[2] = cc;
    shape[3] = d;
    return PNVO_OK;
  };
  if (n == "input") return set(B, c.height, c.width, h->CP);
  if (n == "stem_conv") return set(B, h->Hs, h->Ws, c.baseplanes);
  if (n == "maxpool") return set(B, h->Hp, h->Wp, c.baseplanes);
  if (n == "compression") return set(B, h->fh, h->fw, h->comp_cp);
  if (n == "hidden") return set(B, 1, 1, c.hidden);
  for (const Block &b : h->blocks)
    if (n == b.tap) return set(B, h->last(b).hout, h->last(b).wout, h->last(b).coutp);
  return fail(h, PNVO_ERR_ARG, "unknown tap '" + n + "'");
}

int pnvo_layer_kernel(pnvo_handle h, const char *name, int B, char *family, size_t cap, double *executed_flops) {
  if (!h || !name || !family || cap == 0 || B <= 0) return fail(h, PNVO_ERR_ARG, "bad argument");
  for (size_t li = 1; li < h->convs.size(); ++li) {
    const Layer &l = h->convs[li];
    if (l.name != name) continue;
    const ConvChoice c = pnvo_conv_choice(h, l, B, {});
    if (c.family != ConvChoice::GROUP && pnvo_stem_plan(h, false, {}).writes_slots() && pnvo_small_usable(h, B)) {   // a phase of the persistent small-batch kernel (fp32 MFMA)
      std::snprintf(family, cap, "smallnet");
      if (executed_flops) {
        const int mb = l.cinp >= 128 ? 1 : l.cinp >= 64 ? 2 : 4, th = mb == 4 ? 8 : 4, tw = mb == 1 ? 4 : 8;
        *executed_flops = 2.0 * B * ((l.hout + th - 1) / th) * ((l.wout + tw - 1) / tw) * (th * tw) * (double)rup(l.cout, 16) * l.cinp * l.k * l.kw;
      }
      return PNVO_OK;
    }
    const Layer *c1 = l.block >= 0 && h->blocks[l.block].ds == (int)li ? &h->convs[h->blocks[l.block].conv[0]] : nullptr;
    const ConvChoice cr = c1 ? pnvo_conv_choice(h, *c1, B, {.ride = &l}) : ConvChoice{};
    if (c1 && cr.family == ConvChoice::X3) {        // a downsample conv riding on its block's first conv
      std::snprintf(family, cap, "x2-rides");
      if (executed_flops) *executed_flops = 3.0 * 2.0 * (double)B * cr.x3p.tiles_r * cr.x3p.tiles_c * cr.x3p.MT * 32.0 * l.coutp * (double)l.cinp;
      return PNVO_OK;
    }
    const char *const names[] = {"group", c.x3p.np == 2 ? "x2" : "x3", "fp32-lds", "fp32-generic"};   // ConvChoice::Family
    std::snprintf(family, cap, "%s", names[c.family]);
    if (executed_flops) *executed_flops = c.flops;
    return PNVO_OK;
  }
  return fail(h, PNVO_ERR_ARG, std::string("no residual-stage conv named '") + name + "'");
}

int pnvo_conv_x3_describe(const int *problem, int n, char *buf, size_t cap) {
  if (!buf || cap == 0) return fail(nullptr, PNVO_ERR_ARG, "bad argument");
  if (problem == nullptr) return conv_x3_describe(nullptr, n, buf, cap) == 0 ? PNVO_OK : PNVO_ERR_ARG;   // (past the last row: no message)
  if (n != 23) return fail(nullptr, PNVO_ERR_ARG, "a conv_x3 problem has 23 fields");
  const int *v = problem;
  ConvX3Problem q{.B = v[0], .H = v[1], .W = v[2], .CIN = v[3], .Ho = v[4], .Wo = v[5], .COUTP = v[6], .ks = v[7], .stride = v[8], .np = v[9],
                  .mode = v[10], .tail_scaled = v[11] != 0, .absmax = v[12] != 0, .ds = v[13] != 0};
  q.opt = {.force = v[14], .strip = v[15], .fine = v[16], .w8 = v[17], .m16 = v[18], .ksw = v[19], .persist_wgs = v[20], .rows = v[21], .num_cus = v[22]};
  conv_x3_describe(&q, 0, buf, cap);
  return PNVO_OK;
}

int pnvo_wgrad_describe(const int *problem, int n, char *buf, size_t cap) {
  if (!buf || cap == 0) return fail(nullptr, PNVO_ERR_ARG, "bad argument");
  if (problem == nullptr) return wgrad_describe(nullptr, n, buf, cap) == 0 ? PNVO_OK : PNVO_ERR_ARG;   // (past the last row: no message)
  if (n != 16) return fail(nullptr, PNVO_ERR_ARG, "a weight-gradient problem has 16 fields");
  const int *v = problem;
  const WgradProblem q{.B = v[0], .H = v[1], .W = v[2], .CIN = v[3], .Ho = v[4], .Wo = v[5], .COUT = v[6], .DYC = v[7], .KH = v[8], .KW = v[9],
                       .stride = v[10], .pad = v[11], .mode = v[12], .np = v[13], .wgrad3 = v[14], .wgrad = v[15]};
  for (int k = 0; k < 11; ++k)
    if (v[k] <= 0) return fail(nullptr, PNVO_ERR_ARG, "a weight-gradient problem's sizes are positive");
  if (q.pad < 0 || q.mode < 0 || q.mode > 2 || (q.np != 2 && q.np != 3) || (q.wgrad3 | 1) != 1 || q.wgrad < 0 || q.wgrad > 2)
    return fail(nullptr, PNVO_ERR_ARG, "mode is 0-2, np 2 or 3, wgrad3 0 or 1, wgrad 0-2");
  return wgrad_describe(&q, 0, buf, cap) == 0 ? PNVO_OK : PNVO_ERR_ARG;
}

int pnvo_conv_fp32_describe(const int *problem, int n, char *buf, size_t cap) {
  if (!buf || cap == 0) return fail(nullptr, PNVO_ERR_ARG, "bad argument");
  if (problem == nullptr) return conv_fp32_describe(nullptr, n, buf, cap) == 0 ? PNVO_OK : PNVO_ERR_ARG;   // (past the last row: no message)
  if (n != 33) return fail(nullptr, PNVO_ERR_ARG, "a float32-MFMA conv problem has 33 fields");
  const int *v = problem;
  ConvFp32Problem q{.B = v[0], .H = v[1], .W = v[2], .CIN = v[3], .Ho = v[4], .Wo = v[5], .COUT = v[6], .COUTP = v[7], .KH = v[8], .KW = v[9],
                    .stride = v[10], .pad = v[11], .up = v[12], .y_cstride = v[13], .mode = v[14], .accum = v[15] != 0, .y_sh = v[16], .y_sw = v[17],
                    .y_oh = v[18], .y_ow = v[19], .y_H = v[20], .y_W = v[21], .linear = v[22] != 0, .stats = v[23] != 0, .ksplit_ok = v[24] != 0,
                    .head = v[25], .lds_ok = v[26] != 0};
  q.opt = {.tile = v[27], .wsplit = v[28], .form = v[29], .wave_wgs = v[30], .wave_nt = v[31], .num_cus = v[32]};
  for (int k : {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13, 32})
    if (v[k] <= 0) return fail(nullptr, PNVO_ERR_ARG, "a float32-MFMA conv problem's sizes are positive");
  if (q.pad < 0 || (q.up != 1 && q.up != 2) || q.mode < 0 || q.mode > 2 || q.opt.wsplit < -1 || q.opt.wsplit > 1 || q.opt.form < 0 || q.opt.form > 2 ||
      q.opt.tile < 0 || q.opt.wave_wgs < 0 || q.head < 0 || q.y_sh < 0 || q.y_sw < 0)
    return fail(nullptr, PNVO_ERR_ARG, "pad >= 0, up 1 or 2, mode 0-2, fp32_wsplit -1..1, fp32_form 0-2, the rest non-negative");
  return conv_fp32_describe(&q, 0, buf, cap) == 0 ? PNVO_OK : PNVO_ERR_ARG;
}

int pnvo_timing_mode(pnvo_handle h, int mode) {
  if (!h) return fail(h, PNVO_ERR_ARG, "null handle");
  h->timing = mode ? 1 : 0;
  return PNVO_OK;
}

int pnvo_timing_read(pnvo_handle h, pnvo_kernel_time *entries, int cap, int *n_out) {
  if (!h || !n_out) return fail(h, PNVO_ERR_ARG, "null argument");
  for (auto &r : h->trecs) {
    HIPCHK(h, hipEventSynchronize(r.b));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, r.a, r.b));
    h->tentries[r.entry].total_ms += ms;
    h->evpool.push_back(r.a);
    h->evpool.push_back(r.b);
  }
  h->trecs.clear();
  const int n = (int)h->tentries.size();
  *n_out = n;
  for (int k = 0; k < n && k < cap && entries; ++k) entries[k] = h->tentries[k];
  h->tentries.clear();
  h->tindex.clear();
  return PNVO_OK;
}

size_t pnvo_packed_conv_floats(int cout, int cin, int kh, int kw) { return packed_conv_floats(cout, cin, kh, kw); }

int pnvo_pack_conv_weight(const float *oihw, int cout, int cin, int kh, int kw, float *out) {
  if (!oihw || !out || cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0) return fail(nullptr, PNVO_ERR_ARG, "bad argument");
  pack_conv_weight(oihw, cout, cin, kh, kw, out);
  return PNVO_OK;
}

}  // extern "C"
