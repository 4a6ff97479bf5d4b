// pnvo_model.h — host-side model state shared by pnvo_api.hip (inference) and pnvo_train_api.hip (training step).
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <functional>
#include <string>
#include <vector>

#include "../../include/pnvo.h"
#include "pnvo_internal.h"
#include "dev_buf.h"

using pnvo::DevBuf;
using pnvo::DevPair;

static inline int rup(int x, int m) { return (x + m - 1) / m * m; }
static inline int halve(int x) { return (x - 1) / 2 + 1; }

struct Layer {
  std::string name, gn;     // state_dict prefixes (conv weight, following GroupNorm)
  int cin = 0, cinp = 0, cout = 0, coutp = 0, k = 1, kw = 1, stride = 1, pad = 0;
  int hin = 0, win = 0, hout = 0, wout = 0, groups = 1;
  DevBuf<float> wpk, gamma, beta;
  std::vector<float> host_w;  // OIHW copy of the loaded weight (source of the bf16 packing, pnvo_bf16.hip)
  // float32-on-bf16-pipe path (conv_x3.hip): three-piece packed weights, built on first use after a (re)load
  DevBuf<unsigned short> wpk_x3;
  unsigned long long x3_gen = 0;
  // two-piece float16 form of the same kernel (inference): packed weights, the inverse of their power-of-two scale, and an
  // upper bound of |input activation| from the producers' GroupNorm parameters (float16 pieces need it below 65504)
  DevBuf<unsigned short> wpk_x2;
  unsigned long long x2_gen = 0;
  float x2_oscale = 1.f;
  float in_bound = 3.0e38f;
  int block = -1;           // index into pnvo_model_s::blocks of the residual block this conv belongs to (-1: stem, compression)
  // grouped conv (ResNeXt, resnet.py:63): the CONV's group count (`groups` above is the GroupNorm's); the weight is [cout, cin / cgroups, k, k]
  int cgroups = 1;
  DevBuf<float> wpk_grp;    // conv_group.hip's packing of it
};

// One residual block of the plan: where its convs sit in pnvo_model_s::convs.  build_plan fills the table; every walk over the
// residual stages (forwards, backward, workspaces, range guard, taps) iterates it.  The block output has the geometry of its last
// conv: hout x wout x coutp.
struct Block {
  int stage = 0, index = 0;       // layer<stage>.<index>, stage 1..4
  int nconv = 0;                  // 2 (BasicBlock) or 3 (Bottleneck)
  int conv[3] = {-1, -1, -1};     // chain order
  int ds = -1;                    // the downsample conv of the skip branch, or -1 (identity)
  std::string tap;                // "layer<stage>.<index>"
  // squeeze-and-excite branch (resnet.py:71-93) on the block's last GroupNorm output: se.excite.0 [se_r, C], se.excite.2 [C, se_r]
  int se_r = 0;                   // int(C / 16); 0: no SE branch
  DevBuf<float> se_w1, se_b1, se_w2, se_b2;
};

// Per-handle options (pnvo_set_option; defaults from the PNVO_* environment, read ONCE in pnvo_create).
struct PnvoOptions {
  int stem = 0;        // 0 auto (bf16-matrix-core stem when the model's modalities fit it, else one-hot-aware, else dense), 1 mx, 2 dd, 3 dense
  int conv = 0;        // 0 auto (conv_x3 for launches of >= 192 workgroups, fp32-MFMA kernels below), 1 x3 at any size, 2 fp32, 3 generic
  int stem_form = 0;   // float16-piece stem: 0 auto (fast resident weights when every workgroup gets >= 4 tiles, else one tile per workgroup), 2 one tile per workgroup, 3 resident weights in the tile kernel's summation order (stem_rs_kernel), 4 fast (its own order)
  int pieces = 2;      // operand pieces of conv_x3 at inference: 2 float16 (three product terms) or 3 bf16 (six exact terms)
  int train_pieces = 2;  // the same choice for the TRAINING forward's convs (their backward-data convs keep three bf16 pieces:
                         //   gradients do not fit float16's range)
  int x3_rows = 1;     // 32 -> 32 channel 3x3 stride-1 convs on the row-streaming kernel (conv_rows.hip) where it takes the launch
  int x3_persist = 1;  // shallow-stage 3x3 convs on the persistent form of conv_x3 (next tile's patch fetched during the K loop)
  int x3_strip = 1;    // 64- / 128-channel stride-1 convs on wide strip tiles with the N-tiles split over blockIdx.y (half the weight bytes per pixel)
  int x3_fine = 1;     // small launches of the float16-piece convs take one N-tile per workgroup instead of falling back to the fp32-pipe kernels
  int x3_m16 = 1;      // MFMA-count-bound stride-1 convs (one-tile-per-sample 256-channel launches from 200 tiles on, 128-channel strips) on 16x16x32 MFMAs: M padded to 16 rows
  int x3_w8 = 1;       // 256-channel convs on 6 x 11 maps with a tile per CU or more: eight waves of (3,1) tiles per workgroup (two per SIMD) instead of four of (3,2)
  int x3_ksplit = 1;   // fine-plan conv tiles of three / four M-tiles behind >= 128 input channels: the four waves split the K walk, partial sums meet in LDS
  int fp32_tile = 0;   // float32-MFMA generic kernel: 0 auto, 10*MT+NT forces that wave tile from 8192 output pixels on (experiment knob)
  int fp32_wsplit = -1;  // ... its four waves share one tile and split the reduction: -1 auto, 1 wherever possible, 0 never
  int fp32_form = 0;   // LDS-staged float32 3x3 convs: 0 auto (wave-private patches from 64 input channels on), 1 tile, 2 wave
  int wave_wgs = 3;    // ... workgroups per CU of the wave kernel's persistent grid (0: as many as LDS allows)
  int wave_nt = 1;     // ... 1: one N-tile per wave item; else two where the layer's N-tile count is even
  int fc_rows = 48;    // up to this many samples the hidden layer and the head run as fc_rows.hip's two launches (every model of a grouped forward in one)
  int head_fuse = 1;   // the output head (Linear hidden -> out_dim) is computed by the hidden layer's split-K reduction launch (one launch less)
  int ds_fuse = 1;     // the 1x1 stride-2 downsample conv rides on its block's first 3x3 conv (bit-identical raw output, one launch less, block input read once)
  int gn_fuse = 1;     // conv_x3 launches with one tile per sample finalise their GroupNorm themselves (bit-identical, one launch less)
  int x3_s2 = 1;       // stride-2 convs on conv_x3
  int tail = 1;        // BasicBlock tails fused into the next conv's stager (0: residual_kernel)
  int pool = 1;        // max-pool fused into the stem's epilogue (0: gn_relu_maxpool_kernel)
  int graph = 0;       // forward replayed from a captured hipGraph
  int stem_dbg = 0, stem_dbg_pad = 0;   // developer instrumentation of the stem kernels
  int wgrad_stem = 0;  // 0 bf16 matrix cores, 1 fp32
  int wgrad3 = 1;      // weight gradient of the 3x3 stride-1 convs: 1 bf16 matrix cores (wgrad_x3.hip), 0 fp32 kernels
  int wgrad = 0;       // weight-gradient kernel families (wgrad_plan): 0 auto, 1 lds9 (nine-wave kernel where wgrad3 = 0 would take the twelve-wave one), 2 generic (no LDS-staged family, the float32 stem kernel included)
  int pool_bwd = 1;    // max-pool backward fused into the stem's GroupNorm backward
  int dgrad = 1;       // stride-2 backward-data as four parity-phase convs (0: masked taps)
  int bf16_fuse = 1;   // bf16 path: block tails fused
  int input_fallback = 1;   // contract-breaking input (fractional rgb, soft depth codes): re-run on the dense stem and stay on it
  int small_net = 1;   // batches of <= small_max pairs: everything behind the stem conv in ONE persistent launch (smallnet.hip)
  int small_max = 3;   // largest batch the persistent kernel takes (1..4; round 6: the per-layer launches with their fine plans win from 4 pairs on — 0.370 against 0.400 ms)
  int small_prof = 0;  // developer instrumentation: per-phase times of the persistent kernel on stderr
  int small_coop = 1;  // cooperative launch (hipLaunchCooperativeKernel): every workgroup resident by the runtime's guarantee, also next to other
                       // processes' kernels (+17 us); 0: plain launch of <= 144 workgroups (one per CU) for a process that owns the GPU
};

// The plan options of the float32-MFMA kernels as options o state them (every ConvFp32Problem of a handle takes them from here).
inline pnvo::ConvFp32Opts pnvo_fp32_opts(const PnvoOptions &o, int num_cus) {
  return {.tile = o.fp32_tile, .wsplit = o.fp32_wsplit, .form = o.fp32_form, .wave_wgs = o.wave_wgs, .wave_nt = o.wave_nt, .num_cus = num_cus};
}

struct TimingRec {
  hipEvent_t a, b;
  int entry;
};

struct pnvo_model_s {
  pnvo_config cfg;
  int device = 0;
  std::string err;
  std::string note;           // pnvo_last_note: what a SUCCESSFUL call changed on the handle (never an error)
  bool loaded = false;

  int C = 0, CP = 0;                 // input channels, padded to 8
  int Hs = 0, Ws = 0, Hp = 0, Wp = 0, fh = 0, fw = 0, comp_c = 0, comp_cp = 0;
  std::vector<Layer> convs;          // stem, residual stages in execution order, compression
  std::vector<Block> blocks;         // the residual blocks in forward order
  int comp = -1;                     // index of the compression conv in convs
  const Layer &last(const Block &b) const { return convs[b.conv[b.nconv - 1]]; }   // its geometry is the block output's
  // the conv that reads block k's output: the next block's first conv, or the compression conv
  int next_conv_after(size_t k) const { return k + 1 < blocks.size() ? blocks[k + 1].conv[0] : comp; }
  Layer fc, head;
  DevBuf<float> fc_bias, head_bias;   // fc_bias has 1 or n_acts+1 rows
  DevBuf<float> fc_rows_w;                   // [hidden][fh * fw * comp_cp]: the hidden layer's weight rows in the activation's order (fc_rows.hip)
  DevBuf<float> head_w_plain;                // [out_dim][hidden]: the head's weight as loaded (the head riding on the hidden layer's split-K reduction)
  std::vector<float> mean, stdev;    // host copies for the assemble kernel arguments (reference channel order)
  // fused stem: K-order of the stem = observation tensors concatenated (rgb | depth | dd | tdv), 2-channel pieces
  std::vector<int> stem_ref_of_new;  // new channel -> reference channel (vo_cnn.py:169-174 order), -1 = pad
  std::vector<int> stem_tensor_of_new, stem_ch_of_new;
  DevBuf<float> stem_sc, stem_sh, zero_page; // whitening table in the new order
  DevBuf<float> kpart;               // split-K partials of the linear layers (ConvFp32Plan::scratch_floats); only grows
  DevBuf<float> stem_wpk16;          // stem weights packed for the LDS-staged 16x16x4 kernel
  int CPL = 0;                       // stem channels per pixel in LDS (C rounded up to 16)
  // one-hot-aware stem (stem_dd.hip): dense channels + indicator on the matrix cores, depth bins as a table gather
  bool dd_ok = false;
  int dd_bins = 0;
  std::vector<int> dd_dense_tensor, dd_dense_ch;   // dense channel d -> (observation tensor, channel), -1 = indicator/pad
  DevBuf<float> dd_wpk, dd_table, dd_sc, dd_sh;
  DevBuf<int> dd_flag;               // host-mapped copy of dd_flag_dev (published by the kernel behind the stem): what the HOST reads
  DevBuf<int> dd_flag_dev;           // device memory: raised by a fused stem whose stager met a value outside the observation contract;
                                     // read by the predicated repair launches (a host-mapped flag costs every wave a PCIe round trip)
  DevBuf<unsigned long long> dd_prof;      // PNVO_STEM_DBG=9: {staging, K loop, epilogue} cycles, tiles

  // stem on the bf16 matrix cores (stem_mx.hip): exact three-piece bf16 weights -> float32 results (inference default)
  bool mx_ok = false;
  DevBuf<unsigned short> mx_wpk3;            // three-piece packing (float32 results)
  DevBuf<unsigned short> mx_wpk2;            // two float16 pieces (inference default) and the inverse of their scale
  float mx_oscale = 1.f;
  DevBuf<float> mx_scale2_dev;               // training: {scale, 1/scale} of mx_wpk2 as the device-side re-pack chose it
  bool mx_wpk2_dev = false;                  // mx_wpk2 currently holds the device-side re-pack (scale in mx_scale2_dev), not the host's
  std::vector<float> mx_wk, mx_wk_swapped;   // host [cout][32 slots][49]: whitening-folded weights, as is / for the
                                             //   (cur, prev) channel-swapped pair (geometric-invariance dual forward)
  int mx_xslot[4] = {-1, -1, -1, -1};        // K-slots of the float-modality channels
  std::vector<int> mx_slot_ref, mx_slot_new; // K-slot -> reference channel / position in the stem's tensor-major order (-1: none)
  DevBuf<float> mx_pages;                    // 64 zeros (out-of-image reads)
  DevBuf<unsigned long long> mx_prof;        // PNVO_STEM_DBG=9: per-wave phase cycle sums of stem_mx / stem_ps
  bool mx_prof_rs = false;                   //   ... the last stem launch was the resident-weight form
  int num_cus = 256;                         // compute units of the device (grid of the persistent kernels)
  bool train_mx = false;                     // the attached training step rebuilds the mx stem operands every step
  PnvoOptions opt;
  bool dense_sticky = false;                 // an input outside the mx/dd stems' contract was met: this handle stays on the dense stem
  int fallback_count = 0;                    // forwards re-run on the dense stem
  DevBuf<float> stats_ds;                    // GroupNorm partials of a downsample conv riding on its block's first conv (stats_floats)
  hipEvent_t stem_ev = nullptr;              // recorded behind a contract-checking stem launch (pnvo_mark_stem)
  bool stem_ev_pending = false;
  DevBuf<float> rawws[3];                    // rgb / depth / dd pair tensors of the materialising fallback of the raw entry
  int rawws_cap = 0;                         // batch they are sized for
  int precision = 0;                         // pnvo_set_precision: 0 float32 (default), 1 bfloat16 (BASELINE config 3)
  unsigned long long load_gen = 0;           // bumped by pnvo_load_weights (operands derived lazily are rebuilt)
  unsigned long long weights_gen_at_load = 0;  // weights_gen as pnvo_load_weights left it
  unsigned long long uid = 0;                // process-unique handle id (cache keys that must not alias a re-used address)
  unsigned long long weights_gen = 0;        // bumped by pnvo_load_weights AND by every pnvo_train_refresh (conv_x3 operands)
  void *bf = nullptr;                        // Bf16State (pnvo_bf16.hip)

  int cap = 0;                       // batch the workspace is sized for
  DevBuf<float> xin, stem_raw, bufY[2];
  DevBuf<float> rawA, rawB, rawD, rawC, comp_raw, hid, stats;
  bool bottleneck = false;           // resnet50 / resnet101 backbone and their ResNeXt / SE forms
  bool grouped_se = false;           // a block with a grouped conv or an SE branch: inference on float32 only, no backward
  DevPair<float> ssA, ssB, ssD, ssC;
  DevPair<float> ssE;                // SE models: the gated scale / shift pair of a block's last GroupNorm (se_gate.hip)
  DevBuf<float> tapbuf;

  std::string tap_name;
  float *tap_dst = nullptr;
  size_t tap_cap = 0;

  void *train = nullptr;             // TrainState (pnvo_train_api.hip), present after pnvo_train_attach
  void *small = nullptr;             // SmallNet (smallnet.hip): the persistent small-batch kernel's operands, built on first use

  // Opt-in (PNVO_GRAPH=1): the whole forward (~60 launches) captured once per (batch, tensor addresses, kernel
  // selection) into a hipGraph and replayed (see pnvo_forward for the measurement that keeps it off by default).
  struct GraphEntry {
    const void *key[8];
    int B;
    hipGraph_t graph;
    hipGraphExec_t exec;
    unsigned long long stamp;
  };
  std::vector<GraphEntry> graphs;
  std::vector<GraphEntry> seen;      // call shapes met once (captured when they come back: no capture for one-off calls)
  DevBuf<float> out_ws;              // [cap, out_dim]: the graph's output (copied to the caller's tensor after replay)
  hipStream_t cap_stream = nullptr;
  int graph_mode = -1;               // -1: read PNVO_GRAPH on first use; 0 off; 1 on
  unsigned long long graph_clock = 0;

  int timing = 0;
  std::vector<pnvo_kernel_time> tentries;
  std::map<std::string, int> tindex;
  std::vector<TimingRec> trecs;
  std::vector<hipEvent_t> evpool;
};


// The tail of the previous BasicBlock (resnet.py:47-55) handed to the next block's first conv instead of a pass of its own:
// that conv's input is relu(x*in_scale+in_shift + r), r = res or res*res_scale+res_shift, and it also writes it to `out`
// (the block output: the next skip branch / downsample conv read it).
// res == nullptr: the conv's input x holds the pooled stem keys of stem_mx.hip (POOL); the conv decodes them, applies
// |in_scale|, in_shift and ReLU, and writes the pooled activations to `out`.
struct BlockTail {
  const float *res, *res_scale, *res_shift;
  float *out;
};

// The 1x1 stride-2 downsample conv of a stride-2 BasicBlock (resnet.py:192-195) riding on the launch of the block's first 3x3 conv
// (conv_x3_kernel<.., DSF>): raw output -> y, GroupNorm scale / shift -> ss[0] / ss[1] (finalised with the conv's own).
struct DsRide {
  const Layer *cd;
  float *y;
  float *const *ss;
  float *mu, *rstd;      // [B,groups] statistics of the downsample GroupNorm for a backward pass, or nullptr
};

// A grouped forward (pnvo_forward_grouped_raw): pairs of n = 2 or 3 action models in one launch chain, sorted by model.  h[k] serves
// the samples up to end[k] (h[0] = the handle that runs the chain); kernels pick a sample's operands by its model.
struct GroupedFwd {
  int n;
  pnvo_model_s *h[3];
  int end[3];
};

// One conv launch of pnvo_run_conv: a call site sets the members it uses (designated initializers, in this order).
struct ConvRequest {
  const float *x = nullptr;
  const float *in_scale = nullptr, *in_shift = nullptr;   // [B,CIN] GroupNorm of the producer: relu(x*scale+shift) while staging
  float *y = nullptr;
  int y_cstride = 0;                         // channel stride of y
  float *const *ss = nullptr;                // [2]: GroupNorm scale / shift of this conv's output; nullptr: no GroupNorm (linear layers)
  float *mu = nullptr, *rstd = nullptr;      // [B,groups] statistics of that GroupNorm for a backward pass, or nullptr
  const float *bias = nullptr;
  const int64_t *bias_row = nullptr;         // [B] row of `bias` per sample, or nullptr (row 0)
  int relu_out = 0;
  const float *const *src = nullptr;         // fused stem: the observation tensors A is gathered from (x unused)
  const BlockTail *tail = nullptr;
  const DsRide *ride = nullptr;
  const GroupedFwd *grp = nullptr;
  // the output head on the hidden layer's split-K reduction launch (when there is one): its weight [out_dim][hidden], where it writes
  // [B][out_dim], and whether it did (else the caller launches the head)
  const float *head_w = nullptr;
  float *head_out = nullptr;
  bool *head_rode = nullptr;
  hipStream_t s = nullptr;
};

// Sensor frames of a raw entry (pnvo_forward_raw, pnvo_forward_grouped_raw, pnvo_forward_dual_raw): the stem's RAW stager reads them
// instead of the rgb / depth / discretised-depth pair tensors.
struct RawFrames {
  const unsigned char *rgb = nullptr;        // [B][2][H][W][3] uint8, or nullptr (model without rgb)
  const float *depth = nullptr;              // [B][2][H][W]; non-null: the call runs on sensor frames
  int *err = nullptr;                        // device flag: a depth outside [0, 1]
  const float *edges = nullptr;              // HOST float[bins + 1]: bin edges of the one-hot depth, or nullptr: float32(i / bins)
};

// Which stem a forward of this handle launches and what follows from that.  The rule is written once, in pnvo_stem_plan; the stem
// launch, the workspace, the pooled-key and small-batch paths, the raw and grouped entries and pnvo_layer_kernel read this value.
struct StemPlan {
  // whose place in the forward and whose statistics-slot layout: stem_mx.hip / stem_rs.hip, stem_dd.hip, stem_lds.hip, pnvo_run_conv
  enum Kernel { MX, DD, LDS, GENERIC } kernel = GENERIC;
  bool lds_serves = false;   // stem_lds.hip serves this model: the kernel the input-contract repair and the stand-in run
  bool standin = false;      // dense_sticky: stem_lds_kernel<.., PAIRED> launches in the MX / DD stem's place
  bool repairs = false;      // a stand-in predicated on the contract flag follows the launch (decided on the device)
  bool marks = false;        // pnvo_mark_stem has something to publish / record
  int pieces = 3;            // MX: operand pieces, 2 float16 or 3 bf16
  bool h2_from_host = false; // MX: option pieces=2 and the float16 operand as pnvo_load_weights packed it is current.  The raw and the
                             //   grouped entries ask for this; `pieces` also takes the training step's device-side re-pack (mx_wpk2_dev)
  int slots = 0;             // statistics slots per sample the launch leaves in m->stats ([B][slots][CP][2]); 0: GENERIC (no slots handed on)
  bool writes_slots() const { return kernel != GENERIC; }   // per-tile statistics land in m->stats (smallnet.hip can take over)
  bool pools() const { return kernel == MX; }               // can emit pooled keys
  bool raw_stager() const { return kernel == MX && !standin; }   // sensor frames can go straight into the stem
};

// What a conv launch wants of its kernel beyond layer and batch (designated initializers, in this order).  No buffer pointers: the
// schedule asks before it builds a ConvRequest; pnvo_run_conv derives the launch's own ask from its request.
struct ConvAsk {
  bool gn = true;              // a GroupNorm follows: the launch leaves statistics slots
  bool plain = false;          // fused stem source, bias, output ReLU or y_cstride != coutp (linear layers, generic stem): conv_mfma.hip only
  bool affine = false;         // the producer's GroupNorm scale / shift (+ ReLU) applied while staging
  enum Tail { NONE, SKIP, SKIP_SCALED, KEYS } tail = NONE;   // BlockTail: skip tensor, skip tensor with its own scale / shift, pooled stem keys
  const Layer *ride = nullptr; // the block's downsample conv rides on the launch (DsRide::cd)
  bool rows_form = false;      // the launch itself asks: conv_rows32_kernel may take the tile plan's place (see pnvo_conv_choice)
};

// Which kernel family runs a residual-stage conv at B samples for an ask, and what follows from that.  The rule is written once, in
// pnvo_conv_choice; pnvo_run_conv executes the value, the workspace sizes the statistics buffers from it, the forward schedules
// (tails, rides, the small-generic pre-pass) and pnvo_layer_kernel read it.
struct ConvChoice {
  // conv_group.hip, conv_x3.hip / conv_rows.hip, conv3_lds.hip, conv_mfma.hip
  enum Family { GROUP, X3, FP32_LDS, FP32_GENERIC } family = FP32_GENERIC;
  pnvo::ConvX3Problem x3q{};   // X3: the launch's problem and its plan
  pnvo::ConvX3Plan x3p;
  pnvo::ConvFp32Problem fp32q{};   // FP32_*: the layer's problem as the ask states it, and its plan (family, wave tile and slots hold for
  pnvo::ConvFp32Plan fp32p;        //   the launch whatever its operand mode: conv_fp32_plan)
  int slots = 0;               // statistics slots per sample the launch writes ([B][slots][coutp][2] in m->stats)
  double flops = 0.0;          // executed matrix-core FLOPs (X3: of the tile plan)
};

// One stem launch of pnvo_run_stem (designated initializers, in this order).
struct StemRequest {
  const float *src[4] = {nullptr, nullptr, nullptr, nullptr};   // rgb | depth | dd | tdv pair tensors
  RawFrames raw;
  float *y = nullptr;                        // raw stem output
  float *const *ss = nullptr;                // [2]: GroupNorm scale / shift
  float *mu = nullptr, *rstd = nullptr;      // [B,groups] statistics for a backward pass, or nullptr
  int *pool_keys = nullptr;                  // pooled order-preserving keys (MX only), or nullptr
  bool train_fwd = false;                    // the training forward's stem
  int *slots_out = nullptr;                  // receives the statistics slots per sample the launch wrote
  bool skip_finalize = false;                // the consumer of those slots reduces them itself (smallnet.hip)
  const GroupedFwd *grp = nullptr;
  hipStream_t s = nullptr;
};

// One inference forward (forward_dispatch / forward_body, pnvo_forward_bf16, pnvo_small_forward, the Linear layers).
struct FwdRequest {
  const float *src[4] = {nullptr, nullptr, nullptr, nullptr};   // rgb | depth | dd | tdv pair tensors
  RawFrames raw;
  const int64_t *actions = nullptr;
  float *out = nullptr;
  bool features_only = false;                // pnvo_forward_features: stop after the hidden layer, `out` receives it
  bool stop_after_compression = false;       // pnvo_forward_compression: stop behind the compression conv and its finalisation
  const GroupedFwd *grp = nullptr;           // a grouped forward's models (pnvo_forward_grouped_raw), or nullptr
  hipStream_t s = nullptr;
};

// helpers implemented in pnvo_api.hip
int pnvo_run_conv(pnvo_handle m, const Layer &l, int B, const ConvRequest &r);   // one conv + the GroupNorm finalisation that follows it
ConvChoice pnvo_conv_choice(pnvo_handle m, const Layer &l, int B, const ConvAsk &ask);
bool pnvo_ds_rides(pnvo_handle m, const Block &b, int B);         // does b's downsample conv ride on its first conv's launch (float32 forwards)?
bool pnvo_conv_takes_tail(pnvo_handle m, const Layer &l, int B);   // does the schedule hand l a BlockTail (l on conv_x3, no tap, option tail)?
void pnvo_pack_conv_weight_cinp(const float *oihw, int cout, int cin, int cinp, int kh, int kw, std::vector<float> &out);
StemPlan pnvo_stem_plan(pnvo_handle m, bool train_fwd, const RawFrames &raw);
int pnvo_run_stem(pnvo_handle m, int B, const StemRequest &r);   // the fused stem + the GroupNorm finalisation that follows it
// the geometry and input side of a 16-bit-matrix-core stem launch (pair tensors or sensor frames), and the launch in the form option
// stem_form selects — shared by the float32 forward and pnvo_bf16.hip
void pnvo_stem_mx_input(pnvo_handle m, int B, const float *const *src, const RawFrames &raw, pnvo::StemMXArgs &a);
double pnvo_stem_in_bytes(pnvo_handle m, int B, const RawFrames &raw);   // algorithmic bytes of the stem's input (timing table)
int pnvo_launch_stem_mx(pnvo_handle m, const pnvo::StemMXArgs &a, int pieces, int ntiles, bool bf16_out, const GroupedFwd *grp, hipStream_t s);
int pnvo_mark_stem(pnvo_handle m, hipStream_t s, const StemPlan &p);
int pnvo_input_fallback(pnvo_handle m, hipStream_t s, bool *rerun);   // after the forward is enqueued: wait for the stem, re-run on the dense stem?
// pnvo_api.hip: the observation pairs of B frame pairs into ws[0..2] (rgb | depth | one-hot with the HOST `edges`, nullptr:
// float32(i / bins)), grown to B pairs when *cap is smaller — what every frame entry falls back on when the frame-reading kernels do
// not serve the handle.  ws = nullptr: the inference entries' workspace m->rawws.
int pnvo_raw_materialise(pnvo_handle m, const uint8_t *rgb_frames, const float *depth_frames, int B, const float *edges, int32_t *err_flag,
                         hipStream_t s, pnvo::DevBuf<float> *ws = nullptr, int *cap = nullptr);
int pnvo_check_frames(pnvo_handle m, const char *entry, const uint8_t *rgb_frames, const float *depth_frames, const float *tdv, int B,
                      const void *out);
void pnvo_train_free(pnvo_handle m);   // pnvo_train_api.hip
const float *pnvo_train_weight_ptr(pnvo_handle m, const Layer &l);   // pnvo_train_api.hip: l's weight in the flat parameter buffer (a conv of m, m->fc, m->head), or nullptr
// pnvo_api.hip: the forward up to the compression conv's raw NHWC output (m->comp_raw, channel-padded to m->comp_cp) and its per-sample
// GroupNorm scale / shift (m->ssC), on the per-layer kernels at every batch size (the persistent small-batch kernel is not entered)
int pnvo_forward_compression(pnvo_handle m, const float *depth, int B, void *stream);
const float *pnvo_train_hidden(pnvo_handle m);   // pnvo_train_api.hip: [B, hidden] output of visual_fc of the last train-mode forward, or nullptr
int pnvo_train_backward_from_hidden(pnvo_handle m, const float *dh, bool stop_after_fc, void *stream);   // the backward entered below the output head
void pnvo_chain_in_bounds(pnvo_handle h, const std::function<float(const Layer &)> &gn_bound);   // pnvo_api.hip
const float *pnvo_train_x2_scale(pnvo_handle m, const Layer &l);     // device {scale, 1/scale} of conv l's float16 pieces, or nullptr
void pnvo_bf16_free(pnvo_handle m);    // pnvo_bf16.hip
bool pnvo_small_usable(pnvo_handle m, int B);   // smallnet.hip: does this call shape take the persistent kernel?
int pnvo_small_forward(pnvo_handle m, int B, const FwdRequest &r, int stem_slots);   // stem_slots: as pnvo_run_stem left them in m->stats
void pnvo_small_free(pnvo_handle m);
int pnvo_forward_bf16(pnvo_handle *hs, int nm, int B, const FwdRequest &r, float *const *outs);   // outs[z]: model z's output (r.out unused)
int pnvo_fail(pnvo_handle h, int code, const std::string &msg);
int pnvo_ensure_workspace(pnvo_handle m, int B);
void pnvo_drop_graphs(pnvo_handle m);   // forget the captured forward graphs (their kernel arguments went stale)

#define HIPCHK(h, expr)                                                                                   \
  do {                                                                                                    \
    hipError_t e__ = (expr);                                                                              \
    if (e__ != hipSuccess)                                                                                \
      return pnvo_fail(h, PNVO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));             \
  } while (0)

// scoped HIP-event timing of one launch (no-op unless pnvo_timing_mode(h, 1))
struct PnvoTimed {
  pnvo_model_s *m;
  hipStream_t s;
  int rec = -1;
  PnvoTimed(pnvo_model_s *m_, hipStream_t s_, const std::string &name, double flops, double bytes);
  ~PnvoTimed();
};
