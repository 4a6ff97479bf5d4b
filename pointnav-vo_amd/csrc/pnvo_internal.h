// pnvo_internal.h — declarations shared by the HIP translation units of libpnvo.so (gfx950 only).
#pragma once
#include <mutex>
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pnvo {

constexpr int PNVO_ABSMAX_UINTS = 64 * 16;      // an absolute-maximum record: 64 atomicMax slots, one cache line apart

// A 2-channel slice of one observation tensor feeding the fused stem (MODE 2 of conv_mfma_kernel).
struct SrcPiece {
  const float *base;   // tensor base (nullptr: zero padding piece)
  int nch;             // channels per pixel of that tensor
  int choff;           // first channel of the slice
};

// One convolution / linear layer as an implicit GEMM:  M = B*Ho*Wo output pixels, N = Cout, K = KH*KW*Cin.
struct ConvArgs {
  const float *x;        // [B,H,W,CIN] NHWC, CIN % 8 == 0 (channel-padded)
  const float *wpk;      // packed weights, see pack_conv_weight()
  float *y;              // [M, y_cstride] raw output
  const float *in_scale; // [B,CIN] per-(sample,channel) scale of the fused input transform, or nullptr
  const float *in_shift; // [B,CIN] shift; transform = relu(x*scale+shift) (GroupNorm+ReLU of the producer)
  float *stats;          // [B,slots,COUTP,2] per-(sample,slot,channel) partial (sum, sumsq) or nullptr
  const float *bias;     // [bias_rows,COUT] epilogue bias or nullptr (linear layers)
  const int64_t *bias_row; // [B] row of `bias` per sample (act-embed variants) or nullptr (row 0)
  int B, H, W, CIN;
  int Ho, Wo, COUT, COUTP; // COUTP = COUT rounded up to 32
  int KH, KW, stride, pad;
  int y_cstride;         // channel stride of y (COUT or COUTP)
  int relu_out;          // epilogue ReLU (after bias)
  int slots;             // stats slots per sample
  int lds_floats;        // dynamic LDS available for staging the input transform tables
  int up;                // 2: transposed (backward-data of a stride-2 conv): source = (pos - pad + k) / 2 when even; else 1
  int accum;             // epilogue adds into y instead of overwriting it
  const float *zero_page;            // >= 16 B of zeros (target of masked gathers)
  int y_sh, y_sw, y_oh, y_ow, y_H, y_W;   // y_sh != 0: output pixel (n,i,j) is stored at (n, i*y_sh + y_oh, j*y_sw + y_ow) of a
                                          // [B, y_H, y_W, y_cstride] tensor (one parity phase of a stride-2 backward-data conv)
  int ksplit;            // > 1: blockIdx.z owns a slice of the (tap, channel-group) stages and writes a raw partial
  float *kpart;          // [ksplit][M][y_cstride] partials (bias / ReLU / y are left to ksplit_reduce)
  SrcPiece pieces[8][2][2];          // [j][lane half h][q]: channels 8j+4h+2q, +1 of the stem's K order
};

// The LDS-staged fused stem (stem_lds.hip).
struct StemArgs {
  SrcPiece pieces[8][2][2];   // [j][h][q] -> channels 8j+4h+2q, +1 of the stem's K order (slot g = 2j+h)
  const float *sc, *sh;       // [CPL] whitening x*sc+sh in the stem's channel order (0 for pad channels)
  const float *wpk;           // pack_stem_weight()
  const float *zero_page;     // >= 16 B of zeros (target of masked gathers)
  float *y;                   // [B,Ho,Wo,COUT] raw conv output
  float *stats;               // [B,slots,COUT,2]
  int B, H, W, Ho, Wo, CPL, slots, tiles_x, tiles_y;
  int dbg, lds_pad;           // experiment knobs (PNVO_STEM_DBG="<flags>,<lds_pad_bytes>"): 1 skip staging, 2 skip epilogue
  int paired;                 // 1: stand in for an 8 x 16-tile stem — slots = ceil(Ho/8) * ceil(Wo/16), partials of a tile pair summed
  const int *only_if;         // paired: predicate read on the DEVICE (nullptr: always run) — the launch is a no-op while *only_if == 0
  int *publish;               // paired + only_if: host-mapped copy of the flag, set by this launch when the flag is up
};
int stem_tiles_x(int Wo);
int stem_tiles_y(int Ho);
hipError_t launch_stem_lds(const StemArgs &a, int cout, hipStream_t s);
void pack_stem_weight(const float *oihw_new, int cout, int cinp, int cpl, float *out);

// The one-hot-aware fused stem (stem_dd.hip): dense channels on the matrix cores, one-hot depth bins as a table gather.
struct StemDDArgs {
  SrcPiece pieces[8][2][2];   // [slot][0][q]: dense channels 4*slot + 2q (rgb | depth | tdv | indicator | pad) of 12
  const float *sc, *sh;       // [12] whitening of the dense channels; indicator: sc = 0, sh = 1
  const float *wpk;           // pack_stem_dd_weight of the dense + indicator weights
  const float *table;         // [7 kh][slice]: [7 kw][bins + 1][2 frames][32] one-hot weight rows (row `bins` = 0)
  const float *dd;            // discretised-depth tensor [B,H,W,2*bins]
  const float *zero_page;
  int *bad_onehot;            // device flag: a depth pixel was not one-hot
  float *y, *stats;
  int B, H, W, Ho, Wo, bins, slots, tiles_x, tiles_y, slice_floats;
  int dbg;                    // experiment variants (PNVO_STEM_DBG); 9 = per-phase cycle counters into prof[4]
  unsigned long long *prof;
};
int stem_dd_slice_floats(int bins);
bool stem_dd_supported(int bins);
int stem_dd_slots(int Ho, int Wo);                  // GroupNorm partial-sum slots per sample (tiles)
void pack_stem_dd_weight(const float *w_o12t, int cout, float *out);
hipError_t launch_stem_dd(const StemDDArgs &a, hipStream_t s);
hipError_t launch_stem_dd_repack(const float *w_oihw, int cin, const float *sc_new, const float *sh_new, const int *dense_ref,
                                 const int *dense_new, int nd, const int *dd_ref, const int *dd_new, int bins,
                                 float *table, float *wpk, float *sc12, float *sh12, hipStream_t s);

// The stem on the bf16 matrix cores (stem_mx.hip): float32 results from exact three-piece bf16 weights, or native bf16.
struct StemMXArgs {
  const float *src[4];        // rgb, depth, dd, tdv observation tensors (nullptr if absent)
  const unsigned short *wpk;  // pack_stem_mx_weight(): [49 taps][fragments][N-tiles][64 lanes][8 bf16]
  const float *zero_page;     // >= 128 B of zeros (target of out-of-image reads)
  int *bad_input;             // host-visible flag: a value that must be exact in bf16 was not (PIECES = 3)
  void *y[4];                 // per N-tile (32 output channels): output tensor [B,Ho,Wo,y_cstride] float or bf16
  float *stats[4];            // per N-tile: [B,slots,stats_cstride,2]
  int y_coff[4];              // per N-tile: first channel inside y / stats
  int y_cstride, stats_cstride;
  int B, H, W, Ho, Wo, slots, tiles_x, tiles_y;
  unsigned long long *prof;   // [8 waves][8] phase cycle sums (PNVO_STEM_DBG=9) or nullptr
  // pooled output (float32 results only): [B,Hp,Wp,y_cstride] order-preserving integer keys of max over the 3x3/2 window of
  // sgn(pool_gamma[c]) * x, pre-set to STEM_POOL_INIT; y is not written.  nullptr: the raw output goes to y
  int *pool;
  const float *pool_gamma;    // GroupNorm weight of the stem [cout] (its sign decides max or min)
  int Hp, Wp;
  float oscale;               // PIECES = 2: inverse of the power-of-two scale folded into the packed weights
  const float *oscale_ptr;    //   ... or where it lives on the device (training: the scale follows the weights)
  // RAW staging (pnvo_forward_raw): sensor frames instead of src[0..2]; src[3] stays the top-down view pair tensor
  const unsigned char *raw_rgb;   // [B][2][H][W][3] uint8 or nullptr (model without rgb)
  const float *raw_depth;         // [B][2][H][W] float32; non-null selects the RAW stager
  int raw_flags;                  // bit 0: the model has the depth modality, bit 1: discretised depth
  int *raw_err;                   // device flag: a depth outside [0, 1]
  float edges[12];                // bin edges e_0 .. e_10 of the one-hot depth (float32(i / 10), or RawFrames::edges)
  // developer ablations of stem_rs_kernel (option stem_dbg = 16 + bits; WRONG RESULTS, timing only)
  int dbg;
  // grouped forward (see ConvX3Args): operands of models 1 / 2 (stem_mx_kernel only)
  int grp_end0, grp_end1;
  const unsigned short *wpk_g[2];
  float oscale_g[2];
  const float *pool_gamma_g[2];
};
constexpr int STEM_POOL_INIT = (int)0x807fffffu;   // key of -inf
int stem_mx_slots(int Ho, int Wo);
size_t stem_mx_packed_u16(int pieces, int ntiles);
void pack_stem_mx_weight(const float *wk, int cout, int pieces, const int *xslot, unsigned short *out);
float pack_stem_mx_weight_h(const float *wk, int cout, const int *xslot, unsigned short *out);   // two float16 pieces -> oscale
hipError_t launch_stem_mx(const StemMXArgs &a, int pieces, int ntiles_n, bool bf16_out, hipStream_t s);
bool stem_rs_takes(const StemMXArgs &a, int pieces, int ntiles_n, bool bf16_out, int wgs);   // persistent, weights resident in registers
hipError_t launch_stem_rs(const StemMXArgs &a, int pieces, bool fast, int wgs, hipStream_t s);   // fast: see stem_rs.hip (FAST)                      //   (stem_rs.hip)
hipError_t launch_stem_mx_repack_h(const float *w_oihw, int cin, const float *sc_new, const float *sh_new, const int *slot_ref,
                                   const int *slot_new, const int *xslot, float *scale2, unsigned short *wpk2, hipStream_t s);
hipError_t launch_stem_mx_repack(const float *w_oihw, int cin, const float *sc_new, const float *sh_new, const int *slot_ref,
                                 const int *slot_new, const int *xslot, unsigned short *wpk3, hipStream_t s);

// float32 convs on the bf16 matrix cores by three-piece operand splitting (conv_x3.hip)
struct ConvX3Args {
  const float *x;                    // [B,H,W,CIN] float32 NHWC
  const unsigned short *wpk;         // pack_conv_x3_weight()
  float *y;                          // [B,Ho,Wo,COUTP] raw output
  const float *in_scale, *in_shift;  // [B,CIN] MODE 1: relu(x*scale+shift) applied while staging
  // MODE 2 (fused BasicBlock tail, resnet.py:47-55): the conv's input is relu(x*scale+shift + r), r = res (final activations)
  // or res*res_scale+res_shift (downsample branch); computed while staging and written to xout by the tile that owns the pixel
  const float *res, *res_scale, *res_shift;
  float *xout;
  float *stats;                      // [B,slots,COUTP,2] GroupNorm partial sums or nullptr
  int B, H, W, CIN, Ho, Wo, COUTP;
  int TR, TC, tiles_r, tiles_c, PR, PC, CK, MT, wn, slots;   // the plan's tile geometry (conv_x3_args)
  unsigned long long *prof;          // PNVO_X3_PROF=1: phase cycles of one workgroup (nullptr otherwise)
  // two float16 pieces on a GRADIENT input (backward-data): float bits of max |x| over the input tensor (gn_bwd_apply's absmax); the
  // stager multiplies by 2^(14 - e) before the float16 split, the epilogue divides again (both exact)
  const unsigned *in_absmax;         //   (64 slots of 16 uints: readers take the maximum, absmax_of())
  int rs_bands, rs_rows;             // the rows plan (conv_rows.hip): bands per sample, rows per band
  int rs_dbg;                        // developer ablations (env PNVO_ROWS_DBG; WRONG RESULTS, timing only): 1 no loads, 2 no stores, 4 no MFMAs, 8 no conversion
  const float *oscale_ptr;           // two float16 pieces: where the inverse of the power-of-two scale folded into the packed weights lives on the
  float oscale;                      //   device (training: the scale follows the weights), or (nullptr) the value itself
  // GroupNorm finalisation inside the conv (slots == 1: the workgroup that wrote a sample's only partial sums holds the complete sums
  // of its channels): scale / shift [B,COUTP] as gn_finalize_kernel would write them, bit for bit; nullptr: the separate launch
  const float *gn_gamma, *gn_beta;
  float *gn_scale, *gn_shift;
  float *gn_mu, *gn_rstd;            // [B,groups] mean / reciprocal standard deviation for the backward pass, or nullptr
  int gn_cpg;                        // channels per group (divides 32)
  float gn_eps;
  long gn_P;                         // pixels per sample
  // The block's 1x1 stride-2 downsample conv riding on a 3x3 stride-2 launch (conv_x3_kernel<.., DSF = true>; ds_wpk == nullptr: none):
  // its float16-piece operand (pack_conv_x2_weight of the 1x1 weight), raw output [B,Ho,Wo,COUTP], partial sums (the layout of `stats`,
  // a buffer of its own), weight scale, and its GroupNorm (same groups as the conv's; scale / shift written when the conv's are)
  const unsigned short *ds_wpk;
  float *ds_y, *ds_stats;
  float ds_oscale;
  const float *ds_oscale_ptr;
  const float *ds_gamma, *ds_beta;
  float *ds_scale, *ds_shift;
  float *ds_mu, *ds_rstd;            // [B,groups] for a backward pass, or nullptr
  // GROUPED forward (pnvo_forward_grouped_raw: pairs of up to three action models in one launch chain, sorted by model): sample n
  // belongs to model (n >= grp_end0) + (n >= grp_end1), an end of 0 meaning "no such model" (the structs are zero-filled); models 1 / 2
  // take their operands from [0] / [1]
  int grp_end0, grp_end1;
  const unsigned short *wpk_g[2], *ds_wpk_g[2];
  float oscale_g[2], ds_oscale_g[2];
  const float *gn_gamma_g[2], *gn_beta_g[2], *ds_gamma_g[2], *ds_beta_g[2];
};
#if defined(__HIPCC__)
// One lane = one channel of a sample, lanes of a group adjacent and aligned: GroupNorm scale / shift from the channel's complete
// sums (s1, s2), in gn_finalize_kernel's arithmetic — fp64, the butterfly over the group's lanes in its order (the wider offsets
// of that kernel's 64-lane butterfly add exact zeros), no a*b+c contraction (elementwise.hip is compiled without it).
__device__ __forceinline__ void gn_finalize_lane(float s1, float s2, int cpg, long P, float eps, float gamma, float beta, float *scale, float *shift,
                                                 float *mu_out = nullptr, float *rstd_out = nullptr) {
#pragma clang fp contract(off)
  double d1 = (double)s1, d2 = (double)s2;
  for (int o = cpg >> 1; o >= 1; o >>= 1) {
    d1 += __shfl_xor(d1, o);
    d2 += __shfl_xor(d2, o);
  }
  const double cnt = (double)P * cpg;
  const double mu = d1 / cnt;
  double var = d2 / cnt - mu * mu;
  if (var < 0.0) var = 0.0;
  const double rstd = 1.0 / sqrt(var + (double)eps);
  if (mu_out != nullptr) {                                   // (the group's first lane, as thread 0 of gn_finalize_kernel's block)
    *mu_out = (float)mu;
    *rstd_out = (float)rstd;
  }
  const double sc = rstd * (double)gamma;
  *scale = (float)sc;
  *shift = (float)((double)beta - mu * sc);
}
#endif
// conv_x3 on the host: a PROBLEM (shape, operand pieces, stager mode, the handle's options) -> conv_x3_plan -> a PLAN (kernel family,
// the instance's row in the table of instantiated kernels, launch size, tile geometry) -> conv_x3_args + launch_conv_x3.
struct ConvX3Opts {
  int force;                         // take the layer at any launch size (option conv=x3)
  int strip;                         // wide strip tiles with the N-tiles split over blockIdx.y for 64 / 128 output channels (option x3_strip)
  int fine;                          // allow the fine plan (one N-tile per workgroup) for launches below 224 workgroups (option x3_fine)
  int w8;                            // option x3_w8: eight waves per workgroup (two per SIMD) — 256-channel 6 x 11 maps, one tile per sample
  int m16;                           // option x3_m16: the K loop on 16x16x32 MFMAs, M padded to 16 rows
  int ksw;                           // option x3_ksplit: fine-plan tiles of three / four M-tiles split K over the four waves
  int persist_wgs;                   // > 0: eligible launches take conv_x3p_kernel with this many workgroups (3 per CU); 0: never
  int rows;                          // option x3_rows: 32 -> 32 channel 3x3 stride-1 convs on conv_rows32_kernel where it takes the launch
  int num_cus;
};
struct ConvX3Problem {
  int B, H, W, CIN, Ho, Wo, COUTP, ks, stride;
  int np;                            // operand pieces: 3 = bf16 (six exact product terms), 2 = float16 (three terms)
  int mode;                          // stager: 0 plain, 1 relu(x*scale+shift), 2 block tail with the skip tensor `res`, 3 block tail on pooled keys
  bool tail_scaled;                  // mode 2: the skip branch carries its own scale / shift (a downsample branch)
  bool absmax;                       // a gradient input with its absolute-maximum record (ConvX3Args::in_absmax)
  bool ds;                           // the block's 1x1 stride-2 downsample conv rides on the launch
  ConvX3Opts opt;
};
struct ConvX3Plan {
  enum Family { NONE, TILE, PERSISTENT, ROWS } family = NONE;   // conv_x3_kernel, conv_x3p_kernel, conv_rows32_kernel
  int inst = -1;                     // TILE / PERSISTENT: row of the instance table
  int mode = 0, np = 0;
  int mw = 0, nw = 0;                // the instance's template arguments (16-row / 16-column counts with M16)
  bool dsf = false, w8 = false, ksw = false, m16 = false;
  unsigned grid_x = 0, grid_y = 1;
  int block = 0;
  size_t lds_bytes = 0;
  int TR = 0, TC = 0, tiles_r = 0, tiles_c = 0, PR = 0, PC = 0, CK = 0, MT = 0, wn = 0, slots = 0;
  int rs_bands = 0, rs_rows = 0;     // ROWS: bands per sample, rows per band
  int m_rows = 0;                    // rows of M one tile's MFMAs cover (executed FLOPs): 32 MT, or 16-row sub-tiles x 16 with M16
  explicit operator bool() const { return family != NONE; }
};
ConvX3Plan conv_x3_plan(const ConvX3Problem &q);                                  // pure host code; NONE: outside what the kernels cover
bool conv_rows32_candidate(const ConvX3Problem &q, ConvX3Plan &p);                // the rows form of q, if it takes the launch (conv_rows.hip)
ConvX3Args conv_x3_args(const ConvX3Problem &q, const ConvX3Plan &p);             // shape and the plan's geometry, every operand zero
int conv_x3_describe(const ConvX3Problem *q, int row, char *buf, size_t cap);     // one line for q's plan, or (q == nullptr) for a table row
hipError_t launch_conv_rows32(const ConvX3Args &a, const ConvX3Plan &p, hipStream_t s);
hipError_t launch_conv_x3(const ConvX3Args &a, const ConvX3Plan &p, hipStream_t s);   // TILE / PERSISTENT
hipError_t launch_conv_x3_repack(const float *w_oihw, int cout, int cin, int cinp, int coutp, int kh, int kw, int transposed,
                                 unsigned short *out, hipStream_t s);
void pack_conv_x3_weight(const float *oihw, int cout, int cin, int cinp, int coutp, int kh, int kw, unsigned short *out);
hipError_t launch_conv_x2_scales(const float *params, const long *seg_dev, int nseg, float *out, hipStream_t s);   // [nseg][2]: scale, 1/scale
hipError_t launch_conv_x2_repack(const float *w_oihw, int cout, int cin, int cinp, int coutp, int kh, int kw, const float *scale_dev,
                                 unsigned short *out, hipStream_t s, int transposed = 0);
float pack_conv_x2_weight(const float *oihw, int cout, int cin, int cinp, int coutp, int kh, int kw, unsigned short *out);   // -> oscale

// Native-bf16 convs of the residual stages (conv_bf16.hip); index [z] = model of the launch (dual forward: two).
struct ConvBArgs {
  const unsigned short *x[2];        // [B,H,W,CIN] bf16 NHWC
  const unsigned short *wpk[2];      // pack_conv_bf16_weight()
  void *y[2];                        // [B,Ho,Wo,COUTP] raw output, bf16 (or float for the compression conv)
  const float *in_scale[2], *in_shift[2];   // [B,CIN] MODE 1: relu(x*scale+shift) applied while staging
  // MODE 2 (fused BasicBlock tail, resnet.py:47-55): the conv's input is relu(x*scale+shift + r), r = x2 (final activations)
  // or x2*scale2+shift2 (downsample branch); computed while staging and written to xout by the tile that owns the pixel
  const unsigned short *x2[2];
  const float *in_scale2[2], *in_shift2[2];
  unsigned short *xout[2];
  float *stats[2];                   // [B,slots,COUTP,2] GroupNorm partial sums
  int B, H, W, CIN, Ho, Wo, COUTP;
  int TR, TC, tiles_r, tiles_c, PR, PC, CK, MT, wn, slots;   // filled by conv_bf16_plan
  int persist_wgs;                   // > 0: 32-input-channel layers run persistent with resident weights on this many workgroups
  // the block's 1x1 stride-2 downsample conv riding on a 3x3 stride-2 launch (conv_bf16_kernel DSF; ds_wpk[0] == nullptr: none)
  const unsigned short *ds_wpk[2];
  void *ds_y[2];
  float *ds_stats[2];
  const float *ds_gamma[2], *ds_beta[2];
  float *ds_scale[2], *ds_shift[2];
  // GroupNorm finalisation inside the conv (slots == 1, as ConvX3Args): scale / shift [B,COUTP] per model; nullptr: the separate launch
  const float *gn_gamma[2], *gn_beta[2];
  float *gn_scale[2], *gn_shift[2];
  int gn_cpg;
  float gn_eps;
  long gn_P;
};
bool conv_bf16_plan(ConvBArgs &a, int ks, int stride, int *mw, int *nw, size_t *lds_bytes);
hipError_t launch_conv_bf16(const ConvBArgs &a, int ks, int stride, int mode, bool f32out, int mw, int nw, size_t lds_bytes,
                            int nmodels, hipStream_t s);
void pack_conv_bf16_weight(const float *oihw, int cout, int cin, int cinp, int coutp, int kh, int kw, unsigned short *out);
hipError_t launch_gn_relu_maxpool_bf16(const unsigned short *const *x, const float *const *scale, const float *const *shift,
                                       int B, int H, int W, int C, unsigned short *const *out, int nmodels, hipStream_t s);
hipError_t launch_residual_bf16(const unsigned short *const *a, const float *const *sa, const float *const *ta,
                                const unsigned short *const *b, const float *const *sb, const float *const *tb, int B, long P,
                                int C, unsigned short *const *y, int nmodels, hipStream_t s);

// The float32-MFMA convs on the host, as conv_x3: a PROBLEM (shape, operand mode, epilogue, what the caller can provide, the handle's
// options) -> conv_fp32_plan -> a PLAN (kernel family, the instance's row in the table of instantiated kernels, launch size, splits,
// scratch, statistics slots) -> conv_fp32_args + launch_conv_fp32.  The families:
//   GENERIC   conv_mfma_kernel<MT, NT, MODE, JC, FEAT> (conv_mfma.hip): any conv or Linear layer, A straight from L2
//   LDS_TILE  conv3_lds_kernel<BLK, WY, WX, NT, XF> (conv3_lds.hip): 3x3 stride-1 pad-1 convs, a workgroup stages one patch
//   LDS_WAVE  conv3_wave_kernel<BLK, NT, XF, MT> (conv3_lds.hip): the same convs, every wave stages its own patch
struct ConvFp32Opts {
  int tile;                 // option fp32_tile: 0 auto, 10*MT+NT forces that wave tile from 8192 output pixels on (where NT divides the N-tiles)
  int wsplit;               // option fp32_wsplit: -1 auto, 0 off, 1 on (wherever the split is possible)
  int form;                 // option fp32_form: 0 auto, 1 tile, 2 wave — which LDS-staged kernel
  int wave_wgs;             // option wave_wgs: workgroups per CU of the wave kernel's persistent grid (0: as many as LDS allows)
  int wave_nt;              // option wave_nt: 1 = one N-tile per wave item whatever the layer's N-tile count
  int num_cus;
};
struct ConvFp32Problem {
  int B, H, W, CIN, Ho, Wo, COUT, COUTP, KH, KW, stride, pad, up;
  int y_cstride;            // channel stride of the output (COUT or COUTP)
  int mode;                 // A operand: 0 as stored, 1 relu(x*scale+shift) of the producer's GroupNorm, 2 gathered from the observation tensors
  bool accum;               // the epilogue adds into y
  int y_sh, y_sw, y_oh, y_ow, y_H, y_W;   // y_sh != 0: strided output map (ConvArgs: a parity phase of a stride-2 backward-data conv)
  bool linear;              // a Linear layer's epilogue: bias and / or ReLU
  bool stats;               // GroupNorm partial sums wanted
  bool ksplit_ok;           // the caller can provide split-K scratch (ConvFp32Plan::scratch_floats)
  int head;                 // > 0: the caller offers an output head of this many units to ride on a split-K reduction
  bool lds_ok;              // the caller allows the LDS-staged forms
  ConvFp32Opts opt;
};
struct ConvFp32Plan {
  enum Family { NONE, GENERIC, LDS_TILE, LDS_WAVE } family = NONE;
  int inst = -1;            // row of the instance table
  int MT = 0, NT = 0, MODE = 0, JC = 0, FEAT = 0;   // the instance's template arguments: GENERIC all five; LDS_TILE BLK, WY, WX, NT, MODE;
  int BLK = 0, WY = 0, WX = 0;                      // LDS_WAVE BLK, NT, MODE, MT
  unsigned grid_x = 0, grid_y = 1, grid_z = 1;
  int block = 0;
  size_t lds_bytes = 0;
  int lds_floats = 0;       // GENERIC: LDS floats for the input-transform tables (ConvArgs::lds_floats)
  int wsplit = 0;           // GENERIC: the four waves of a workgroup share one 32-pixel tile and split its reduction (FEAT 1)
  int ksplit = 1;           // GENERIC: > 1: K slices over blockIdx.z, raw partials to scratch, reduced by a second launch
  size_t scratch_floats = 0;
  enum Reduce { NO_REDUCE, PLAIN, HEAD } reduce = NO_REDUCE;   // that launch: ksplit_reduce_kernel, or ksplit_reduce_head_kernel with the head riding
  unsigned reduce_grid = 0;
  int tiles_x = 0, tiles_y = 0, ngroups = 0;   // LDS forms: tiles (wave: pixel blocks) per sample, N-tile groups
  long items = 0;           // work items: workgroups (GENERIC), (tile, N-tile group) items the persistent grid walks (LDS forms)
  int slots = 0;            // statistics slots per sample
  int wave_rows = 0;        // what launch_gn_finalize is given as WM: MT * 32 (GENERIC: slots follow the flattened wave tiles), 0 (LDS: fixed slots)
  explicit operator bool() const { return family != NONE; }
};
struct ConvFp32Head {       // the output head riding on the split-K reduction: plain [out_dim][COUT] weight, bias, out [B][out_dim]
  const float *w, *b;
  int out_dim;
  float *out;
};
ConvFp32Plan conv_fp32_plan(const ConvFp32Problem &q);                            // pure host code; NONE: no instantiated kernel serves q
ConvArgs conv_fp32_args(const ConvFp32Problem &q, const ConvFp32Plan &p);         // geometry and the plan's fields, every operand zero
int conv_fp32_describe(const ConvFp32Problem *q, int row, char *buf, size_t cap); // one line for q's plan, or (q == nullptr) for a table row
// the launch, and behind a split-K launch its reduction y = [relu](sum_z kpart[z] + bias[row]) — with the head on it where the plan says so
hipError_t launch_conv_fp32(const ConvArgs &a, const ConvFp32Plan &p, hipStream_t s, const ConvFp32Head *head = nullptr);
// conv3_lds.hip's instances for the table, and the dynamic LDS of a tile / wave kernel of that shape
template <int BLK, int WY, int WX, int NT, int XF> hipError_t conv3_tile_launch(const ConvArgs &a, const ConvFp32Plan &p, hipStream_t s);
template <int BLK, int NT, int XF, int MT> hipError_t conv3_wave_launch(const ConvArgs &a, const ConvFp32Plan &p, hipStream_t s);
size_t conv3_tile_lds_bytes(int blk, int wy, int wx);
size_t conv3_wave_lds_bytes(int blk, int mt);
// fc_rows.hip: the hidden layer (+ GroupNorm / ReLU of its input) and the output head for <= 32 samples, every action model of a grouped
// forward in one launch each
constexpr int FC_ROWS_MAXV = 12;          // 16-byte vectors of a weight row per lane: Kp <= 3072
struct FcRowsArgs {
  const float *x, *sc, *sh;               // compression conv's raw output [B][Kp] (Kp = fh * fw * cp), its GroupNorm scale / shift [B][cp]
  float *hid, *out;                       // [B][hidden], [B][out_dim]
  const int64_t *actions;                 // act-embed models: the bias row of a sample (nullptr: row 0)
  int B, Kp, cp, hidden, out_dim, ngroups;
  int end[3];                             // one past the last sample of each action model
  const float *w[3], *bias[3], *head_w[3], *head_b[3];   // per model: [hidden][Kp] rows in the activation's (h, w, padded c) order, bias rows, head
};
hipError_t launch_fc_rows(const FcRowsArgs &a, bool with_head, hipStream_t s);
size_t packed_conv_floats(int cout, int cin, int kh, int kw);
void pack_conv_weight(const float *oihw, int cout, int cin, int kh, int kw, float *out);

// GroupNorm statistics -> per-(sample,channel) scale/shift.
// fixed_ns > 0: every sample has exactly fixed_ns slots (stem tiles); else slots follow the flattened wave tiles.
// mu_out / rstd_out (optional, [B,G]) keep the statistics for the backward pass.
struct GnGroup {                     // grouped forward: affine parameters of models 1 / 2 (sample n -> model as in ConvX3Args)
  int end0, end1;
  const float *gamma[2], *beta[2];
};
hipError_t launch_gn_finalize(const float *stats, int B, int slots, int CP, int C, int G, long P, int WM,
                              const float *gamma, const float *beta, float eps, float *scale, float *shift,
                              hipStream_t s, int fixed_ns = 0, float *mu_out = nullptr, float *rstd_out = nullptr,
                              const GnGroup *grp = nullptr);

// Two GroupNorms of one geometry in one launch (fixed slots per sample), each in gn_finalize_kernel's arithmetic; mu / rstd of set 0.
hipError_t launch_gn_finalize_pair(const float *const *stats, int B, int slots, int CP, int C, int G, long P, const float *const *gamma,
                                   const float *const *beta, float eps, float *const *scale, float *const *shift, float *const *mu_out,
                                   float *const *rstd_out, hipStream_t s, const GnGroup *grp0 = nullptr, const GnGroup *grp1 = nullptr);
hipError_t launch_gn_finalize2(const float *const *stats, int B, int slots, int CP, int C, int G, long P, const float *const *gamma,
                               const float *const *beta, float eps, float *const *scale, float *const *shift, int nmodels,
                               hipStream_t s);

// Input assembly + whitening (vo_cnn.py:110-176) into channel-padded NHWC.
struct AssembleArgs {
  const float *src[4];   // rgb, depth, dd, tdv (nullptr if absent)
  int nsrc[4];           // pair channel counts
  const float *mean;     // [C] or nullptr
  const float *stdev;    // [C]
  int C, CP;
  long npix;             // B*H*W
  float *out;            // [npix, CP]
};
hipError_t launch_assemble(const AssembleArgs &a, hipStream_t s);

// relu(gn(x)) then MaxPool 3x3 s2 p1.
hipError_t launch_gn_relu_maxpool(const float *x, const float *scale, const float *shift, int B, int H, int W,
                                  int C, float *out, hipStream_t s);

// *host_flag = 1 if *dev_flag != 0 (one lane): the input-contract flag for the handle's host-side decisions.
hipError_t launch_flag_publish(const int *dev_flag, int *host_flag, hipStream_t s);

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per DEVICE: true exactly once per (device, `seen` mask) — the caller then sets the
// attributes of its kernels for that device.  Serialised by `mu` (two handles on two GPUs may launch from two threads).
inline bool pnvo_first_launch_on_device(std::mutex &mu, unsigned long long &seen) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return true;
  const unsigned long long bit = 1ull << (dev & 63);
  std::lock_guard<std::mutex> lk(mu);
  if (seen & bit) return false;
  seen |= bit;
  return true;
}

// Pooled order-preserving keys (the fused stems' POOL output) from a raw stem output; a no-op while *only_if == 0 (device-side).
hipError_t launch_pool_keys_from_raw(const float *x, const float *gamma, int B, int H, int W, int C, int *keys, const int *only_if,
                                     hipStream_t s);

// The grouped 3x3 conv of the ResNeXt blocks (conv_group.hip): C -> C channels in groups of cg, stride 1 or 2, pad 1.
struct ConvGroupArgs {
  const float *x;                    // [B,H,W,C] NHWC
  const float *wpk;                  // pack_conv_group_weight()
  const float *in_scale, *in_shift;  // [B,C]: relu(x * scale + shift) while the operand is fetched; nullptr: x as it is
  float *y;                          // [B,Ho,Wo,C] raw output
  float *stats;                      // [B,slots,C,2] partial (sum, sumsq) per 32-pixel slot, or nullptr
  int B, H, W, Ho, Wo, C, cg, stride, slots;
};
int conv_group_slots(int P);         // statistics slots per sample
bool conv_group_supported(int C, int cg, int ks, int stride, int pad);
size_t conv_group_packed_floats(int C, int cg);
void pack_conv_group_weight(const float *w, int C, int cg, float *out);   // w: torch's [C][cg][3][3]
hipError_t launch_conv_group(const ConvGroupArgs &a, hipStream_t s);

// The squeeze-and-excite gate of an SE block (se_gate.hip): (scale, shift) [B,C] of the block's last GroupNorm -> (g * scale, g * shift),
// g = sigmoid(W2 . relu(W1 . mean_p(GN(x)) + b1) + b2).
struct SeGateArgs {
  const float *x;                    // [B,P,C] raw output of the block's last conv
  const float *scale, *shift;        // [B,C]
  const float *w1, *b1, *w2, *b2;    // [R,C], [R], [C,R], [C]
  float *out_scale, *out_shift;      // [B,C]
  int B, P, C, R;
};
bool se_gate_supported(int C, int R);
hipError_t launch_se_gate(const SeGateArgs &a, hipStream_t s);

// y = relu(a*sa+ta + r)  with r = b (plain) or b*sb+tb.  a,b,y: [B,P,C].
hipError_t launch_residual(const float *a, const float *sa, const float *ta, const float *b, const float *sb,
                           const float *tb, int B, long P, int C, float *y, hipStream_t s);

// y = relu(x*s+t)  (materialise a normalised activation; used for taps only)
hipError_t launch_apply_ss_relu(const float *x, const float *s, const float *t, int B, long P, int C, float *y,
                                hipStream_t st);

hipError_t launch_discretize_depth(const float *depth, int64_t n, int64_t in_stride, int bins, float *onehot,
                                   int64_t out_stride, int32_t *err_flag, hipStream_t s, const float *edges = nullptr);
hipError_t launch_topdown_f64(const float *depth, int N, int H, int W, int64_t in_fstride, int64_t in_pstride,
                              const double *consts, int rows_around_center, float *out, int64_t out_fstride,
                              int64_t out_pstride, void *work, hipStream_t s);
hipError_t launch_half_to_float(const unsigned short *src, long n, float *dst, hipStream_t s);
hipError_t launch_dataset_pairs(const unsigned char *prev_rgb, const unsigned char *cur_rgb, const unsigned short *prev_depth,
                                const unsigned short *cur_depth, const float *tdv_frames, const int *src, const int *swap,
                                int N, int M, int H, int W, int bins, const float *edges, float *o_rgb, float *o_depth,
                                float *o_dd, float *o_tdv, int *err_flag, hipStream_t s);
hipError_t launch_ring_assemble(const unsigned char *up_rgb, const float *up_dep, const float *up_tdv, unsigned char *ring_rgb,
                                float *ring_dep, float *ring_tdv, const int *idx, int n, int H, int W, unsigned char *pair_rgb,
                                float *pair_dep, float *pair_tdv, hipStream_t s);
hipError_t launch_frame_pairs(const unsigned char *rgb, const float *depth, int n, int H, int W, int bins, float *o_rgb,
                              float *o_depth, float *o_dd, int *err_flag, hipStream_t s, const float *edges = nullptr);
hipError_t launch_dataset_frames(const unsigned char *prev_rgb, const unsigned char *cur_rgb, const unsigned short *prev_depth,
                                 const unsigned short *cur_depth, const int *src, const int *swap, int N, int M, int H, int W,
                                 unsigned char *o_rgb, float *o_depth, int *err_flag, hipStream_t s);
size_t topdown_workspace_bytes(int N, int H, int W);
hipError_t launch_topdown(const float *depth, int N, int H, int W, int64_t in_fstride, int64_t in_pstride,
                          const float *consts_host, int rows_around_center, float *out, int64_t out_fstride,
                          int64_t out_pstride, void *work, hipStream_t s, int64_t out_pair = 0);

// ---- training step (train_kernels.hip) ---------------------------------------------------------------------------
struct SrcLane {            // stem weight gradient: the observation-tensor slot feeding input channel (lane) i
  const float *base;
  int nch, choff;
  float sc, sh;
};

// Weight gradients on the host, as conv_x3: a PROBLEM (shape, input mode, operand pieces the caller permits, the handle's two options)
// -> wgrad_plan -> a PLAN (kernel family, the instance's row in the table of instantiated kernels, both launches' sizes, the geometry
// the kernels read) -> wgrad_args + launch_wgrad.  The families:
//   GENERIC   wgrad_kernel<TG, MODE>: any conv, taps in groups of TG (9 / 7 / 6 / 3 / 1), four units per workgroup
//   LDS9      wgrad3_lds_kernel<MODE, STRIDE>: nine waves, 3x3 pad-1 convs of 32-channel multiples, two persistent workgroups per CU
//   MW12      wgrad3_mw_kernel<MODE, STRIDE>: twelve waves, four units of (ci-tile, co-tile, row group) per workgroup, one per CU
//   STEM_LDS  wgrad_stem_lds_kernel: the 7x7 stride-2 stem from the observation tensors in float32, one workgroup per CU
//   X3        wgrad3_x3_kernel<MODE, NP> (wgrad_x3.hip): 3x3 stride-1 convs on the bf16 matrix cores, operands in NP pieces
struct WgradProblem {
  int B, H, W, CIN, Ho, Wo, COUT, DYC, KH, KW, stride, pad;
  int mode;                 // 0 plain, 1 producer GN+ReLU recomputed, 2 gathered+whitened observation tensors
  int np;                   // 2: the caller permits two float16 pieces per operand (granted to X3 alone); 3: three bf16 pieces
  int wgrad3;               // option wgrad3: 1 X3 allowed, 0 float32 kernels
  int wgrad;                // option wgrad: 0 auto, 1 lds9 (no X3 / MW12 once wgrad3 has excluded X3), 2 generic (no LDS family at all)
};
struct WgradPlan {
  enum Family { GENERIC, LDS9, MW12, STEM_LDS, X3 } family = GENERIC;
  int inst = -1;            // row of the instance table
  unsigned grid = 0, reduce_grid = 0;   // main launch, wgrad_reduce_kernel
  int block = 0;
  size_t lds_bytes = 0, partial_floats = 0;
  int np = 0;               // X3: 2 float16 pieces (three terms, dY scaled from its absolute maximum) or 3 bf16 pieces (six terms)
  int TG = 0, groups = 0, ci_tiles = 0, pairs = 0, chunks = 0;
  long pix_per_chunk = 0;
  int TH = 0, TW = 0, tiles_x = 0, tiles_y = 0, tiles_per_chunk = 0;
  // MW12: units per workgroup = cs ci-tiles x os co-tiles x rs row groups (= 4), workgroups = pair groups x wg_chunks, LDS buffers
  int cs = 0, os = 0, rs = 0, wg_chunks = 0, nbuf = 0;
  int xr_rsegs = 0;         // X3: row segments per strip
};

struct WgradArgs {
  const float *x;           // input activation [B,H,W,CIN] (mode 0/1)
  const float *in_scale, *in_shift;   // [B,CIN] (mode 1: relu(x*scale+shift))
  const float *dy;          // [B,Ho,Wo,DYC] gradient of the conv's raw output
  float *partial;           // [units][TG][32][32]
  const float *zero_page;
  SrcLane src[32];          // mode 2
  int B, H, W, CIN, Ho, Wo, COUT, DYC, KH, KW, stride, pad;
  int mode;
  int TG, groups, ci_tiles, pairs, chunks;      // the plan's geometry (wgrad_args)
  long pix_per_chunk;
  int TH, TW, tiles_x, tiles_y, tiles_per_chunk;
  int cs, os, rs, wg_chunks, nbuf;
  long grad_pitch;          // row pitch of the OIHW gradient tensor (0: cin_out * KH * KW)
  int xr_rsegs;
  const unsigned *dy_absmax;   // X3 with two float16 pieces: dY is scaled by 2^(14 - e) from this record, un-scaled on the accumulators
};
WgradPlan wgrad_plan(const WgradProblem &q);                                     // pure host code
bool wgrad_x3_plan(const WgradProblem &q, WgradPlan &p);                          // the X3 branch (wgrad_x3.hip); false: shape outside it
WgradArgs wgrad_args(const WgradProblem &q, const WgradPlan &p);                  // shape and the plan's geometry, every operand zero
int wgrad_describe(const WgradProblem *q, int row, char *buf, size_t cap);       // one line for q's plan, or (q == nullptr) for a table row
hipError_t launch_wgrad(const WgradArgs &a, const WgradPlan &p, float *grad, const int *ci_perm, int cin_out, hipStream_t s);
inline size_t wgrad_partial_floats(const WgradPlan &p) { return p.partial_floats; }
// the X3 kernel's instances for the table: wgrad_x3_launch<MODE, NP>
template <int MODE, int NP> hipError_t wgrad_x3_launch(const WgradArgs &a, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s);
// Weight gradient of the 7x7 stem on the bf16 matrix cores (wgrad_stem_mx.hip): exact three-piece bf16 on both operands.
struct WgradStemMXArgs {
  const float *src[4];        // rgb, depth, discretised depth, top-down view observation tensors (nullptr if absent)
  const float *dy;            // [B,Ho,Wo,32] gradient of the stem's raw output
  const float *zero_page;     // >= 16 B of zeros (source of the DMA pieces outside the image)
  float *partial;             // [nwg][49][48][32] (set by the launcher)
  int B, H, W, Ho, Wo;
  int tiles_x, tiles_y, tiles_per_wg, nwg;   // filled by wgrad_stem_mx_plan
  unsigned long long *prof;   // PNVO_WSM_PROF: phase cycle counters of one workgroup, or nullptr
};
// The same kernel fed by the SENSOR frames (pnvo_train_forward_raw): src[0..2] stay null, src[3] is the top-down pair tensor.
struct WgradStemMXFrameArgs : WgradStemMXArgs {
  const unsigned char *rgb_frames;   // [B][2][H][W][3] uint8, or nullptr (model without rgb)
  const float *depth_frames;         // [B][2][H][W] float32
  float edges[12];                   // bin edges e_0 .. e_10 of the one-hot depth (+ 1 pad)
  int flags;                         // bit 0: the model has the depth modality, bit 1: the one-hot depth
};
void wgrad_stem_mx_plan(WgradStemMXArgs &a);
hipError_t launch_wgrad_stem_mx_frames(const WgradStemMXFrameArgs &a, float *scratch, const float *sc_new, const float *sh_new,
                                       const int *slot_ref, const int *slot_new, int cin, float *grad, hipStream_t s);
size_t wgrad_stem_mx_scratch_floats(const WgradStemMXArgs &a);
hipError_t launch_wgrad_stem_mx(const WgradStemMXArgs &a, float *scratch, const float *sc_new, const float *sh_new, const int *slot_ref,
                                const int *slot_new, int cin, float *grad, hipStream_t s);

hipError_t launch_gn_bwd(const float *x, const float *dout, const float *scale, const float *shift, const float *mu,
                         const float *rstd, const float *gamma, int B, long P, int C, int Creal, int G, int mask,
                         float *part, float *coef, float *dgamma, float *dbeta, float *dx, hipStream_t s, unsigned *absmax = nullptr);
hipError_t launch_gn_bwd_pool(const float *x, const float *dpool, const unsigned char *idx, int Hs, int Ws, int Hp, int Wp,
                              const float *scale, const float *shift, const float *mu, const float *rstd, const float *gamma, int B, int C,
                              int G, float *part, float *coef, float *dgamma, float *dbeta, float *dx, hipStream_t s);
hipError_t launch_relu_mask(const float *dy, const float *y, const float *add, long n, float *g, hipStream_t s);
hipError_t launch_add(const float *a, const float *b, long n, float *o, hipStream_t s);
hipError_t launch_maxpool_train(const float *x, const float *scale, const float *shift, int B, int H, int W, int C,
                                float *out, unsigned char *idx, hipStream_t s);
hipError_t launch_maxpool_bwd(const float *dpool, const unsigned char *idx, int B, int H, int W, int C, float *dact,
                              hipStream_t s);
hipError_t launch_rmv_merge(const float *m12, int C, int B, float *mean, float *var, float *count, hipStream_t s);
hipError_t launch_rmv_merge(const double *m12, int C, int B, float *mean, float *var, float *count, hipStream_t s);   // float64 moments
// the same merge with the batch's frame count read from the device (a double: the all-reduced count of the data-parallel input stage)
hipError_t launch_rmv_merge_dev(const double *m12, int C, const double *nb, float *mean, float *var, float *count, hipStream_t s);
hipError_t launch_colsum(const float *x, int rows, int cols, int ld, float *out, hipStream_t s);
hipError_t launch_padcopy(const float *src, int rows, int cols, int ldd, float *dst, hipStream_t s);
// y = [relu(x*scale[n,c]+shift[n,c]) or x] * keep/(1-p); keep = hash(seed, step, layer, element) >= p.  x viewed as
// [B][row] with row = P*C elements (C = channel count for the scale index); x == nullptr writes the bare scaled mask.
hipError_t launch_dropout(const float *x, const float *scale, const float *shift, int B, long P, int C, float p,
                          uint64_t seed, uint64_t step, int layer, float *y, hipStream_t s);
hipError_t launch_embed_gather(const float *emb, const long long *actions, int B, int rows, float *out, int *err, hipStream_t s);
hipError_t launch_embed_bias(const float *efeat, const float *w1, long pitch, int flat, const float *b1, int B, int hidden,
                             float *bias, hipStream_t s);
hipError_t launch_embed_backward(const float *gh, const float *efeat, const float *w1, long pitch, int flat, int B, int hidden,
                                 float *dw1, float *dfeat, hipStream_t s);
hipError_t launch_embed_scatter(const float *dfeat, const long long *actions, int B, int rows, float *demb, hipStream_t s);
hipError_t launch_mse_loss(const float *pred, const float *target, int B, int D, float *loss, float *grad, hipStream_t s);
hipError_t launch_mse_loss_coef(const float *pred, const float *target, const float *coef, int n, float *loss, float *grad,
                                hipStream_t s);
hipError_t launch_geo_inverse_loss(const float *deltas, const int *actions, int P, int move_forward, float weight, float *out,
                                   float *grad, hipStream_t s);
hipError_t launch_adam(float *p, const float *g, float *m, float *v, long n, float lr, float b1, float b2, float eps,
                       int step, hipStream_t s);
hipError_t launch_gather(const float *src, const int *map, long n, float *dst, hipStream_t s);
struct GatherSeg {
  const int *map;
  float *dst;
  long start;
};
hipError_t launch_gather_all(const float *src, const GatherSeg *segs, int nseg, long total, hipStream_t s);
hipError_t launch_whiten_table(const float *mean, const float *var, const int *ref_of_new, const int *tensor_of_new, int CPL,
                               float *sc, float *sh, hipStream_t s);
struct MomentsArgs {
  const float *src[4];
  int nch[4];
  int tensor[64], ch[64];   // reference channel c -> (observation tensor, channel inside it)
  const float *center;      // [C] or nullptr
  long npix;
  int pw;                   // 1: mean of (x - center), 2: mean of (x - center)^2, 3: both (out[0..C), out[C..2C))
  int nblk[4];              // filled by launch_moments: blocks of each tensor (proportional to its channel count)
};
// The same moments from the sensor frames (pnvo_input_moments_raw).  Quantity q: 0-5 rgb pair channel | 6-7 depth | 8-27 one-hot | 28-29 tdv.
struct MomentsRawArgs {
  const unsigned char *rgb;  // [B][2][H][W][3] or nullptr
  const float *depth;        // [B][2][H][W]
  const float *tdv;          // [B][H][W][2] or nullptr
  int cof[30];               // reference channel of quantity q, or -1 (the model lacks it)
  const float *center;       // [C] or nullptr
  long npix, fpix;           // B*H*W, H*W
  int pw;
  int *err_flag;             // set when a depth lies outside [0, 1]
  float edges[12];
};
constexpr int MOMENTS_RAW_BLOCKS = 1024;
hipError_t launch_moments_raw(const MomentsRawArgs &a, int C, double *part, float *out, hipStream_t s);
constexpr int MOMENTS_BLOCKS = 2048;   // partial slots per row: `part` holds 2 * C * MOMENTS_BLOCKS doubles
hipError_t launch_moments(const MomentsArgs &a, int C, double *part, float *out, hipStream_t s);

}  // namespace pnvo
