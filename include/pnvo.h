/*
 * include/pnvo.h — C ABI of the MI355X-native PointNav-VO visual-odometry hot path (libpnvo.so).
 *
 * The reference (Xiaoming-Zhao/PointNav-VO) is 100 % Python and has no FFI; the "plugin API" this path sits
 * behind is the model registry + nn.Module protocol.  Each entry point below names the
 * reference interface it replaces (paths relative to /root/reference); INTEGRATION.md shows the ctypes stub
 * and the registry hook a maintainer would add on the reference side.
 *
 * Conventions: plain C types only (no torch / HIP types in signatures; a stream is passed as void* holding a
 * hipStream_t).  Every function returns 0 (PNVO_OK) or a negative error code and never throws; the message of
 * the last error on a handle is available from pnvo_last_error().  All tensor arguments of the compute entry
 * points are DEVICE pointers owned by the caller, NHWC, float32 unless stated; calls are asynchronous on the
 * given stream and never wait for the whole forward (the one partial wait — for the stem kernel, so that inputs
 * outside the fused stems' contract are handled inside the call — is described at pnvo_check_inputs and can be
 * switched off).  A handle is not thread-safe: one handle per
 * (process, stream), one process per GPU (the reference's own model: launch.py:11-12).
 */
#ifndef PNVO_H_
#define PNVO_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNVO_OK 0
#define PNVO_ERR_ARG (-1)      /* bad argument / unsupported configuration */
#define PNVO_ERR_HIP (-2)      /* a HIP runtime call failed (message has hipGetErrorString) */
#define PNVO_ERR_STATE (-3)    /* call order violated (e.g. forward before load_weights) */
#define PNVO_ERR_WEIGHTS (-4)  /* state_dict table does not match the configured architecture */
#define PNVO_ERR_INPUT (-5)    /* observation data violates the reference's own contract (see pnvo_check_inputs) */

typedef struct pnvo_model_s *pnvo_handle;

/*
 * Architecture of one VO model = the constructor kwargs of the registered reference classes
 * (pointnav_vo/vo/models/vo_cnn.py:183-198, called at pointnav_vo/rl/common/base_trainer_with_vo.py:68-80).
 * n_* are PAIR channel counts: 6 / 2 / 2*discretized_depth_channels / 2, or 0 when the modality is not in
 * observation_space.  ngroups is baseplanes/2 (vo_cnn.py:206); backbone is resnet18 (resnet.py:226-229).
 */
typedef struct {
  int32_t width, height;      /* observation_size = (W, H) */
  int32_t n_rgb, n_depth, n_dd, n_tdv;
  int32_t baseplanes;         /* resnet_baseplanes (32; 64 for the *_wider variants, vo_cnn.py:325) */
  int32_t hidden;             /* hidden_size */
  int32_t out_dim;            /* output_dim (3: dx, dz, dyaw) */
  int32_t normalize;          /* normalize_visual_inputs -> RunningMeanAndVar present */
  int32_t act_embed;          /* 1 for vo_cnn_act_embed variants (vo_cnn_act_embed.py:17-75) */
  int32_t n_acts;             /* embedding rows - 1 (N_ACTS = 4) */
  int32_t flat_size;          /* after_compression_flat_size (2048) */
  int32_t max_batch;          /* workspace sizing hint; the workspace grows on demand */
  int32_t backbone_depth;     /* 0 or 18: resnet18 (BasicBlock); 50 / 101: Bottleneck [3,4,6,3] / [3,4,23,3] (resnet.py:226-241) */
  /* Appended; zero keeps the models above.  Both need backbone_depth 50 or 101 (resnet.py:244-286). */
  int32_t resnext;            /* 1: ResNeXtBottleneck geometry — expansion 2, stage planes 2 * baseplanes * 2^(s-1), and the 3x3 conv of the
                                 FIRST block of each stage grouped with cardinality baseplanes / 2 (resnet.py:198-210 hands the
                                 cardinality to that block only) */
  int32_t se;                 /* 1: every block carries the squeeze-and-excite branch (resnet.py:71-140): se.excite.{0,2}.{weight,bias} */
} pnvo_config;

/* One entry of the reference state_dict: name exactly as model.state_dict() spells it,
 * row-major data at blob[offset .. offset+prod(shape)), reference layout (OIHW convs, [N][K] linears). */
typedef struct {
  const char *name;
  uint64_t offset;            /* in floats */
  int32_t ndim;
  int64_t shape[4];
} pnvo_tensor_desc;

/* Replaces: vo_model_cls(**kwargs).to(device)  (base_trainer_with_vo.py:68-81). */
int pnvo_create(const pnvo_config *cfg, int device, pnvo_handle *out);

/* Replaces: model.load_state_dict(ckpt["model_state"])  (base_trainer_with_vo.py:92-99).
 * blob is HOST memory (copied and re-laid out for the kernels; the caller keeps ownership).  Every tensor the
 * architecture needs must be present with the reference's shape, else PNVO_ERR_WEIGHTS. */
int pnvo_load_weights(pnvo_handle h, const float *blob, size_t n_floats, const pnvo_tensor_desc *toc, int ntoc);

/*
 * Replaces: model.eval(); model(obs_pairs[, actions])  (base_trainer_with_vo.py:286-291;
 * VisualOdometryCNNBase.forward vo_cnn.py:229-233; ResNetEncoder.forward :110-179).
 *   rgb   [B,H,W,n_rgb]   values 0..255        (obs_pairs["rgb"])
 *   depth [B,H,W,n_depth] values 0..1          (obs_pairs["depth"])
 *   dd    [B,H,W,n_dd]    one-hot {0,1}        (obs_pairs["discretized_depth"])
 *   tdv   [B,H,W,n_tdv]   values 0..1          (obs_pairs["top_down_view"])
 *   actions [B] int64 (act_embed variants only, else NULL)
 *   out   [B,out_dim]
 * Pointers of absent modalities must be NULL.  Dropout is identity (eval); "rnd" mode is not provided.
 */
int pnvo_forward(pnvo_handle h, const float *rgb, const float *depth, const float *dd, const float *tdv,
                 const int64_t *actions, int B, float *out, void *stream);

/*
 * Per-handle options: kernel-family selection and behaviour switches.  The reference has no counterpart (torch dispatches its
 * kernels itself); these exist so that tests and benchmarks can A/B the kernel families and so that integrations configure
 * a handle in code, not through the process environment.  The PNVO_<KEY> environment variables of earlier rounds are only
 * the DEFAULTS, read once in pnvo_create; no entry point reads the environment afterwards.
 *   key               values (first = default)             meaning
 *   "stem"            auto | mx | dd | dense                 stem kernel: bf16 matrix cores with exact 3-piece weights | one-hot
 *                                                            table gather | all-fp32 MFMA (takes ANY float input)
 *   "conv"            auto | x3 | fp32 | generic             3x3 / strided convs: 3-piece bf16-pipe kernel for launches of >= 192
 *                                                            workgroups (auto) or always (x3) | fp32-MFMA LDS kernels | generic
 *   "x3_s2"           on | off                               stride-2 convs on the 3-piece kernel
 *   "tail", "pool"    fused | separate                       BasicBlock tails / the max-pool folded into neighbouring kernels
 *   "input_fallback"  on | off                               see pnvo_check_inputs
 *   "small_net"       on | off                               batches of <= small_max pairs (the navigation loop's call shape,
 *   "small_max"       4 (1..4)                               rl/ppo/ppo_trainer.py:836-841): everything behind the stem conv in ONE
 *   "small_coop"      1 | 0                                  persistent launch (smallnet.hip) — default models with BasicBlock
 *                                                            backbones, options conv/tail/pool at their defaults, no tap.
 *                                                            small_coop = 1: hipLaunchCooperativeKernel (all workgroups resident
 *                                                            by the runtime's guarantee); 0: plain launch, 17 us less per call,
 *                                                            for a process that has the GPU to itself (one workgroup per CU, 144
 *                                                            of 256: two such kernels started at the same instant from different
 *                                                            queues could each hold half the chip — the barrier's bounded spin
 *                                                            then leaves NaN poses and fails the handle's next call)
 *   "graph"           0 | 1                                  replay the forward from a captured hipGraph
 *   "wgrad_stem"      mx | fp32        "pool_bwd" fused | separate        "dgrad" phase | masked        (training step)
 *   "wgrad3"          x3 | fp32                              weight gradient of the 3x3 stride-1 convs on the bf16 matrix cores |
 *                                                            on the float32 kernels
 *   "wgrad"           auto | lds9 | generic                  float32 weight-gradient kernels: lds9 takes the nine-wave LDS kernel
 *                                                            where the twelve-wave one would run (only what wgrad3 = fp32 leaves
 *                                                            off the matrix cores), generic skips every LDS-staged kernel, the
 *                                                            float32 stem kernel included
 *   "bf16_fuse"       on | off         "stem_dbg" <int>                                           (experiments)
 * Unknown keys / values return PNVO_ERR_ARG with the accepted spellings in pnvo_last_error.
 */
int pnvo_set_option(pnvo_handle h, const char *key, const char *value);
/* Current value of an option as text ("dense (fallback)" for "stem" once the input fallback engaged). */
int pnvo_get_option(pnvo_handle h, const char *key, char *buf, size_t cap);

/*
 * The same forward from the SENSOR frames (SURVEY.md section 8(b) sketch): replaces the observation construction of
 * BaseRLTrainerWithVO._compute_local_delta_states_from_vo (base_trainer_with_vo.py:172-269) AND the model call (:286-291)
 * without materialising obs_pairs — pair concatenation, the uint8 -> float cast and _discretize_depth_func (:135-167) happen in
 * the stem's operand fetch (7.86 MB per pair of float32 observation tensors are neither written nor read).
 *   rgb_frames   device uint8   [B][2][H][W][3]  (prev frame, cur frame; NULL for models without rgb)
 *   depth_frames device float32 [B][2][H][W]     values 0..1 (feeds the depth and the discretised-depth modality)
 *   tdv          device float32 [B][H][W][2]     the two top-down views (pnvo_topdown_view with out_pstride 2), NULL without it
 *   err_flag     device int32, may be NULL: set to 1 when a depth lies outside [0, 1] (the reference asserts, :136-137)
 * Results are bit-identical to pnvo_build_obs_pairs + pnvo_forward.  Configurations the frame-reading stem does not cover
 * (option stem / pieces away from their defaults, an attached training step, models outside its K-slot layout) are served by
 * materialising the pairs into a workspace of the handle first: same results, the cost of the separate path.
 */
int pnvo_forward_raw(pnvo_handle h, const uint8_t *rgb_frames, const float *depth_frames, const float *tdv, const int64_t *actions,
                     int B, float *out, int32_t *err_flag, void *stream);
/* pnvo_forward_dual (bfloat16, two action models, the second on the swapped pair) from the sensor frames. */
int pnvo_forward_dual_raw(pnvo_handle ha, pnvo_handle hb, const uint8_t *rgb_frames, const float *depth_frames, const float *tdv, int B,
                          float *out_a, float *out_b, int32_t *err_flag, void *stream);

/*
 * GROUPED forward (round 6): the pairs of up to three SEPARATE-ACTION models in one launch chain — what the navigation loop's call
 * needs when BaseRLTrainerWithVO._compute_local_delta_states_from_vo (base_trainer_with_vo.py:277-294: vo_model[act]) is batched over
 * environments: 8-32 pairs per simulator step split over the "forward" / "left" / "right" models are three forwards of ~50 dependent
 * launches each, bound by launch latency.  The pairs are sorted by model: handles[k] serves counts[k] consecutive pairs of the frame
 * tensors (layout of pnvo_forward_raw), sum(counts) == B, n_models <= 3, a count may be 0.  Every kernel of the chain picks a pair's
 * weights, weight scales and GroupNorm affine parameters by its model; the hidden layer and head run per model on its rows.
 * Requirements (else PNVO_ERR_STATE, never a fallback): float32 inference handles of one architecture on one device, default
 * float16-piece kernels, no training step attached, no tap, not an act-embed model.  Per pair float32-grade equal (same
 * tolerances against the fp64 oracle) to the model's own pnvo_forward_raw, whose kernel choice depends on the batch size.
 * One model with a non-zero count: the call is pnvo_forward_raw on that handle.
 */
int pnvo_forward_grouped_raw(const pnvo_handle *handles, const int32_t *counts, int n_models, const uint8_t *rgb_frames,
                             const float *depth_frames, const float *tdv, int B, float *out, int32_t *err_flag, void *stream);
/* PNVO_OK when these (1..3, non-null) handles can share a grouped forward, else the error it would return with the reason in
 * pnvo_last_error(handles[0]): what a caller's dispatch between one grouped and several per-model forwards asks. */
int pnvo_grouped_supported(const pnvo_handle *handles, int n_models);

/*
 * Arithmetic of pnvo_forward for this handle: 0 = float32 (default: exact-float32 products on the matrix cores), 1 = bfloat16
 * (BASELINE config 3: bf16 operands and bf16 activations in HBM, float32 accumulation / GroupNorm statistics / Linear layers).
 * The reference has no such switch (it would be model.bfloat16(), which also rounds the normalisation and the head);
 * resnet18 BasicBlock models with 32 base planes only.  Takes effect at the next forward; no reload needed.
 */
int pnvo_set_precision(pnvo_handle h, int precision);

/*
 * Replaces: the geometric-invariance dual forward of the joint left/right training and evaluation
 *   pred_a = vo_model[act_a](batch_pairs);  pred_b = vo_model[act_b](swapped batch_pairs)
 * (pointnav_vo/vo/engine/vo_cnn_regression_geo_invariance_engine.py:569-602; the swapped (cur, prev) entries are built by
 * pointnav_vo/vo/dataset/regression_geo_invariance_iter_dataset.py:342-386).  Both models run in every launch; model b sees
 * each observation tensor with its [prev | cur] channel halves exchanged WITHOUT the caller materialising the swapped pair
 * (a permutation of b's stem weights), so the observation tensors are read once.  Both handles must have the same
 * architecture and precision 1 (bfloat16).  Tensor contract as pnvo_forward; out_a / out_b [B,out_dim].
 */
int pnvo_forward_dual(pnvo_handle ha, pnvo_handle hb, const float *rgb, const float *depth, const float *dd, const float *tdv,
                      int B, float *out_a, float *out_b, void *stream);

/* Replaces: BaseRLTrainerWithVO._discretize_depth_func (base_trainer_with_vo.py:135-167), batched and strided so
 * that it writes straight into obs_pairs["discretized_depth"]:
 *   for p in [0,n): d = depth[p*in_stride];  onehot[p*out_stride + i] = (e_i <= d < e_{i+1}) for i in [0,bins)
 * (last bin closed; e_i = float32(i/bins), :105-115).  err_flag (device int32, may be NULL) is set to 1 if any
 * value is outside [0,1] (the reference asserts, :136-137). */
int pnvo_discretize_depth(const float *depth, int64_t n, int64_t in_stride, int bins, float *onehot,
                          int64_t out_stride, int32_t *err_flag, void *stream);

/*
 * Replaces: NormalizedDepth2TopDownViewHabitatTorch.gen_top_down_view (pointnav_vo/utils/geometry_utils.py:
 * 516-556), batched over N frames with no host round trip (the reference syncs 4..1066 times per frame and
 * round-trips through cv2 on the host, :529-536,582-606).
 *   frame f, pixel p=(h*W+w): depth[f*in_fstride + p*in_pstride]  ->  out[f*out_fstride + p*out_pstride]
 *   consts[7] (HOST): kinv00, kinv02, min_x, x_den, depth_scale, z_den, min_depth — computed by the caller exactly
 *   as the reference does (torch.inverse(K), _get_x_range; see pointnav-vo_amd/trainer.py).
 *   work: device scratch of pnvo_topdown_workspace_bytes(N,H,W) bytes.
 */
size_t pnvo_topdown_workspace_bytes(int N, int H, int W);
/* Both top-down views of n_pairs (prev, cur) frame pairs in ONE pass of the three kernels (the boundary call's shape:
 * base_trainer_with_vo.py:239-249 builds them one after the other): depth_frames device float32 [n_pairs][2][H][W] ->
 * tdv_pairs [n_pairs][H][W][2] (channel 0 = prev frame).  work >= pnvo_topdown_workspace_bytes(2 * n_pairs, H, W).  Same values as
 * two pnvo_topdown_view calls with out_pstride 2. */
int pnvo_topdown_view_pairs(const float *depth_frames, int n_pairs, int H, int W, const float *consts, int rows_around_center,
                            float *tdv_pairs, void *work, void *stream);
int pnvo_topdown_view(const float *depth, int N, int H, int W, int64_t in_fstride, int64_t in_pstride,
                      const float *consts, int rows_around_center, float *out, int64_t out_fstride,
                      int64_t out_pstride, void *work, void *stream);

/*
 * Replaces: the observation construction of BaseRLTrainerWithVO._compute_local_delta_states_from_vo
 * (base_trainer_with_vo.py:172-269) for n (prev, cur) pairs at once — numpy -> tensor copies, pair concatenation,
 * _discretize_depth_func, the two top-down views — as one pairs kernel + the top-down kernels on the given stream:
 *   rgb_frames   device uint8   [n][2][H][W][3]  (prev frame, cur frame; NULL for models without rgb)
 *   depth_frames device float32 [n][2][H][W]
 *   -> rgb_pairs [n,H,W,6] (0..255 as float), depth_pairs [n,H,W,2], dd_pairs [n,H,W,2*bins] (bins > 0), tdv_pairs [n,H,W,2]
 *      (NULL: skip; tdv_consts as for pnvo_topdown_view, tdv_work >= pnvo_topdown_workspace_bytes(n,H,W))
 *   err_flag (device int32, may be NULL) is set when a depth lies outside [0,1] (the reference asserts, :136-137).
 */
int pnvo_build_obs_pairs(const uint8_t *rgb_frames, const float *depth_frames, int n, int H, int W, int bins,
                         const float *tdv_consts, int rows_around_center, void *tdv_work, float *rgb_pairs, float *depth_pairs,
                         float *dd_pairs, float *tdv_pairs, int32_t *err_flag, void *stream);

/* Frame ring of the batched boundary call.  Consecutive simulator steps of an environment share a frame — this step's prev_obs IS the
 * last step's cur_obs (rl/ppo/ppo_trainer.py:724-841 keeps `prev_obs = observations`) — so the caller uploads one frame per environment
 * and step; the other half of every pair, and its top-down view, come from a per-environment device slot, which then takes the new frame.
 *   up_rgb / up_depth / up_tdv   device: the m uploaded frames [m][H][W][3] uint8 / [m][H][W] float32 / their top-down views [m][H][W]
 *                                 (pnvo_topdown_view on up_depth); up_rgb / up_tdv NULL for models without the modality
 *   ring_rgb / ring_depth / ring_tdv   device: [slots][H][W][3] / [slots][H][W] / [slots][H][W], owned by the caller across calls
 *   idx   device int32 [3][n]: for pair i the index into up_* of its cur frame | of its prev frame, or -1: take the prev frame from
 *         ring slot idx[2][i] | the ring slot that records the cur frame, or -1: none (every slot at most once per call)
 *   -> rgb_frames [n][2][H][W][3], depth_frames [n][2][H][W], tdv_pairs [n][H][W][2]: the inputs of pnvo_forward_raw, bit-identical to
 *      staging both frames of every pair. */
int pnvo_ring_assemble(const uint8_t *up_rgb, const float *up_depth, const float *up_tdv, uint8_t *ring_rgb, float *ring_depth,
                       float *ring_tdv, const int32_t *idx, int n, int H, int W, uint8_t *rgb_frames, float *depth_frames, float *tdv_pairs,
                       void *stream);

/* Host helper of the same boundary: gathers n separately allocated host frames (each bytes_each long) into one (pinned)
 * staging buffer with `threads` copy threads — the per-frame numpy copies were what bounded the batched boundary call. */
int pnvo_stage_frames(const void *const *src, int n, size_t bytes_each, void *dst, int threads);
/* Two frame lists (the rgb frames and the depth frames of a chunk) in one call: one wake-up of the copy workers. */
int pnvo_stage_frames2(const void *const *src_a, size_t bytes_a, void *dst_a, const void *const *src_b, size_t bytes_b, void *dst_b,
                       int n, int threads);

/* ---- VO dataset input pipeline on the device: what StatePairRegressionDataset._process_data
 * does per sample on 20 CPU workers (pointnav_vo/vo/dataset/regression_geo_invariance_iter_dataset.py:205-454), per chunk
 * on the GPU.  Reading the HDF5 file stays with the caller (h5py). ---- */

/* The numpy twin of the top-down view, NormalizedDepth2TopDownViewHabitat.gen_top_down_view (geometry_utils.py:275-470),
 * which the dataset uses (:247-262): same steps as pnvo_topdown_view with the projection in float64.
 *   consts[7] (HOST doubles): inv(K)[0,0], inv(K)[0,2], min_x, x_range*(1+eps), max_depth-min_depth, (max_depth-min_depth)*(1+eps),
 *   min_depth — computed by the caller with numpy as the reference does (pointnav-vo_amd/dataset.py). */
int pnvo_topdown_view_f64(const float *depth, int N, int H, int W, int64_t in_fstride, int64_t in_pstride,
                          const double *consts, int rows_around_center, float *out, int64_t out_fstride,
                          int64_t out_pstride, void *work, void *stream);

/* float16 bit patterns -> float32 (the HDF5 depth arrays, generate_datasets.py:272,290). */
int pnvo_half_to_float(const uint16_t *src, int64_t n, float *dst, void *stream);

/* Batch assembly for M entries from the N samples of a chunk (device pointers):
 *   prev_rgb/cur_rgb [N,H*W*3] uint8, prev_depth/cur_depth [N,H*W] float16 bits, tdv_frames [2,N,H*W] float32 (top-down view of
 *   the prev frames then the cur frames; NULL -> zeros), src[m] = sample of entry m, swap[m] != 0 -> the entry is (cur, prev)
 *   (the geometric-inversion entry, :342-386).  Outputs (each may be NULL): rgb_pairs [M,H,W,6] (0..255), depth_pairs [M,H,W,2],
 *   dd_pairs [M,H,W,2*bins] one-hot with the caller's HOST edges[bins+1] (the dataset compares float16 depth with
 *   float16-rounded edges, regression_iter_dataset.py:32-69; NULL -> float32(i/bins)), tdv_pairs [M,H,W,2].
 *   err_flag is set when a depth is outside [0,1] (the reference asserts, :33-34). */
int pnvo_dataset_pairs(const uint8_t *prev_rgb, const uint8_t *cur_rgb, const uint16_t *prev_depth, const uint16_t *cur_depth,
                       const float *tdv_frames, const int32_t *src, const int32_t *swap, int N, int M, int H, int W, int bins,
                       const float *edges, float *rgb_pairs, float *depth_pairs, float *dd_pairs, float *tdv_pairs,
                       int32_t *err_flag, void *stream);

/* The frame form of pnvo_dataset_pairs: the same M entries as SENSOR frames, the inputs of pnvo_train_forward_raw /
 * pnvo_input_moments_raw — rgb_frames uint8 [M][2][H][W][3] and depth_frames float32 [M][2][H][W] (the float16 depth widened), entry
 * m from sample src[m], a swap[m] != 0 entry as (cur, prev).  1.44 MB per 341x192 pair with the top-down pair tensor against 7.86 MB
 * of pair tensors; the one-hot depth is not stored (the training step derives it from depth_frames with the edges it is given: pass
 * it the edges pnvo_dataset_pairs would have compared with).  Either output may be NULL.  The top-down pair tensor of the same
 * entries comes from pnvo_dataset_pairs with only tdv_pairs non-null.  err_flag is set when a depth is outside [0,1]. */
int pnvo_dataset_frames(const uint8_t *prev_rgb, const uint8_t *cur_rgb, const uint16_t *prev_depth, const uint16_t *cur_depth,
                        const int32_t *src, const int32_t *swap, int N, int M, int H, int W, uint8_t *rgb_frames, float *depth_frames,
                        int32_t *err_flag, void *stream);

/* ---- training step (BASELINE config 4).  One optimisation step of one action model, replacing the body of the
 * reference's training iteration: zero_grad / forward in train mode / loss / backward / optimizer.step()
 * (pointnav_vo/vo/engine/vo_cnn_regression_geo_invariance_engine.py:855-901; loss vo_cnn_engine.py:135-198; Adam
 * :122-133).  Parameters and gradients are caller-owned DEVICE buffers, flat, in the order of `toc` (the reference's
 * state_dict parameter order), so a data-parallel job all-reduces ONE buffer (RCCL).  Dropout must be 0. ---- */

/* Bind the flat parameter / gradient buffers (n_floats each) and build the device-side re-packing maps.
 * toc: parameters only (no RunningMeanAndVar buffers).  Also refreshes the kernel operands from `params`. */
int pnvo_train_attach(pnvo_handle h, float *params, float *grads, size_t n_floats, const pnvo_tensor_desc *toc, int ntoc);

/* Re-pack the kernel operands from the flat parameters (call after every optimiser step; replaces nothing in the
 * reference — torch modules read their parameters in place). */
int pnvo_train_refresh(pnvo_handle h, void *stream);

/* model.train(); out = model(obs_pairs) with every activation kept for the backward pass.  run_mean / run_var: device
 * [C] RunningMeanAndVar buffers AFTER this step's update (running_mean_and_var.py:23-63; the caller performs the
 * update — and its all-reduces — with pnvo_input_moments). */
int pnvo_train_forward(pnvo_handle h, const float *rgb, const float *depth, const float *dd, const float *tdv, int B,
                       const float *run_mean, const float *run_var, float *out, void *stream);

/*
 * pnvo_train_forward from the SENSOR frames (tensor contract of pnvo_forward_raw): rgb_frames uint8 [B][2][H][W][3] (NULL for models
 * without rgb), depth_frames float32 [B][2][H][W], tdv float32 [B][H][W][2] (NULL without it).  No observation-pair tensors are
 * built: the stem reads the frames in its operand fetch, and the training state records that the last forward came from frames (the
 * frame pointers and the edges are kept) — pnvo_train_backward / pnvo_train_backward_from_hidden then run the stem's weight gradient on
 * the same frames, so the caller keeps them alive and unchanged until the backward has run.
 *   edges    HOST float[bins + 1], the bin edges of the one-hot depth (e_i <= d < e_{i+1}, last bin closed); NULL: float32(i / bins),
 *            the navigation boundary's.  A step fed by the dataset passes the float16-rounded edges the dataset compares with.
 *   err_flag device int32, may be NULL: set to 1 when a depth lies outside [0, 1]; never read by the library.
 * Results are bit-identical to pnvo_build_obs_pairs (with these edges) + pnvo_train_forward + pnvo_train_backward.  The call makes no
 * host wait of any kind: sensor frames are inside the stems' input contract by construction, so unlike pnvo_train_forward there is
 * no stem event to wait for.  That holds for handles whose training step runs the 16-bit-matrix-core stem (the default models at
 * option stem auto / mx, wgrad_stem mx, no input fallback engaged).  Every other handle (vo_cnn_wider, options stem=dd / stem=dense,
 * wgrad_stem=fp32) is served by materialising the pairs into a workspace of the training state with the existing kernels and taking
 * the pair path: same results as that path, the cost of the separate path (its wait included).
 */
int pnvo_train_forward_raw(pnvo_handle h, const uint8_t *rgb_frames, const float *depth_frames, const float *tdv, const float *edges,
                           int B, const float *run_mean, const float *run_var, float *out, int32_t *err_flag, void *stream);

/* act_embed variants (vo_cnn_act_embed.py:63-72): the actions [B] (DEVICE int64, values in [0, n_acts]) of the NEXT
 * pnvo_train_forward / pnvo_train_backward pair; the caller keeps the buffer alive until the backward has run. */
int pnvo_train_set_actions(pnvo_handle h, const int64_t *actions);

/* loss.backward() given dLoss/dOut [B,out_dim]: fills the whole gradient buffer (overwrites; no accumulation). */
int pnvo_train_backward(pnvo_handle h, const float *grad_out, void *stream);

/*
 * Gradient-ready hook for data-parallel training (replaces nothing in the reference, whose VO training is single-process;
 * it is what torch DDP's bucketed all-reduce would do for config 4's RCCL gradient exchange).  During pnvo_train_backward the
 * library calls fn(user, first, count, stream) on the host each time the gradients of the flat range [first, first + count)
 * are final — i.e. the launches producing them are enqueued on `stream` — latest layers first: [layer4 .. output head],
 * [layer2 .. layer3], [stem .. layer1] for the reference's parameter order (other orders: one range at the end).  The caller
 * records an event and starts the all-reduce of that range on its communication stream while the rest of the backward runs.
 * pnvo_train_grad_buckets returns the same ranges without running a backward (a rank that must join the collectives of a
 * step in which it had no data).  fn = NULL removes the hook.
 */
typedef void (*pnvo_grad_ready_fn)(void *user, uint64_t first, uint64_t count, void *stream);
int pnvo_train_set_grad_hook(pnvo_handle h, pnvo_grad_ready_fn fn, void *user);
int pnvo_train_grad_buckets(pnvo_handle h, uint64_t *first, uint64_t *count, int cap, int *n_out);

/* Per-channel moments of the assembled network input (reference channel order, rgb/255), the statistics behind
 * RunningMeanAndVar's train-mode update: out[c] = mean_{n,pixel} (x_c - center_c)^power, power in {1,2}; center may be
 * NULL (0).  out: device [C].  power 3: both moments about `center` in ONE pass over the observation tensors —
 * out[c] = mean (x_c - center_c), out[C + c] = mean (x_c - center_c)^2, out: device [2C]. */
int pnvo_input_moments(pnvo_handle h, const float *rgb, const float *depth, const float *dd, const float *tdv, int B,
                       const float *center, int power, float *out, void *stream);
/* The same moments from the sensor frames (tensors, edges and err_flag as pnvo_train_forward_raw; power 1, 2 or 3): one pass over the
 * frames, fp64 partial sums in a fixed order, no atomics.  Every term is the float32 value pnvo_input_moments forms from the pair
 * tensors, so the two agree to the last float32 ulp or two (the fp64 sums run in a different order); handles the frame-reading
 * kernels do not serve (see pnvo_train_forward_raw) run pnvo_input_moments on the materialised pairs. */
int pnvo_input_moments_raw(pnvo_handle h, const uint8_t *rgb_frames, const float *depth_frames, const float *tdv, const float *edges,
                           int B, const float *center, int power, float *out, int32_t *err_flag, void *stream);

/* RunningMeanAndVar.forward, training branch, for ONE process (running_mean_and_var.py:41-60; the multi-process branch
 * :27-38 needs its all-reduces between the steps and stays on the host): m12 = pnvo_input_moments(power 3, center = the
 * current running mean) of a batch of B pairs; mean / var [C] and count [1] are the module's float32 buffers, updated in place
 * (batch mean, variance about it, Chan's merge).  All pointers are device pointers; asynchronous on `stream`. */
int pnvo_rmv_merge(const float *m12, int C, int B, float *mean, float *var, float *count, void *stream);

/* loss = sum_d mean_i (target - pred)^2 (vo_cnn_engine.py:146-194, unit weights) into *loss (device scalar, may be
 * NULL) and dLoss/dPred into grad [B,D] (may be NULL). */
int pnvo_mse_loss(const float *pred, const float *target, int B, int D, float *loss, float *grad, void *stream);

/* The regression loss in its general form: loss = sum_e coef[e] (target[e] - pred[e])^2 over n = B*D elements, grad =
 * dLoss/dPred.  coef carries everything _compute_loss multiplies by (vo_cnn_engine.py:146-194: loss_weights["dx"|"dz"|"dyaw"],
 * dz_regress_masks) and the 1/len(subset) of the per-data-type means the geometric-invariance engine takes
 * (vo_cnn_regression_geo_invariance_engine.py:690-740); the host builds it (pointnav-vo_amd/train.py regression_coef). */
int pnvo_mse_loss_coef(const float *pred, const float *target, const float *coef, int n, float *loss, float *grad,
                       void *stream);

/* _compute_geo_invariance_inverse_loss (vo_cnn_regression_geo_invariance_engine.py:367-449).  deltas [n_entries,3] in the
 * alternating order the reference asserts (cur_rel_to_prev_0, prev_rel_to_cur_0, ...); actions [n_entries] int32 (the even
 * rows are read; rows equal to move_forward drop the dz constraint).  out4 (device, may be NULL) = {weight * loss,
 * abs_diff_rot, abs_diff_pos[0], abs_diff_pos[1]}; grad (may be NULL) = weight * dLoss/dDeltas [n_entries,3]. */
int pnvo_geo_inverse_loss(const float *deltas, const int32_t *actions, int n_entries, int move_forward, float weight,
                          float *out4, float *grad, void *stream);

/* The regression metrics of an evaluation pass (VOCNNRegressionGeometricInvarianceEngine.eval, engine :1020-1257, through
 * _process_one_batch(train_flag=False) :618-751 and _compute_and_update_info :1259-1311 around vo_cnn_engine.py:135-198): ONE
 * launch turns a batch's predictions into the reference's table of per-subset metrics and adds it to running totals.  All
 * pointers are DEVICE memory:
 *   pred, target [M,3] float32, columns (dx, dz, dyaw);  slot [M] int32, the table row an entry belongs to — the caller numbers
 *   the (action model, data type) subsets; -1 and every other value outside [0, n_slots) belong to no row and are never used as
 *   an index;  weights [M,3] float32, _compute_loss_weights' per-entry values, NULL = ones;  dz_mask [M] float32, NULL = ones;
 *   table [n_slots][3][4] FLOAT64 and count [n_slots] int64, both accumulated into.
 * Per slot and d, over the slot's entries S:  loss = mean_S(diff^2 [* mask for dz] * w_d);  abs_diff = mean sqrt(diff^2 [* mask]),
 * for dz over the entries of S with mask == 1 only;  target_magnitude = mean|target| + 1e-8 over those same entries;
 * relative_diff = abs_diff / target_magnitude;  a dz subset without a mask == 1 entry gives abs_diff 0, target_magnitude 1e-8,
 * relative_diff 0 and still the mean over S as its loss.  table[slot][d][0..3] += multiplier * {loss, abs_diff, target_magnitude,
 * relative_diff}, count[slot] += |S|;  multiplier is cur_batch_size in evaluation (update="sum") and 1 for the training logs
 * (update="append").
 * Departure from the reference: a slot WITHOUT entries adds nothing and keeps its count, where the reference takes the mean of an
 * empty tensor and carries NaN into its totals.
 * Float64 arithmetic, no atomics, one fixed summation order (strided per-thread partials, then a fixed tree): the same inputs
 * give the same bits.  One workgroup, any M >= 1.  Asynchronous on `stream`, never waits for the device.  A null required
 * pointer, M <= 0, n_slots <= 0 or n_slots > PNVO_VO_METRICS_MAX_SLOTS return PNVO_ERR_ARG before any launch. */
#define PNVO_VO_METRICS_MAX_SLOTS 16
int pnvo_vo_metrics(const float *pred, const float *target, const int32_t *slot, const float *weights, const float *dz_mask, int M,
                    int n_slots, float multiplier, double *table, int64_t *count, void *stream);

/* nn.Dropout(p) of the two places the reference has one — before visual_fc's Linear and before output_head's Linear
 * (pointnav_vo/vo/models/vo_cnn.py:216-227) — for the train-mode forward/backward.  torch's RNG stream cannot be
 * reproduced; the mask is a counter-based hash of (seed, forward count, layer, element): keep with probability 1-p,
 * kept values scaled by 1/(1-p), the same mask in the backward pass.  p = 0 (default) disables it. */
int pnvo_train_set_dropout(pnvo_handle h, float p, uint64_t seed);

/* The scaled mask (0 or 1/(1-p)) the LAST pnvo_train_forward used: layer 0 -> [B, fh*fw, compression channels padded to a multiple of 32]
 * (the kernel's NHWC order of the flattened feature), layer 1 -> [B, hidden], layer 2 -> [B, 32] (the action-embedding
 * columns of act_embed variants).  For checkers. */
int pnvo_train_dropout_mask(pnvo_handle h, int layer, float *out, void *stream);

/* torch.optim.Adam(weight_decay=0, amsgrad=False) on flat device buffers; step counts from 1.  lr, beta1 and beta2 are taken as the
 * decimals their caller wrote in double (the shortest decimal that rounds to the float given: 0.999f -> 0.999), and every constant
 * of the step - the complements 1 - beta1 and 1 - beta2, lr / (1 - beta1^step), sqrt(1 - beta2^step) - is formed from them in double
 * on the host and rounded to float once, as torch does; exp_avg is torch's lerp_.  The moments of a checkpoint are then those of
 * torch's float32 Adam to float32 rounding, in both directions. */
int pnvo_adam_step(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, size_t n, float lr, float beta1,
                   float beta2, float eps, int step, void *stream);

/* Free everything owned by the handle. */
int pnvo_destroy(pnvo_handle h);

/* ---- the navigation policy's per-step forward: PointNavResNetPolicy.act
 * (pointnav_vo/rl/policies/policy.py:29-46, resnet_policy.py:26-58 and 177-282) for the depth-only configuration of
 * configs/rl/ddppo_pointnav.yaml (resnet18 backbone, 2-layer LSTM, normalize_visual_inputs False, no obs transform); the recurrent
 * core is torch.nn.LSTM or torch.nn.GRU (RL.Policy.rnn_backbone, model_utils/rnns/rnn_state_encoder.py:28). ---- */
#define PNVO_RNN_LSTM 0
#define PNVO_RNN_GRU 1
typedef struct {
  int32_t width, height;      /* frame W, H (341, 192) of every visual type; the encoder sees (W/2, H/2) after avg_pool2d(2) */
  int32_t baseplanes;         /* resnet_baseplanes (32) */
  int32_t hidden;             /* hidden_size (512) */
  int32_t n_actions;          /* action_space.n (4) */
  int32_t rnn_layers;         /* num_recurrent_layers (2) */
  int32_t flat_size;          /* after_compression_flat_size (2048) */
  int32_t rnn_type;           /* PNVO_RNN_LSTM (0: a zeroed field keeps the LSTM) or PNVO_RNN_GRU (1); anything else is refused */
  /* RL.Policy.visual_types / normalize_visual_inputs (resnet_policy.py:82-101; ddppo_trainer.py:118-132).  All three zero: the
   * depth-only, un-normalised policy of the entry points that take `depth` alone. */
  int32_t rgb_channels;       /* 0: no "rgb" among the visual types; 3: observations["rgb"] feeds the encoder in front of the depth */
  int32_t no_depth;           /* 1: "depth" is not among the visual types (needs rgb_channels = 3); 0: it is */
  int32_t normalize;          /* normalize_visual_inputs -> net.visual_encoder.running_mean_and_var */
  /* RL.Policy.backbone (resnet_policy.py:96-101), appended; all three zero: resnet18.  The fields of pnvo_config with the same names:
   * resnet50 / resnet101 = (50 / 101, 0, 0), se_resnet50 = (50, 0, 1), resneXt50 = (50, 1, 0), se_resneXt50 / 101 = (50 / 101, 1, 1).
   * The act, encode and visual_features entry points serve every backbone; the encoder of a non-resnet18 policy has no backward:
   * pnvo_policy_evaluate / _evaluate_rgbd refuse it (evaluate pnvo_policy_encode's output with pnvo_policy_evaluate_features), and
   * pnvo_policy_backward with train_encoder = 1 does too. */
  int32_t backbone_depth, resnext, se;
} pnvo_policy_config;

typedef struct pnvo_policy_s *pnvo_policy_handle;

/* policy_cls(observation_space=..., action_space=..., ...).to(device) — ddppo_trainer.py:115-133. */
int pnvo_policy_create(const pnvo_policy_config *cfg, int device, pnvo_policy_handle *out);

/* actor_critic.load_state_dict(...) — ddppo_trainer.py:140-146; tensor names exactly as PointNavResNetPolicy.state_dict()
 * spells them ("net.visual_encoder.backbone.conv1.0.weight", "net.state_encoder.rnn.weight_ih_l0",
 * "action_distribution.linear.weight", "critic.fc.weight", ...).  blob is HOST memory. */
int pnvo_policy_load_weights(pnvo_policy_handle h, const float *blob, size_t n_floats, const pnvo_tensor_desc *toc,
                             int ntoc);

/* features, rnn_hidden_states = net(observations, rnn_hidden_states, prev_actions, masks); logits / value of the two
 * heads (policy.py:32-36).  All pointers are DEVICE memory:
 *   depth [B,H,W,1] in 0..1 (observations["depth"]);  goal [B,2] = pointgoal_with_gps_compass (rho, phi);
 *   prev_actions [B] int64;  masks [B] (0 at an episode start);  hidden_in / hidden_out [S, B, hidden] with S = 2*rnn_layers for
 *   the LSTM (h of every layer, then c of every layer: rnn_state_encoder.py:47-61) and S = rnn_layers for the GRU (h only);
 *   features [B,hidden], logits [B,n_actions], value [B] may each be NULL.  Sampling / argmax over the logits stays with the
 *   caller (policy.py:38-43).
 *   hidden_in and hidden_out must not overlap (a layer's kernel writes its state while other workgroups still read it):
 *   overlapping ranges are refused with PNVO_ERR_ARG before anything is launched. */
int pnvo_policy_act(pnvo_policy_handle h, const float *depth, const float *goal, const int64_t *prev_actions,
                    const float *masks, const float *hidden_in, int B, float *hidden_out, float *features, float *logits,
                    float *value, void *stream);

/* ---- the visual encoder on its own, and the policy fed with its output (the reference's frozen-encoder training,
 * RL.DDPPO.train_encoder False: ddppo_trainer.py:158-161,257-271 stores net.visual_encoder(batch) in the rollout as
 * observations["visual_features"], and PointNavResNetNet.forward takes that entry instead of running the encoder,
 * resnet_policy.py:249-252). ----
 *
 * pnvo_policy_features_shape: shape = {C, fh, fw} of ResNetEncoder.output_shape for this handle's frame size; F = C * fh * fw.
 * pnvo_policy_encode: depth [B,H,W,1] -> features_out [B,C,fh,fw] (NCHW, device) = relu(GroupNorm(compression conv(backbone(
 *   avg_pool2d(depth, 2))))), on the per-layer kernels at every batch size.
 * pnvo_policy_act_features: pnvo_policy_act with visual_features [B,C,fh,fw] in place of depth: the encoder does not run, visual_fc
 *   reads net.visual_fc.1.weight in torch's [hidden, F] layout (rows in the NCHW flatten's order; F need not be a multiple of 4).  Same
 *   outputs, same refusal of overlapping hidden_in / hidden_out.  The sums of visual_fc run in another order than on the depth path:
 *   float32-grade equal, not bit-equal. */
int pnvo_policy_features_shape(pnvo_policy_handle h, int64_t shape[3]);
int pnvo_policy_encode(pnvo_policy_handle h, const float *depth, int B, float *features_out, void *stream);
int pnvo_policy_act_features(pnvo_policy_handle h, const float *visual_features, const float *goal, const int64_t *prev_actions,
                             const float *masks, const float *hidden_in, int B, float *hidden_out, float *features, float *logits,
                             float *value, void *stream);

/* ---- RGB / RGB-D input and RunningMeanAndVar (ResNetEncoder.forward, resnet_policy.py:146-174: rgb / 255, torch.cat([rgb, depth]),
 * F.avg_pool2d(x, 2), running_mean_and_var; model_utils/running_mean_and_var.py:22-63) for handles created with rgb_channels,
 * no_depth or normalize set.  pnvo_policy_act_rgbd / _encode_rgbd / _evaluate_rgbd are pnvo_policy_act / _encode / _evaluate with
 *   rgb         [B,H,W,3] values 0..255, uint8 (rgb_is_u8 = 1) or float32 (0): the same bits either way; NULL without rgb_channels
 *   depth       [B,H,W,1] float32; NULL with no_depth
 *   run_mean, run_var [C], run_count [1]   the module's own float32 buffers _mean, _var, _count (C = rgb_channels + depth): borrowed,
 *               never owned; NULL without normalize
 *   training    0: the buffers are read (module.eval()); 1: the batch — the B (or T * N) frames of this call — is merged into them first,
 *               in place, on `stream`, with no host synchronisation, and the input is whitened with the UPDATED values
 *               (running_mean_and_var.py:23-63, single process).  Ignored without normalize.
 * One launch (policy_input_kernel) reads the frames once and writes the pooled NHWC tensor in the encoder handle's layout — one float
 * modality of 2C channels [rgb / 255, depth | zeros] — and, when training, per-workgroup partial sums of the first and second moments
 * about the current running mean; a second small launch adds the partials in a fixed order (the same bits on every run) and
 * pnvo_rmv_merge's kernel folds them into the buffers (the moments stay float64 up to there: the first batches are centred on a
 * running mean of zero).  The whitening rides on the encoder's float32 stem as its per-channel scale / shift pair,
 * rewritten on the device from the buffers at every call; the encoder runs on the per-layer kernels at every batch size.
 * On a handle with all three fields zero these calls are the depth-only ones (rgb, the statistics and `training` must be NULL / 0);
 * the depth-only entry points refuse the other handles. */
int pnvo_policy_act_rgbd(pnvo_policy_handle h, const void *rgb, int rgb_is_u8, const float *depth, float *run_mean, float *run_var,
                         float *run_count, int training, const float *goal, const int64_t *prev_actions, const float *masks,
                         const float *hidden_in, int B, float *hidden_out, float *features, float *logits, float *value, void *stream);
int pnvo_policy_encode_rgbd(pnvo_policy_handle h, const void *rgb, int rgb_is_u8, const float *depth, float *run_mean, float *run_var,
                            float *run_count, int training, int B, float *features_out, void *stream);
/* (policy.py:52-63 around the same encoder: the update of rl/ppo/ppo.py:61-139 merges every minibatch it evaluates) */
int pnvo_policy_evaluate_rgbd(pnvo_policy_handle h, const void *rgb, int rgb_is_u8, const float *depth, float *run_mean, float *run_var,
                              float *run_count, int training, const float *goal, const int64_t *prev_actions, const float *masks,
                              const float *hidden_in, int T, int N, const int64_t *actions, int train_encoder, float *hidden_out,
                              float *value, float *logp, float *entropy, void *stream);
/* The input stage on its own (tools/bench_policy.py and tests; not part of the drop-in surface; replaces resnet_policy.py:150-168 and,
 * with moments, running_mean_and_var.py:24-42): pooled_out [B,H/2,W/2,2C]; mode 0: pool only; 1: pool and moments in one pass; 2: pool,
 * then the moments from a second pass over pooled_out (the two-launch form the fused one is measured against).  Modes 1 and 2 write
 * m12_out [2C'] (float64) with C' = rgb_channels + depth: mean (x - center), then mean (x - center)^2, over the B * (H/2) * (W/2) pooled pixels;
 * center [C'] may be NULL (0). */
int pnvo_policy_input_stage(pnvo_policy_handle h, const void *rgb, int rgb_is_u8, const float *depth, const float *center, int mode, int B,
                            float *pooled_out, double *m12_out, void *stream);

int pnvo_policy_destroy(pnvo_policy_handle h);

/* ---- the baseline navigation policy: PointNavBaselinePolicy (pointnav_vo/rl/ppo/policy.py:82-163), the one the reference's plain
 * PPOTrainer builds (rl/ppo/ppo_trainer.py:79-85).  SimpleCNN (model_utils/visual_encoders/simple_cnn.py: Conv 8x8 s4 + ReLU, Conv 4x4 s2
 * + ReLU, Conv 3x3 s1, Flatten (NCHW), Linear + ReLU; bias, no normalisation, no padding) on cat([rgb / 255, depth]); the raw goal
 * vector behind its embedding; one GRU layer (RNNStateEncoder's defaults); the two heads of the policy above.  A handle of its own: all
 * float32 (FMA chains in the convs, fp32 matrix cores in the Linear), every sum in a fixed order, so a sample's bits depend neither on
 * the batch size nor on its position.  A step is seven launches: conv1 (reads the sensor frames: / 255 and the channel concatenation
 * happen in its loader), conv2, conv3, the split-K Linear, partial sums + GRU input row, the GRU layer, the heads.  Its PPO update is
 * the pnvo_baseline_train_* group below. ---- */
typedef struct {
  int32_t width, height;      /* frame W, H of every visual type: both >= 36 (the smallest frame that leaves conv3 one output pixel) */
  int32_t rgb_channels;       /* 0: no "rgb" in the observation space; 3: it is there */
  int32_t depth_channels;     /* 0: no "depth"; 1: it is there.  Both zero: a blind policy, x = goal alone, no encoder */
  int32_t hidden;             /* hidden_size (512): a positive multiple of 8 */
  int32_t n_actions;          /* action_space.n: 1 to 32 */
  int32_t goal_dim;           /* observation_space.spaces[goal_sensor_uuid].shape[0]: 1 to 8 (2) */
} pnvo_baseline_config;

typedef struct pnvo_baseline_s *pnvo_baseline_handle;

int pnvo_baseline_create(const pnvo_baseline_config *cfg, int device, pnvo_baseline_handle *out);

/* Tensor names as PointNavBaselinePolicy.state_dict() spells them: net.visual_encoder.cnn.{0,2,4,6}.{weight,bias} (absent when blind),
 * net.state_encoder.rnn.{weight_ih_l0,weight_hh_l0,bias_ih_l0,bias_hh_l0}, action_distribution.linear.*, critic.fc.*.  blob is HOST
 * memory; a missing or mis-shaped tensor gives PNVO_ERR_WEIGHTS.  The conv weights are re-laid [ky][kx][c][o], the Linear's columns are
 * permuted from the NCHW flatten's order to the NHWC order conv3 writes, weight_ih_l0 is zero-padded to a row pitch that is a multiple
 * of four floats. */
int pnvo_baseline_load_weights(pnvo_baseline_handle h, const float *blob, size_t n_floats, const pnvo_tensor_desc *toc, int ntoc);

/* net.visual_encoder(observations): rgb [B,H,W,3] values 0..255, uint8 (rgb_is_u8 = 1) or float32 (0), the same bits either way, NULL
 * without rgb_channels; depth [B,H,W,1] float32, NULL without depth_channels -> embed [B,hidden].  Device pointers, asynchronous on
 * `stream`.  A blind handle has no encoder: PNVO_ERR_STATE. */
int pnvo_baseline_encode(pnvo_baseline_handle h, const void *rgb, int rgb_is_u8, const float *depth, int B, float *embed, void *stream);

/* One step: x = cat([embed, goal]); x, h = GRU(x, h * mask); logits / value of the two heads.  goal [B,goal_dim] as the sensor gives
 * it; masks [B]; hidden_in / hidden_out [1,B,hidden], which must not overlap (PNVO_ERR_ARG before anything is launched); features
 * [B,hidden], logits [B,n_actions] and value [B] may each be NULL.  prev_actions is no input of this policy. */
int pnvo_baseline_act(pnvo_baseline_handle h, const void *rgb, int rgb_is_u8, const float *depth, const float *goal, const float *masks,
                      const float *hidden_in, int B, float *hidden_out, float *features, float *logits, float *value, void *stream);

int pnvo_baseline_destroy(pnvo_baseline_handle h);

/* ---- one PPO minibatch update of the baseline policy (what the reference's PPOTrainer does with it: rl/ppo/ppo.py:61-139 around
 * Policy.evaluate_actions), the pnvo_policy_* update step's contract on this handle: rollout forward with saved activations, the PPO
 * loss, back-propagation through time and through SimpleCNN into ONE flat gradient buffer.  float32; no torch autograd, no atomics
 * (two runs of the same update give the same bits).  Rows of every [M, ...] tensor are T-major, row t*N + n, M = T*N. ----
 *
 * pnvo_baseline_train_attach: params / grads are DEVICE buffers of n_floats floats (16-byte aligned) holding every tensor of
 * PointNavBaselinePolicy.named_parameters() in torch's own layouts at the offsets of `toc` (multiples of 4 floats).  Requires
 * pnvo_baseline_load_weights before it; that call is refused from then on.  After it the tensors whose layout already is torch's
 * (weight_hh_l0, every bias, the heads) are read from `params` directly — pnvo_baseline_act / _encode included — and the handle's
 * kernel-layout operands ([K][Cout] conv weights, the Linear's weight with its columns in NHWC order, weight_ih_l0 at the padded
 * pitch) are rebuilt from `params` on the device, here and by every pnvo_baseline_train_refresh: an optimiser step on `params`
 * followed by a refresh is all it takes for the next act to use the new weights.  Gradients land in `grads` in torch's layouts (OIHW
 * convs, the Linear's columns in the NCHW flatten's order, weight_ih_l0 [3H, hidden + goal_dim] unpadded).  Every entry is checked
 * before the handle changes. */
int pnvo_baseline_train_attach(pnvo_baseline_handle h, float *params, float *grads, size_t n_floats, const pnvo_tensor_desc *toc,
                               int ntoc);
int pnvo_baseline_train_refresh(pnvo_baseline_handle h, void *stream);

/* value, action_log_probs, entropy, rnn_hidden_states = evaluate_actions(...), everything the backward needs kept in the handle: the
 * frames in the dtype given (rgb [M,H,W,3] uint8 or float32, depth [M,H,W,1]; NULL as the handle's visual types say), masks [M],
 * actions [M] int64 and hidden_in [1,N,hidden] are copied, the caller's tensors may be gone by the backward.  goal [M,goal_dim];
 * hidden_in / hidden_out must not overlap; value [M], logp [M], entropy [1] may each be NULL.  The state is masked at every step.  The
 * embedding, the value and the final state have the bits T successive pnvo_baseline_act calls give.  prev_actions is no input of this
 * policy.  Workspaces grow on demand. */
int pnvo_baseline_evaluate(pnvo_baseline_handle h, const void *rgb, int rgb_is_u8, const float *depth, const float *goal,
                           const float *masks, const float *hidden_in, int T, int N, const int64_t *actions, float *hidden_out,
                           float *value, float *logp, float *entropy, void *stream);

/* As pnvo_policy_ppo_loss, for the last pnvo_baseline_evaluate. */
int pnvo_baseline_ppo_loss(pnvo_baseline_handle h, const float *actions_logp_old, const float *adv, const float *value_preds,
                           const float *returns, float clip, float value_coef, float entropy_coef, int use_clipped_value_loss,
                           float *out3, void *stream);

/* total.backward(): fills the whole gradient buffer (overwrites).  train_encoder = 0 (no net.visual_encoder.* parameter with
 * requires_grad) skips SimpleCNN's backward — the Linear cnn.6 included, it is part of net.visual_encoder — and leaves that range
 * exactly zero; the other gradients have the bits of the full backward.  A blind handle has no encoder tensors at all. */
int pnvo_baseline_backward(pnvo_baseline_handle h, int train_encoder, void *stream);

/* As pnvo_policy_clip_grad_norm. */
int pnvo_baseline_clip_grad_norm(pnvo_baseline_handle h, float max_norm, float *norm_out, void *stream);

/* As pnvo_policy_train_timing / _timing_read: the same five phases (encoder forward, GRU forward + heads, loss, heads + BPTT + d embed,
 * encoder backward). */
int pnvo_baseline_train_timing(pnvo_baseline_handle h, int mode);
int pnvo_baseline_train_timing_read(pnvo_baseline_handle h, double ms[5]);

/* ---- one PPO minibatch update of the navigation policy (rl/ppo/ppo.py:61-139 around Policy.evaluate_actions, policy.py:52-63):
 * rollout forward with saved activations, the PPO loss, back-propagation through time into ONE flat gradient buffer.  float32; no
 * torch autograd anywhere on the path.  Rows of every [M, ...] tensor are T-major, row t*N + n (the order
 * RolloutStorage.recurrent_generator yields), M = T*N. ----
 *
 * pnvo_policy_train_attach: params / grads are DEVICE buffers of n_floats floats holding every tensor of
 * PointNavResNetPolicy.named_parameters() in that order at the offsets of `toc` (offsets multiples of 4 floats, the buffer 16-byte
 * aligned), followed by at least pnvo_policy_train_tail_floats(h) further floats that belong to the library (the stem weight
 * [C0,C,7,7] zero-padded to the encoder handle's 2C input channels, and that handle's unused output head).  After the call the recurrent part
 * and the heads read their weights from `params` — pnvo_policy_act included, so an optimiser step on `params` followed by
 * pnvo_policy_train_refresh is all it takes for the next act to use the new weights — and the visual encoder is attached with
 * pnvo_train_attach.  pnvo_policy_load_weights is refused from then on.  Requires pnvo_policy_load_weights before it. */
size_t pnvo_policy_train_tail_floats(pnvo_policy_handle h);
int pnvo_policy_train_attach(pnvo_policy_handle h, float *params, float *grads, size_t n_floats, const pnvo_tensor_desc *toc,
                             int ntoc);

/* Re-pack the encoder's kernel operands from `params` (after an optimiser step or any other write to it). */
int pnvo_policy_train_refresh(pnvo_policy_handle h, void *stream);

/* Non-resnet18 policies (backbone_depth / resnext / se): the encoder is NOT attached — it keeps the copy of its weights that
 * pnvo_policy_load_weights made, pnvo_policy_train_refresh leaves it alone, and no optimiser step may move it (train_encoder False).
 * After a write to the encoder's range of `params` from outside (a checkpoint loaded on resume) this call re-reads it: a device-to-
 * host copy and pnvo_load_weights on the encoder handle, with the table pnvo_policy_train_attach took; it waits for `stream`.  On a
 * resnet18 policy it is pnvo_policy_train_refresh. */
int pnvo_policy_train_reload_encoder(pnvo_policy_handle h, const pnvo_tensor_desc *toc, int ntoc, void *stream);

/* value, action_log_probs, entropy, rnn_hidden_states = evaluate_actions(...) with everything the backward needs kept in the
 * handle.  depth [M,H,W,1], goal [M,2], prev_actions [M] int64, masks [M], actions [M] int64; hidden_in / hidden_out
 * [S, N, hidden], S = 2*rnn_layers (LSTM) or rnn_layers (GRU), as pnvo_policy_act (must not overlap); value [M], logp [M] =
 * log pi(action), entropy [1] = mean row entropy may each be NULL.
 * The hidden state is masked at every step (equal to the reference's segment-wise masking).  M = N (T = 1) is the reference's
 * single_forward case.  Workspaces grow on demand: a call with a larger M than any before allocates, later ones do not.
 * train_encoder is accepted for symmetry with pnvo_policy_backward; the forward keeps the same activations either way. */
int pnvo_policy_evaluate(pnvo_policy_handle h, const float *depth, const float *goal, const int64_t *prev_actions,
                         const float *masks, const float *hidden_in, int T, int N, const int64_t *actions, int train_encoder,
                         float *hidden_out, float *value, float *logp, float *entropy, void *stream);

/* pnvo_policy_evaluate with visual_features [M,C,fh,fw] (pnvo_policy_features_shape) in place of depth: the encoder does not run.  The
 * feature rows are copied into the handle (the caller's tensor may be gone by the backward).  pnvo_policy_ppo_loss and
 * pnvo_policy_backward then work as after pnvo_policy_evaluate; the backward learns from the handle which kind of evaluate came last,
 * fills net.visual_fc.1.{weight,bias}, the embeddings, the recurrent tensors and the heads, takes no gradient with respect to the
 * features and leaves the encoder's range exactly zero, whatever train_encoder says. */
int pnvo_policy_evaluate_features(pnvo_policy_handle h, const float *visual_features, const float *goal, const int64_t *prev_actions,
                                  const float *masks, const float *hidden_in, int T, int N, const int64_t *actions, float *hidden_out,
                                  float *value, float *logp, float *entropy, void *stream);

/* The minibatch loss of rl/ppo/ppo.py:101-126 for the last pnvo_policy_evaluate: out3 (device) = {value_loss, action_loss,
 * dist_entropy}; the gradient of total = value_loss * value_coef + action_loss - dist_entropy * entropy_coef with respect to the
 * logits and the value stays in the handle for pnvo_policy_backward.  All inputs [M], device.  value_preds may be NULL when
 * use_clipped_value_loss is 0. */
int pnvo_policy_ppo_loss(pnvo_policy_handle h, const float *actions_logp_old, const float *adv, const float *value_preds,
                         const float *returns, float clip, float value_coef, float entropy_coef, int use_clipped_value_loss,
                         float *out3, void *stream);

/* total.backward(): fills the whole gradient buffer (overwrites; no accumulation).  No gradient is taken with respect to the
 * rollout's initial hidden state.  train_encoder = 0 (the reference's _static_encoder: net.visual_encoder frozen) stops after
 * visual_fc — its weight and bias gradients are filled, the encoder's range is left zero. */
int pnvo_policy_backward(pnvo_policy_handle h, int train_encoder, void *stream);

/* nn.utils.clip_grad_norm_(parameters, max_norm) on the gradient buffer, on the device: the global 2-norm (written to norm_out
 * [1], device, may be NULL) and the scaling by max_norm / (norm + 1e-6) when that is below 1.  No host synchronisation. */
int pnvo_policy_clip_grad_norm(pnvo_policy_handle h, float max_norm, float *norm_out, void *stream);

/* The same with the gradient scaled first, in the same two launches: the norm is that of scale * g (each product rounded to float32
 * before it is squared, as a separate g *= scale pass would leave it), and g <- g * (scale * clip) is written once, clip = min(1,
 * max_norm / (norm + 1e-6)).  max_norm <= 0: scale only (norm_out still receives the norm).  scale = 1 gives the bits of
 * pnvo_policy_clip_grad_norm.  Data-parallel training passes scale = 1 / world_size behind the gradient's all-reduce (sum). */
int pnvo_policy_clip_grad_norm_scaled(pnvo_policy_handle h, float scale, float max_norm, float *norm_out, void *stream);

/*
 * Gradient-ready hook of the policy's update step, the contract of pnvo_train_set_grad_hook: during pnvo_policy_backward the library
 * calls fn(user, first, count, stream) on the host each time a range of the flat gradient is final (its producing launches are
 * enqueued on `stream`).  Every float of every parameter that has a gradient in this backward is reported exactly once; a range may
 * span the alignment gaps between neighbouring tensors (always zero) and never reaches the library's tail behind the last parameter.
 * Order: the embeddings, the recurrent tensors and the heads before the encoder's backward is entered; then — through the encoder
 * handle's own hook — the encoder and net.visual_fc without the stem weight; the stem weight last, once it has been un-padded from the
 * tail.  With train_encoder = 0, and after pnvo_policy_evaluate_features, net.visual_fc follows the first group and the encoder's range
 * (exactly zero on every rank) is not reported.  pnvo_policy_grad_buckets returns the ranges of such a backward, in its order, without
 * running one: first / count hold up to cap entries, *n_out receives the number there are.  fn = NULL removes the hook.
 */
int pnvo_policy_set_grad_hook(pnvo_policy_handle h, pnvo_grad_ready_fn fn, void *user);
int pnvo_policy_grad_buckets(pnvo_policy_handle h, int train_encoder, int from_features, uint64_t *first, uint64_t *count, int cap,
                             int *n_out);

/*
 * Cross-process reduction of RunningMeanAndVar's batch statistics inside the input stage (running_mean_and_var.py:24-42 under
 * torch.distributed).  With a hook set, every entry point that merges in training mode (pnvo_policy_act_rgbd, _encode_rgbd,
 * _evaluate_rgbd) leaves in `sums` (a caller-owned device buffer of 2C + 1 doubles, C = the policy's input channels) the un-normalised
 * sums about the current running mean c — sums[ch] = sum (x - c), sums[C + ch] = sum (x - c)^2 over the call's pooled pixels,
 * sums[2C] = its number of frames — calls fn(user, sums, 2C + 1, stream) on the host, which must enqueue on `stream` an in-place
 * sum of the buffer over the ranks, and then takes the batch moments and Chan's merge from the reduced sums and the reduced frame count,
 * both read on the device: one round, no host synchronisation of the library's own.  The running mean is the same on all ranks (the
 * caller broadcasts the buffers once), so the reduced second sums give the variance about the global batch mean.  One rank, or a hook
 * that leaves the buffer alone: the bits of the path without a hook.  fn = NULL removes the hook.
 */
typedef void (*pnvo_stats_reduce_fn)(void *user, double *sums, int n, void *stream);
int pnvo_policy_set_stats_hook(pnvo_policy_handle h, pnvo_stats_reduce_fn fn, void *user, double *sums);

/* Phase timing of the update step with HIP events recorded on the launch stream (tools/bench_ppo_update.py; not part of the drop-in
 * surface).  mode 0 = off, 1 = on.  pnvo_policy_train_timing_read waits for the last pnvo_policy_backward and returns the
 * milliseconds of the last evaluate / ppo_loss / backward: {encoder forward, LSTM or GRU forward + heads, loss, heads + BPTT +
 * embedding backward, encoder backward}. */
int pnvo_policy_train_timing(pnvo_policy_handle h, int mode);
int pnvo_policy_train_timing_read(pnvo_policy_handle h, double ms[5]);

/* ---- RolloutStorage on the device (pointnav_vo/rl/common/rollout_storage.py; pointnav-vo_amd/rollout_storage.py owns the
 * tensors).  Stateless: DEVICE pointers to the storage's contiguous tensors, their sizes and a stream.  T = num_steps, N = num_envs;
 * float32 fields are [T, N] (rewards, action_log_probs) or [T+1, N] (value_preds, returns, masks), actions [T, N] and prev_actions
 * [T+1, N] are int64, recurrent_hidden_states is [T+1, L, N, H] with hidden_row = L*N*H floats per step.  Each call is ONE launch
 * and never waits for the device.  Null pointers, non-positive sizes and a step outside the storage return PNVO_ERR_ARG. ---- */

/* Replaces the seven small copy_ calls of insert() (rollout_storage.py:83-89): the *_in rows ([L,N,H] / [N]) go to row step + 1 of
 * recurrent_hidden_states, prev_actions and masks and to row step of actions, action_log_probs, value_preds and rewards.
 * 0 <= step < T.  The caller advances its step. */
int pnvo_rollout_insert(float *recurrent_hidden_states, int64_t *actions, int64_t *prev_actions, float *action_log_probs,
                        float *value_preds, float *rewards, float *masks, int T, int N, int64_t hidden_row, int step,
                        const float *hidden_in, const int64_t *actions_in, const float *action_log_probs_in,
                        const float *value_preds_in, const float *rewards_in, const float *masks_in, void *stream);

/* Replaces after_update()'s copies of the small fields (rollout_storage.py:97-99): row `step` of recurrent_hidden_states, masks and
 * prev_actions moves to row 0.  0 <= step <= T (0: nothing to do). */
int pnvo_rollout_after_update(float *recurrent_hidden_states, int64_t *prev_actions, float *masks, int T, int N, int64_t hidden_row,
                              int step, void *stream);

/* Replaces compute_returns() (rollout_storage.py:102-120) over the first `step` rows (0 <= step <= T; DD-PPO ends rollouts early):
 *   use_gae != 0: value_preds[step] = next_value; gae = 0; for t = step-1 .. 0:
 *                   delta = (rewards[t] + (gamma * value_preds[t+1]) * masks[t+1]) - value_preds[t]
 *                   gae = delta + (gamma_tau * masks[t+1]) * gae;   returns[t] = gae + value_preds[t]
 *   use_gae == 0: returns[step] = next_value; for t = step-1 .. 0: returns[t] = ((returns[t+1] * gamma) * masks[t+1]) + rewards[t]
 * in float32 with one rounding per operation, the reference's order: bit-equal to its torch result when gamma and gamma_tau are
 * float32(gamma) and float32 of the double product gamma * tau.  next_value [N].  Rows the reference leaves alone are not written.
 * A lane per environment; the [step(+1), N] slabs are staged in LDS with coalesced row loads, and read straight from global memory
 * when a rollout is too long for the LDS budget. */
int pnvo_rollout_compute_returns(const float *rewards, float *value_preds, const float *masks, float *returns, const float *next_value,
                                 int T, int N, int step, int use_gae, float gamma, float gamma_tau, void *stream);

/* Replaces the per-environment slicing, stacking and flattening of recurrent_generator() for ONE minibatch (rollout_storage.py:
 * 143-199): the environments perm[start .. start + n_mb) (perm: int64 [N], every entry in [0, N) — validated by the caller, and an
 * entry outside is skipped, never dereferenced) of the first `steps` rows of the seven [.., N] fields — advantages is [>= steps, N] —
 * are written T-major, row t * n_mb + j, and recurrent_hidden_states[0, :, perm[start + j]] to hidden_out [L, n_mb, H]. */
int pnvo_rollout_gather(const float *recurrent_hidden_states, const int64_t *actions, const int64_t *prev_actions,
                        const float *value_preds, const float *returns, const float *masks, const float *action_log_probs,
                        const float *advantages, const int64_t *perm, int N, int L, int H, int steps, int start, int n_mb,
                        float *hidden_out, int64_t *actions_out, int64_t *prev_actions_out, float *value_preds_out, float *returns_out,
                        float *masks_out, float *action_log_probs_out, float *advantages_out, void *stream);

/* The same gather for one sensor (rollout_storage.py:146-149, 169-171, 186-189): frames [>= steps, N, F] -> out [steps * n_mb, F],
 * frame t * n_mb + j = frames[t, perm[start + j]].  16-byte loads and stores when F % 4 == 0 and both bases are 16-byte aligned,
 * a scalar form otherwise; the grid strides over the work and is bounded by the compute-unit count. */
int pnvo_rollout_gather_frames(const float *frames, const int64_t *perm, int N, int64_t F, int steps, int start, int n_mb, float *out,
                               void *stream);

/* ---- Goal and pose of the navigation loop on the device (pointnav_vo/utils/geometry_utils.py:69-99, 115-144; the loop of
 * rl/ppo/ppo_trainer.py:724-891; pointnav-vo_amd/geometry.py's GoalTracker owns the tensors).  Stateless: DEVICE pointers to the
 * caller's contiguous state tensors over E environments — goal float64 [E,3] (the goal in the agent frame), rot float64 [E,4]
 * ([x,y,z,w]), pos float64 [E,3], polar float32 [E,2] ((rho, -phi): the policy's pointgoal_with_gps_compass) — and a stream.
 * env: DEVICE int32 [n], the state row of each input row, distinct and inside [0, E) (validated by the caller: the calls do not
 * know E); NULL means rows 0..n-1.  State rows that env does not name are not written.  rot and pos may be NULL together: only
 * the goal is tracked.  One thread per row; float64 in the operation order of geometry.py's compute_goal_pos_batch /
 * compute_global_state with one rounding per operation, so everything but sin, cos, hypot and atan2 is bit-equal to those host
 * functions.  Each call is ONE launch (none for n == 0) and never waits for the device.  A null required pointer, n < 0 or
 * exactly one of rot / pos being NULL return PNVO_ERR_ARG. ---- */

/* Row i of deltas (DEVICE float32 (dx, dz, dyaw), rows delta_row_stride floats apart, widened to double first) advances state
 * row env[i]: goal and polar as compute_goal_pos_batch, rot and pos as compute_global_state. */
int pnvo_nav_update(const float *deltas, int64_t delta_row_stride, const int32_t *env, int n, double *goal, double *rot, double *pos,
                    float *polar, void *stream);

/* Episode start (ppo_trainer.py:727-740): goal[env[i]] and polar[env[i]] become compute_goal_pos(goal_world[i], start_delta[i])
 * and rot / pos rows env[i] the start pose.  goal_world, start_delta ((sx, sz, 2 atan2(r_y, r_w)), computed by the caller),
 * start_pos: DEVICE float64 [n,3]; start_rot [n,4]; start_rot / start_pos are read only when the pose is tracked.  The same
 * device function as the update, with a double delta. */
int pnvo_nav_reset(const double *goal_world, const double *start_delta, const double *start_rot, const double *start_pos,
                   const int32_t *env, int n, double *goal, double *rot, double *pos, float *polar, void *stream);

/* ---- Evaluation bookkeeping of the same loop (ppo_trainer.py:742-805, 845-873, 1104-1128; geometry.py's NavEvalStats owns the
 * tensors, NavEvalBook is the host form and the definition).  Per environment: steps int64 [E] (VO steps of the running episode),
 * abs_sum float64 [E,3] (sum of |delta - gt|), std_sum float64 [E,3]; optionally traj float64 [E, max_steps, 16], one record
 * (delta[3], gt[3], std[3], rot[4], pos[3]) per step holding the pose AFTER the step.  Run totals: episodes and steps_total int64
 * [1], l2_sum / std_sum_total / diff_sum float64 [3].  Every sum is sequential — step order within an episode, row order of the
 * call across episodes — so everything but sqrt / atan2 of the yaw diff (and the sin / cos of the pose) is bit-equal to the host
 * form.  One launch each, no atomics, no LDS, no host wait. ---- */

/* pnvo_nav_update with the book's step in front of it: for row i and e = env[i], in this order, abs_sum[e] += |double(delta_i) -
 * gt_i|, std_sum[e] += double(std_i) (zeros when std is NULL), then goal / polar / rot / pos exactly as pnvo_nav_update (the same
 * device functions: the tracker's state is bit for bit what that call writes), steps[e] += 1, and with traj the record of this
 * step at traj[e, steps[e] before the step] (not written once that index reaches max_steps; the caller refuses such a step).
 * gt: DEVICE float64 [n,3]; std: DEVICE float32 [n,3] or NULL, both contiguous.  rot and pos are required. */
int pnvo_nav_update_eval(const float *deltas, int64_t delta_row_stride, const int32_t *env, int n, double *goal, double *rot,
                         double *pos, float *polar, const double *gt, const float *std, int64_t *steps, double *abs_sum,
                         double *std_sum, double *traj, int max_steps, void *stream);

/* Episode end of rows env[i], BEFORE their pnvo_nav_reset: diff[i] = (|sim_x - vo_x|, |sim_z - vo_z|, angle between sim_rot[i] and
 * rot[e]: dq = conj(sim) * vo, 2 atan2(sqrt((dq_x^2 + dq_y^2) + dq_z^2), |dq_w|)) when steps[e] >= 1, zeros otherwise; then, walking
 * the rows in call order with one thread per component, l2_sum += abs_sum[e], std_sum_total += std_sum[e], diff_sum += diff[i],
 * steps_total += steps[e], episodes += 1, and steps / abs_sum / std_sum of e are cleared.  One workgroup: the diff rows are spread
 * over its threads, a barrier separates them from the walk.  sim_pos [n,3], sim_rot [n,4], diff [n,3]: DEVICE float64. */
int pnvo_nav_episode_end(const int32_t *env, int n, const double *sim_pos, const double *sim_rot, const double *rot,
                         const double *pos, int64_t *steps, double *abs_sum, double *std_sum, int64_t *episodes,
                         int64_t *steps_total, double *l2_sum, double *std_sum_total, double *diff_sum, double *diff, void *stream);

/* F.avg_pool2d(x, 2) of 1-channel NHWC frames [N,H,W,1] -> [N,H/2,W/2,2] with channel 1 = 0 (resnet_policy.py:168). */
int pnvo_avgpool2(const float *depth, int N, int H, int W, float *out, void *stream);

/* Message of the last failing call on this handle (or of the last failing handle-less call if h is NULL). */
const char *pnvo_last_error(pnvo_handle h);

/* One-line note of the last SUCCESSFUL call that changed the handle's behaviour (the dense-stem fallback of pnvo_check_inputs,
 * a refused cooperative launch): "" when there is none.  Kept apart from pnvo_last_error, which only ever holds failures. */
const char *pnvo_last_note(pnvo_handle h);

/* ---- introspection used by tests and bench.py (not part of the drop-in surface) ---- */

/* Copy an intermediate activation of the NEXT pnvo_forward into dst (device, capacity in floats).  Names:
 * "input", "stem_conv", "maxpool", "layer{1..4}.{0,1}", "compression", "hidden".  Channel-padded NHWC; the
 * actual shape is returned by pnvo_tap_shape.  Pass name=NULL to clear. */
int pnvo_set_tap(pnvo_handle h, const char *name, float *dst, size_t capacity);
int pnvo_tap_shape(pnvo_handle h, const char *name, int B, int64_t shape[4]);

/* Per-kernel timing with HIP events recorded on the launch stream.  mode 0 = off, 1 = on.
 * pnvo_timing_read synchronises the events, fills up to cap entries and resets the accumulators. */
typedef struct {
  char name[96];
  int64_t launches;
  double total_ms;
  double flops;               /* algorithmic FLOPs of those launches (2*MACs), 0 for non-GEMM kernels */
  double bytes;               /* algorithmic bytes of those launches (tensor reads + writes, once each) */
} pnvo_kernel_time;
/* The same forward stopped after visual_fc's Linear + ReLU: hidden_out [B, hidden] (device).  This is the visual
 * feature the navigation policy consumes (rl/policies/resnet_policy.py:243-250) — see pnvo_policy_* below. */
int pnvo_forward_features(pnvo_handle h, const float *rgb, const float *depth, const float *dd, const float *tdv,
                          const int64_t *actions, int B, float *hidden_out, void *stream);

/* The fused stems exploit the reference's own observation contract: rgb holds integers 0..255 (uint8 frames cast to float,
 * base_trainer_with_vo.py:196-207) and the discretised depth is one-hot per frame (what _discretize_depth_func produces and
 * asserts, :163).  The reference MODEL, however, accepts any float tensor (vo_cnn.py:110-176), so a drop-in must too:
 *   option input_fallback = on (default): pnvo_forward / pnvo_forward_features stay ASYNCHRONOUS — no host wait.  Behind the fused
 *     stem the call enqueues the float32 stem once more, PREDICATED ON THE DEVICE on the flag the fused stem raises when a value
 *     breaks the contract (stem_lds_kernel<.., PAIRED> + pool_keys_from_raw_kernel: both return at once while the flag is down,
 *     ~2 x 3 us of GPU time for contract inputs), so the forward that met such a value repairs itself and delivers the correct
 *     result.  The host reads the (host-mapped) flag at its next entry, without waiting: from then on the handle launches the
 *     float32 stem directly (pnvo_last_note holds a one-line note, pnvo_get_option(h, "stem") reports "dense (fallback)";
 *     pnvo_set_option(h, "stem", ...) lifts it — the one call that waits for the device, to lower the flag safely).  Works inside a
 *     hipGraph capture too (the repair is captured with the forward).  pnvo_train_forward keeps a host-side decision: its
 *     backward must know which stem ran, so it waits (hipEventSynchronize) for its stem kernel — the first of its launches —
 *     and re-runs on the dense stem when the flag is up; the same holds for models the float32 LDS stem does not serve
 *     (stem outputs other than 32 / 64 channels).
 *   option input_fallback = off: no repair launches and no wait; the stem raises the flag and pnvo_check_inputs (definitive after
 *     the caller synchronised the stream) as well as every later forward on the handle return PNVO_ERR_INPUT until the weights
 *     are re-loaded. */
int pnvo_check_inputs(pnvo_handle h);

/* Which kernel family a conv of the residual stages / the compression conv (state_dict prefix, e.g.
 * "visual_encoder.backbone.layer1.0.convs.0") runs on at batch B with the handle's current options — "x2" / "x3" (float32 results
 * from three float16 / six bf16 MFMA terms per product), "fp32-lds", "fp32-generic", "smallnet" (a phase of the persistent
 * small-batch kernel: option small_net, batches <= small_max) — and the matrix-core FLOPs one launch EXECUTES (tile and
 * channel padding and the six-term expansion included): what bench.py prices against the peak of that pipe. */
int pnvo_layer_kernel(pnvo_handle h, const char *name, int B, char *family, size_t cap, double *executed_flops);

/* Host only (no device, no handle): what the conv_x3 planner decides for one problem, as one line in buf —
 *   "<family> <instance key> | grid <x>x<y> block <threads> lds <bytes> | <tile geometry> slots <n> mrows <n>"   tile, persistent
 *   "rows mode<m> | grid <x> block <threads> lds <bytes> | bands <n> rows <n> slots <n>"                          the row-streaming form
 *   "none"                                                                                                        conv_x3.hip leaves the launch
 * problem: n = 23 ints — B, H, W, CIN, Ho, Wo, COUTP (padded channels), kernel size, stride, operand pieces (2 / 3), stager mode
 * (0-3), tail skip with its own scale, gradient input with an absolute-maximum record, riding downsample conv (0 / 1 each), then the
 * plan options force, strip, fine, w8, m16, ksplit, persistent workgroups, rows (options conv=x3, x3_strip ... x3_rows) and the CU count.
 * problem == NULL: the instance key of row n of the table of instantiated kernels, PNVO_ERR_ARG past its last row. */
int pnvo_conv_x3_describe(const int *problem, int n, char *buf, size_t cap);

/* Host only (no device, no handle): what the weight-gradient planner of the training step decides for one problem, as one line —
 *   "<family> <instance> | grid <n> block <threads> lds <bytes> partial <scratch floats> reduce <grid of the reduce launch> | <geometry>"
 * family: generic, lds9, mw12, stem_lds, x3.  problem: n = 16 ints — B, H, W, CIN, Ho, Wo, COUT, DYC (channels per pixel of the output
 * gradient), KH, KW, stride, pad, mode (0 plain input, 1 producer GroupNorm + ReLU recomputed, 2 observation tensors), operand pieces
 * (2: the float16 form is permitted, 3), option wgrad3 (1 x3, 0 fp32), option wgrad (0 auto, 1 lds9, 2 generic).
 * problem == NULL: the instance name of row n of the table of instantiated kernels, PNVO_ERR_ARG past its last row. */
int pnvo_wgrad_describe(const int *problem, int n, char *buf, size_t cap);

/* Host only (no device, no handle): what the planner of the float32-MFMA convs and Linear layers decides for one problem, as one line —
 *   "<family> <instance> | grid <x>x<y>x<z> block <threads> lds <bytes> wsplit <0/1> ksplit <slices> scratch <floats> reduce <none|plain|head> <grid>
 *    | tiles <x>x<y> groups <n> items <n> ldsf <floats> slots <n> wrows <n>"          or "none" (no instantiated kernel serves it)
 * family: generic (mt, nt, mode, jc, feat), lds_tile (blk, wy, wx, nt, mode), lds_wave (blk, nt, mode, mt).  problem: n = 33 ints — B, H, W,
 * CIN, Ho, Wo, COUT, COUTP, KH, KW, stride, pad, up (2: input upsampled by two), channel stride of the output, operand mode (0 plain,
 * 1 producer GroupNorm + ReLU, 2 observation tensors), accumulate (0 / 1), the strided output map y_sh, y_sw, y_oh, y_ow, y_H, y_W (y_sh = 0:
 * dense), then 0 / 1 each: linear epilogue (bias / ReLU), statistics wanted, split-K scratch available; the units of an output head offered
 * to ride on a split-K reduction (0: none); LDS-staged forms allowed (0 / 1); then the plan options fp32_tile (0 auto, 10*MT+NT),
 * fp32_wsplit (-1 auto, 0, 1), fp32_form (0 auto, 1 tile, 2 wave), wave_wgs, wave_nt and the CU count.
 * problem == NULL: the instance key of row n of the table of instantiated kernels, PNVO_ERR_ARG past its last row. */
int pnvo_conv_fp32_describe(const int *problem, int n, char *buf, size_t cap);

int pnvo_timing_mode(pnvo_handle h, int mode);
int pnvo_timing_read(pnvo_handle h, pnvo_kernel_time *entries, int cap, int *n_out);

/* Host-only helper (no GPU needed): pack an OIHW conv weight into the kernel's MFMA operand order.
 * out must hold pnvo_packed_conv_floats(cout, cin, kh, kw) floats. */
size_t pnvo_packed_conv_floats(int cout, int cin, int kh, int kw);
int pnvo_pack_conv_weight(const float *oihw, int cout, int cin, int kh, int kw, float *out);

/* ---- Observation transform (VO.OBS_TRANSFORM / RL.OBS_TRANSFORM): resize the shortest edge with area interpolation and center
 * crop, on the device.  Replaces image_resize_shortest_edge + center_crop (pointnav_vo/utils/misc_utils.py:241-288, :291-318) as
 * ResizeCenterCropper (:81-121) and Resizer (:330-366) call them.  The caller computes the sizes on the host as the reference
 * does (pointnav-vo_amd/obs_transforms.py): the resized grid rs_h x rs_w and the crop window out_h x out_w at (crop_y, crop_x)
 * inside it (crop_y = crop_x = 0 and out = rs for a plain resize).  Only the crop window is computed.
 *   src: n NHWC frames of `channels` (1..4) channels, src_dtype 0 = uint8 (converted to float exactly), 1 = float32; element
 *        strides between frames / rows / pixels (channels are adjacent).
 *   dst: float32; frame f goes to dst + (f / dst_group) * dst_group_stride + (f % dst_group) * dst_member_stride, rows and pixels
 *        at the given element strides — dst_group = 2 with member stride 3 (rgb) or 1 (depth) writes (prev, cur) frame pairs
 *        straight into the channel halves of [n/2,H,W,6] / [n/2,H,W,2] observation pairs.
 *   div_rule: torch's CPU adaptive_avg_pool2d divides by the window in two ways, by the memory format it receives:
 *        0 = contiguous NCHW input, (sum / kh) / kw;  1 = channels-last input, sum / (kh * kw).  Sums run in float32 in torch's
 *        order (input row outer, column inner); results are bit-exact to F.interpolate(mode="area") in that format.
 * No host synchronisation.  Bad sizes, strides or a crop window outside the resized grid return PNVO_ERR_ARG. */
int pnvo_resize_area(const void *src, int src_dtype, int n, int in_h, int in_w, int channels, int64_t src_frame_stride,
                     int64_t src_row_stride, int64_t src_pix_stride, int rs_h, int rs_w, int crop_y, int crop_x, int out_h, int out_w,
                     float *dst, int dst_group, int64_t dst_group_stride, int64_t dst_member_stride, int64_t dst_row_stride,
                     int64_t dst_pix_stride, int div_rule, void *stream);

const char *pnvo_version(void);

/* Bytes this library currently holds in device and host-mapped memory, over all handles of the process (0 before the first
 * pnvo_create and again after the last destroy).  Memory the caller owns (tensors, flat parameter buffers) is not counted. */
long long pnvo_device_bytes_live(void);

#ifdef __cplusplus
}
#endif
#endif /* PNVO_H_ */
