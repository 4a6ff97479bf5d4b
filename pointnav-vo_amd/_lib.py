"""ctypes binding of csrc/libpnvo.so — the C ABI declared in include/pnvo.h.

There is NO fallback: if the HIP library is missing or fails to load, importing this module raises.  The product
path never routes through oracle/ or any CPU implementation.
"""
import ctypes as C
import os

import numpy as np

# torch bundles its own ROCm runtime (torch/lib/libamdhip64.so, same SONAME as /opt/rocm's).  It must be the FIRST HIP
# runtime mapped into the process, so that libpnvo.so's NEEDED libamdhip64.so.7 resolves to the copy torch uses:
# two HIP/HSA runtimes in one process do not both get the GPU ("no ROCm-capable device is detected").
import torch  # noqa: F401,E402

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libpnvo.so")

PNVO_OK = 0


GRAD_READY_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p)
STATS_REDUCE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)        # pnvo_stats_reduce_fn


class PnvoError(RuntimeError):
    pass


class pnvo_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "width", "height", "n_rgb", "n_depth", "n_dd", "n_tdv", "baseplanes", "hidden", "out_dim", "normalize",
        "act_embed", "n_acts", "flat_size", "max_batch", "backbone_depth", "resnext", "se")]


class pnvo_tensor_desc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("offset", C.c_uint64), ("ndim", C.c_int32), ("shape", C.c_int64 * 4)]


class pnvo_kernel_time(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("launches", C.c_int64), ("total_ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double)]


# every symbol include/pnvo.h declares (tests/test_abi.py checks the exported set against the header)
_SIGNATURES = {
    "pnvo_create": (C.c_int, [C.POINTER(pnvo_config), C.c_int, C.POINTER(C.c_void_p)]),
    "pnvo_load_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(pnvo_tensor_desc), C.c_int]),
    "pnvo_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                               C.c_void_p, C.c_void_p]),
    "pnvo_forward_raw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "pnvo_forward_dual_raw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "pnvo_forward_grouped_raw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "pnvo_grouped_supported": (C.c_int, [C.c_void_p, C.c_int]),
    "pnvo_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "pnvo_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p]),
    "pnvo_get_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t]),
    "pnvo_forward_dual": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_build_obs_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_stage_frames": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_int]),
    "pnvo_stage_frames2": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int]),
    "pnvo_discretize_depth": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_void_p]),
    "pnvo_topdown_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "pnvo_topdown_view_f64": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "pnvo_half_to_float": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "pnvo_dataset_pairs": (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 5 + [C.c_void_p] * 7),
    "pnvo_dataset_frames": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_void_p] * 4),
    "pnvo_topdown_view_pairs": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "pnvo_topdown_view": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                    C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                    C.c_void_p]),
    "pnvo_train_attach": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(pnvo_tensor_desc), C.c_int]),
    "pnvo_train_refresh": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pnvo_train_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_train_forward_raw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_input_moments_raw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_void_p,
                                         C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_train_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_train_set_grad_hook": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_train_grad_buckets": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_int)]),
    "pnvo_input_moments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_int, C.c_void_p, C.c_void_p]),
    "pnvo_rmv_merge": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_train_set_actions": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pnvo_mse_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_mse_loss_coef": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_geo_inverse_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "pnvo_vo_metrics": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_train_set_dropout": (C.c_int, [C.c_void_p, C.c_float, C.c_uint64]),
    "pnvo_train_dropout_mask": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "pnvo_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_float,
                                 C.c_float, C.c_float, C.c_int, C.c_void_p]),
    "pnvo_destroy": (C.c_int, [C.c_void_p]),
    "pnvo_ring_assemble": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_last_error": (C.c_char_p, [C.c_void_p]),
    "pnvo_last_note": (C.c_char_p, [C.c_void_p]),
    "pnvo_set_tap": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]),
    "pnvo_tap_shape": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_int64)]),
    "pnvo_check_inputs": (C.c_int, [C.c_void_p]),
    "pnvo_forward_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p]),
    "pnvo_policy_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "pnvo_policy_load_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]),
    "pnvo_policy_act": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_policy_features_shape": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "pnvo_policy_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "pnvo_policy_act_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_policy_evaluate_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_policy_act_rgbd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "pnvo_policy_encode_rgbd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_int, C.c_void_p, C.c_void_p]),
    "pnvo_policy_evaluate_rgbd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_policy_input_stage": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "pnvo_policy_destroy": (C.c_int, [C.c_void_p]),
    "pnvo_baseline_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "pnvo_baseline_load_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]),
    "pnvo_baseline_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "pnvo_baseline_act": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_baseline_destroy": (C.c_int, [C.c_void_p]),
    "pnvo_baseline_train_attach": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(pnvo_tensor_desc), C.c_int]),
    "pnvo_baseline_train_refresh": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pnvo_baseline_evaluate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_baseline_ppo_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float,
                                         C.c_int, C.c_void_p, C.c_void_p]),
    "pnvo_baseline_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "pnvo_baseline_clip_grad_norm": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "pnvo_baseline_train_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "pnvo_baseline_train_timing_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "pnvo_policy_train_tail_floats": (C.c_size_t, [C.c_void_p]),
    "pnvo_policy_train_attach": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(pnvo_tensor_desc), C.c_int]),
    "pnvo_policy_train_refresh": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pnvo_policy_train_reload_encoder": (C.c_int, [C.c_void_p, C.POINTER(pnvo_tensor_desc), C.c_int, C.c_void_p]),
    "pnvo_policy_evaluate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                       C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_policy_ppo_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float,
                                       C.c_int, C.c_void_p, C.c_void_p]),
    "pnvo_policy_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "pnvo_policy_clip_grad_norm": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "pnvo_policy_clip_grad_norm_scaled": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "pnvo_policy_set_grad_hook": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_policy_grad_buckets": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int,
                                           C.POINTER(C.c_int)]),
    "pnvo_policy_set_stats_hook": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pnvo_policy_train_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "pnvo_policy_train_timing_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "pnvo_rollout_insert": (C.c_int, [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_int64, C.c_int] + [C.c_void_p] * 7),
    "pnvo_rollout_after_update": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p]),
    "pnvo_rollout_compute_returns": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_float, C.c_float, C.c_void_p]),
    "pnvo_rollout_gather": (C.c_int, [C.c_void_p] * 9 + [C.c_int] * 6 + [C.c_void_p] * 9),
    "pnvo_rollout_gather_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64] + [C.c_int] * 3 + [C.c_void_p, C.c_void_p]),
    "pnvo_nav_update": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int] + [C.c_void_p] * 5),
    "pnvo_nav_reset": (C.c_int, [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 5),
    "pnvo_nav_update_eval": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int] + [C.c_void_p] * 10 + [C.c_int, C.c_void_p]),
    "pnvo_nav_episode_end": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 14),
    "pnvo_avgpool2": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pnvo_layer_kernel": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_double)]),
    "pnvo_conv_x3_describe": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_char_p, C.c_size_t]),
    "pnvo_wgrad_describe": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_char_p, C.c_size_t]),
    "pnvo_conv_fp32_describe": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_char_p, C.c_size_t]),
    "pnvo_timing_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "pnvo_timing_read": (C.c_int, [C.c_void_p, C.POINTER(pnvo_kernel_time), C.c_int, C.POINTER(C.c_int)]),
    "pnvo_packed_conv_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "pnvo_pack_conv_weight": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pnvo_resize_area": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                                   C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int64,
                                   C.c_int64, C.c_int64, C.c_int, C.c_void_p]),
    "pnvo_version": (C.c_char_p, []),
    "pnvo_device_bytes_live": (C.c_longlong, []),
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise PnvoError(
            f"{LIB_PATH} is missing: the HIP extension has not been built.  Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C pointnav-vo_amd/csrc`).  "
            "There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError here == the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(rc, handle=None):
    if rc != PNVO_OK:
        msg = lib.pnvo_last_error(handle)
        raise PnvoError(f"libpnvo error {rc}: {msg.decode() if msg else '?'}")


def make_toc(entries):
    """[(name, offset in floats, shape)] -> the pnvo_tensor_desc array the load / attach calls take."""
    toc = (pnvo_tensor_desc * len(entries))()
    for i, (name, offset, shape) in enumerate(entries):
        toc[i].name = name.encode()
        toc[i].offset = int(offset)
        toc[i].ndim = len(shape)
        for k, s in enumerate(shape):
            toc[i].shape[k] = int(s)
    return toc


def pack_tensors(named_tensors):
    """[(name, tensor)] -> (host float32 blob of the tensors back to back, its toc)."""
    blob = np.ascontiguousarray(np.concatenate(
        [t.detach().to("cpu", torch.float32).reshape(-1).numpy() for _, t in named_tensors]), dtype=np.float32)
    entries, off = [], 0
    for name, t in named_tensors:
        entries.append((name, off, tuple(t.shape)))
        off += t.numel()
    return blob, make_toc(entries)


def version():
    return lib.pnvo_version().decode()
