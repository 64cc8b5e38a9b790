"""ctypes binding of libcrw_hip.so (C ABI: include/crw_hip.h) for the Python host code.

PyTorch-ROCm is plumbing here: it owns device memory and streams; every product computation of
the random walk goes through the HIP library.  There is NO fallback: if the library is missing or
a tensor is not on an MI355X device the call raises.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CRW_HIP_LIB") or os.path.join(_HERE, "libcrw_hip.so")  # CRW_HIP_LIB: A/B of two builds (tools/)

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "crw_hip.h")


def _header_abi_version():
    """CRW_ABI_VERSION as include/crw_hip.h defines it -- the number is written nowhere else."""
    import re
    m = re.search(r"^#define\s+CRW_ABI_VERSION\s+(\d+)", open(HEADER_PATH).read(), re.M)
    if not m:
        raise RuntimeError(f"no CRW_ABI_VERSION in {HEADER_PATH}")
    return int(m.group(1))


ABI_VERSION = _header_abi_version()
CRW_OK, CRW_EINVAL, CRW_EWORKSPACE, CRW_EHIP = 0, 1, 2, 3
CHAIN_F32, CHAIN_BF16, CHAIN_BF16X3 = 0, 1, 2
_ERR = {1: "CRW_EINVAL (bad shape / null pointer / unsupported size)",
        2: "CRW_EWORKSPACE (workspace too small)", 3: "CRW_EHIP (HIP launch failed)"}

_c_int, _c_f, _c_sz, _p = ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p

# name -> (restype, argtypes); mirrors include/crw_hip.h one to one
SIGNATURES = {
    "crw_abi_version": (_c_int, []),
    "crw_build_arch": (ctypes.c_char_p, []),
    "crw_last_hip_error": (_c_int, []),
    "crw_padded_nodes": (_c_int, [_c_int, _c_int]),
    "crw_walk_state_bytes": (_c_sz, [_c_int, _c_int, _c_int, _c_int]),
    "crw_walk_scratch_bytes": (_c_sz, [_c_int, _c_int, _c_int, _c_int]),
    "crw_affinity_ws_bytes": (_c_sz, [_c_int, _c_int, _c_int]),
    "crw_affinity_fwd": (_c_int, [_p, _c_int, _c_int, _c_int, _c_int, _c_f, _p, _p, _p, _p, _p, _c_sz, _p]),
    "crw_walk_fwd": (_c_int, [_p, _p, _c_int, _c_int, _c_int, _c_int, _p, _c_sz, _p, _p, _p]),
    "crw_walk_bwd": (_c_int, [_p, _p, _c_int, _c_int, _c_int, _c_int, _p, _c_sz, _p, _c_sz, _p, _p]),
    "crw_affinity_bwd": (_c_int, [_p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_f, _p, _p, _p]),
    "crw_normalize": (_c_int, [_p, _c_int, _c_int, _p, _p, _p]),
    "crw_labelprop_topk": (_c_int, [_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_f, _c_int, _c_int, _p, _p, _p]),
    "crw_labelprop_topk_grid": (_c_int, [_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_f, _c_int, _c_int, _c_int, _p, _p, _p]),
    "crw_labelprop_gather": (_c_int, [_p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_int, _p, _p, _p]),
    "crw_pelt_rbf": (_c_int, [_p, _c_int, ctypes.c_double, _c_int, _c_int, ctypes.c_double, _p, _c_int]),
    "crw_labelprop_propagate": (_c_int, [_p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _p, _p, _p]),
    "crw_labelprop_topk_scores": (_c_int, [_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_f, _c_int, _c_int, _c_int, _p, _p, _p]),
    "crw_labelprop_sweep_weights": (_c_int, [_p, _c_int, _c_int, _c_int, _p, _c_int, _p, _p]),
    "crw_labelprop_propagate_batch": (_c_int, [_p, _p, _p, _c_sz] + [_c_int] * 7 + [_p, _p, _p]),
    "crw_labelprop_propagate_sliding": (_c_int, [_p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _p, _p, _p]),
    "crw_labelprop_propagate_sliding_batch": (_c_int, [_p, _p, _p, _c_sz] + [_c_int] * 7 + [_p, _p, _p]),
    "crw_xent_metric": (_c_int, [_p, _c_int, _c_int, _c_int, _p, _p]),
    "crw_confusion_ws_bytes": (_c_sz, [_c_sz, _c_int]),
    "crw_confusion": (_c_int, [_p, _c_int, _p, _c_int, _p, _c_int, _c_sz, _c_int, _c_int, _c_int, _c_int, _p, _p, _p, _c_sz, _p]),
    "crw_horizons_ws_bytes": (_c_sz, [_c_int, _c_int, _c_int]),
    "crw_horizons": (_c_int, [_p, _c_int, _p, _c_int, _p, _c_int, _c_int, _c_int, _c_sz] + [_c_int] * 7 + [_p, _p, _p, _p, _c_sz, _p]),
    "crw_labelprop_confidence": (_c_int, [_p, _c_int, _c_int, _c_int, _c_int, _c_int, _p, _p]),
    "crw_merge_confidence": (_c_int, [_p, _p, _p, _p, _c_int, _c_sz, _p, _p, _p, _p]),
    "crw_calibration_ws_bytes": (_c_sz, [_c_sz, _c_int, _c_int]),
    "crw_calibration": (_c_int, [_p, _c_int, _p, _c_int, _p, _p, _c_int, _c_sz, _c_int, _c_int, _c_int, _c_int, _c_int, _p, _p, _p, _p,
                                 _c_sz, _p]),
    "crw_labelmap_dense": (_c_int, [_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _p, _c_int, _p, _c_sz, _p]),
    "crw_labelmap_dense_batch": (_c_int, [_p] + [_c_int] * 8 + [_p, _c_int, _p, _c_sz, _c_sz, _p]),
    "crw_labelmap_ordered_workspace": (_c_sz, [_c_int, _c_int, _c_int]),
    "crw_labelmap_ordered": (_c_int, [_p] + [_c_int] * 6 + [_p, _c_int, _c_int, _p, _c_int, _p, _c_sz, _p, _c_sz, _p]),
    "crw_labelmap_ordered_batch": (_c_int, [_p] + [_c_int] * 7 + [_p, _c_int, _c_int, _p, _c_int, _p, _c_sz, _c_sz, _p, _c_sz, _p]),
    "crw_labelmap_ordered_joint": (_c_int, ([_p] + [_c_int] * 4) * 2 + [_c_int] * 4 + [_p, _c_int, _c_int, _p, _c_int, _p, _c_sz, _p, _c_sz, _p]),
    "crw_labelmap_ordered_joint_batch": (_c_int, ([_p] + [_c_int] * 4) * 2 + [_c_int] * 5 + [_p, _c_int, _c_int, _p, _c_int, _p, _c_sz, _c_sz, _p,
                                                  _c_sz, _p]),
    "crw_labelmap_posterior_workspace": (_c_sz, [_c_int, _c_int, _c_int]),
    "crw_labelmap_ordered_posterior": (_c_int, [_p] + [_c_int] * 6 + [_p, _c_int, _c_f, _p, _c_int, _c_sz, _p, _p, _c_sz, _p, _c_sz, _p]),
    "crw_labelmap_ordered_joint_posterior": (_c_int, ([_p] + [_c_int] * 4) * 2 + [_c_int] * 4 + [_p, _c_int, _c_int, _c_f, _p, _c_int, _c_sz, _p,
                                                      _p, _c_sz, _p, _c_sz, _p]),
    "crw_labelmap_posterior_workspace_batch": (_c_sz, [_c_int] * 4),
    "crw_labelmap_ordered_posterior_batch": (_c_int, [_p] + [_c_int] * 7 + [_p, _c_int, _c_f, _p, _c_int, _c_sz, _c_sz, _p, _p, _c_sz, _c_sz, _p,
                                                      _c_sz, _p]),
    "crw_labelmap_ordered_joint_posterior_batch": (_c_int, ([_p] + [_c_int] * 4) * 2 + [_c_int] * 5 + [_p, _c_int, _c_int, _c_f, _p, _c_int,
                                                            _c_sz, _c_sz, _p, _p, _c_sz, _c_sz, _p, _c_sz, _p]),
    "crw_linear128_wgrad_ws_bytes": (_c_sz, [_c_int]),
    "crw_linear128_wgrad": (_c_int, [_p, _p, _p, _c_int, _p, _c_sz, _p]),
    "crw_adam_step": (_c_int, [_p, _p, _p, _p, ctypes.c_long, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                               _c_int, _p]),
    "crw_gemm_f32": (_c_int, [_p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_int, _p]),
    "crw_enc_pack_weights": (_c_int, [_p, _c_int, _c_int, _p, _p, _p, _p, _p]),
    "crw_enc_pack_input": (_c_int, [_p, _c_int, _c_int, _p, _p, _p]),
    "crw_enc_pack_input_map": (_c_int, [_p, _c_int, _c_int, _c_int, _c_int, _p, _p, _p]),
    "crw_enc_conv3x3_map": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "crw_enc_conv3x3_wgrad_map": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _p, _p, _p, _p, _p, _p, _p, _c_sz, _p]),
    "crw_enc_conv3x3": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "crw_enc_gap_bwd": (_c_int, [_p, _p, _c_int, _c_int, _c_int, _p, _p, _p]),
    "crw_enc_wgrad_ws_bytes": (_c_sz, [_c_int, _c_int, _c_int, _c_int]),
    "crw_enc_conv3x3_wgrad": (_c_int, [_c_int, _c_int, _c_int, _c_int, _p, _p, _p, _p, _p, _p, _p, _p, _c_sz, _p]),
    "crw_enc_front_pack": (_c_int, [_p, _p, _p, _p, _p, _p]),
    "crw_enc_front_saved_bytes": (_c_sz, [_c_int]),
    "crw_enc_front_fwd": (_c_int, [_c_int, _p, _c_int, _c_int, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "crw_enc_front_fwd_map": (_c_int, [_c_int, _p, _c_int, _c_int, _c_int, _c_int, _p, _p, _p, _p, _p, _p, _p, _p]),
    "crw_enc_front_ws_bytes": (_c_sz, [_c_int, _c_int]),
    "crw_enc_front_bwd": (_c_int, [_c_int, _p, _c_int, _c_int, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                   _c_sz, _p]),
    "crw_enc_front_bwd_map": (_c_int, [_c_int, _p, _c_int, _c_int, _c_int, _c_int, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                       _c_sz, _p]),
    # Resnet encoder kernels
    "crw_rn_padded_patches": (_c_int, [_c_int]),
    "crw_rn_pack_conv": (_c_int, [_p, _c_int, _c_int, _c_int, _c_int, _p, _p, _p, _p, _p]),
    "crw_rn_stem_toeplitz_ld": (_c_int, [_c_int]),
    "crw_rn_pack_stem": (_c_int, [_p, _c_int, _c_int, _p, _p, _p, _p, _p]),
    "crw_rn_conv_part_floats": (_c_sz, [_c_int, _c_int, _c_int]),
    "crw_rn_conv": (_c_int, [_c_int] * 12 + [_p] * 8),
    "crw_rn_wgrad_ws_bytes": (_c_sz, [_c_int] * 12),
    "crw_rn_wgrad": (_c_int, [_c_int] * 12 + [_p] * 6 + [_c_sz, _p]),
    "crw_rn_bn_stats_ws_bytes": (_c_sz, [_c_int]),
    "crw_rn_bn_stats": (_c_int, [_p, _c_int, _c_int, _c_int, _p, _p, _p, _p, _c_f, _c_f, _p, _p, _c_sz, _p]),
    "crw_rn_bn_apply": (_c_int, [_p, _p, _p, _p, _p, _p, _c_int, _c_int, _c_int, _c_int, _p, _p, _p]),
    "crw_rn_bn_pool": (_c_int, [_p, _p, _c_int, _c_int, _c_int, _c_int, _p, _p, _p, _p]),
    "crw_rn_bn_bwd_ws_bytes": (_c_sz, [_c_int, _c_int, _c_int]),
    "crw_rn_bn_bwd": (_c_int, [_p] * 7 + [_c_int] * 3 + [_p] * 10 + [_c_sz, _p]),
    "crw_rn_pool_bwd_ws_bytes": (_c_sz, [_c_int] * 4),
    "crw_rn_pool_bwd": (_c_int, [_p] * 5 + [_c_int] * 4 + [_p] * 5 + [_c_sz, _p]),
    "crw_rn_stem_ws_bytes": (_c_sz, []),
    "crw_rn_stem_fwd": (_c_int, [_p] + [_c_int] * 6 + [_p] * 6 + [_c_f, _c_f] + [_p] * 4 + [_c_sz, _p]),
    "crw_rn_stem_bwd": (_c_int, [_p] * 5 + [_c_int] * 4 + [_p] * 5 + [_c_sz, _p]),
    "crw_rn_split": (_c_int, [_p, _c_int, _c_int, _p, _p, _p]),
    "crw_rn_colsum_ws_bytes": (_c_sz, [_c_int]),
    "crw_rn_colsum": (_c_int, [_p, _c_int, _c_int, _p, _p, _c_sz, _p]),
    "crw_rn_bn_stats_rows": (_c_int, [_p, _c_int, ctypes.c_double, _c_int, _p, _p, _p, _p, _c_f, _c_f, _p, _p, _c_sz, _p]),
    "crw_rn_stem_stats": (_c_int, [_p] + [_c_int] * 4 + [_p] * 6 + [_c_f, _c_f, _p, _p, _c_sz, _p]),
    "crw_rn_stem16_rows": (_c_int, []),
    "crw_rn_pack_stem16": (_c_int, [_p, _p, _p, _p]),
    "crw_rn_stem16_fwd": (_c_int, [_p, _c_int, _c_int, _p, _p, _p, _p, _p]),
    "crw_rn_stem_band_ok": (_c_int, [_c_int, _c_int]),
    "crw_rn_stem_band_fwd": (_c_int, [_p, _c_int, _c_int, _c_int, _c_int, _p, _p, _p, _p, _p]),
    "crw_rn_stem16_ws_bytes": (_c_sz, []),
    "crw_rn_stem16_wgrad": (_c_int, [_p, _c_int, _c_int, _p, _p, _p, _p, _p, _c_sz, _p]),
    "crw_rn_stem16_bwd": (_c_int, [_p, _c_int, _c_int] + [_p] * 11 + [_c_sz, _p]),
    "crw_rn_train_ws_bytes": (_c_sz, [_c_int] * 4),
    "crw_rn_train_fwd": (_c_int, [_p] + [_c_int] * 4 + [_p, _p, _p, _c_f, _c_f, _p, _p, _c_sz, _p]),
    "crw_rn_train_fwd_nograd": (_c_int, [_p] + [_c_int] * 4 + [_p, _p, _p, _c_f, _c_f, _p, _p, _c_sz, _p]),
    "crw_rn_train_bwd": (_c_int, [_p, _p] + [_c_int] * 4 + [_p, _p, _p, _c_sz, _p]),
    "crw_rn_eval_fwd": (_c_int, [_p] + [_c_int] * 4 + [_p, _p, _p, _c_f, _p, _p, _c_sz, _p]),
    "crw_rn_stem_cols": (_c_int, [_c_int]),
    "crw_rn_timing_enable": (_c_int, [_c_int]),
    "crw_rn_timing_read": (_c_int, [_p, _c_int]),
    "crw_gemm_bf16_ws_bytes": (_c_sz, [_c_int, _c_int, _c_int]),
    "crw_gemm_bf16": (_c_int, [_p, _p, _p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _p, _c_sz, _c_int, _p]),
}

# include/crw_hip_chain.h, likewise one to one: the conv-trunk chain (optional: `has_conv_chain()`)
CHAIN_SIGNATURES = {
    "crw_enc_conv_fwd_chain": (_c_int, [_c_int, _c_int] + [_p] * 18),
}

# include/crw_hip_restart.h, likewise: label propagation whose context restarts at an origin frame (optional: `has_anchor_restart()`)
RESTART_SIGNATURES = {
    "crw_labelprop_topk_origin": (_c_int, [_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_f, _c_int, _c_int, _c_int, _p, _p, _p, _c_int, _p]),
    "crw_labelprop_propagate_origin": (_c_int, [_p, _p, _p] + [_c_int] * 6 + [_p, _p, _p, _p]),
    "crw_labelprop_propagate_origin_batch": (_c_int, [_p, _p, _p, _c_sz] + [_c_int] * 7 + [_p, _p, _p, _p]),
}

# include/crw_hip_novelty.h, likewise: context novelty, where a labelled trace would help (optional: `has_novelty()`)
NOVELTY_SIGNATURES = {
    "crw_labelprop_novelty": (_c_int, [_p] + [_c_int] * 7 + [_p, _p, _p, _c_int, _p]),
}

# include/crw_hip_longmem.h, likewise: the sliding rule with n_long long-term frames, a memory bank (optional: `has_long_memory()`)
LONGMEM_SIGNATURES = {
    "crw_labelprop_topk_long": (_c_int, [_p] + [_c_int] * 6 + [_c_f, _c_int, _c_int, _p, _p, _c_int, _c_int, _p]),
    "crw_labelprop_propagate_long": (_c_int, [_p, _p] + [_c_int] * 7 + [_p, _p, _c_int, _p]),
}

# include/crw_hip_align.h, likewise: a bank aligned to its item -- segment-centred features, a bias on the long-term keys (optional: `has_align()`)
ALIGN_SIGNATURES = {
    "crw_center_normalize_ws_bytes": (_c_sz, [_c_int, _c_int, _c_int]),
    "crw_center_normalize": (_c_int, [_p, _c_int, _c_int, _p, _p, _c_int, _p, _c_sz, _p, _p, _p]),
    "crw_labelprop_topk_long_bias": (_c_int, [_p] + [_c_int] * 6 + [_c_f, _c_int, _c_int, _p, _p, _c_int, _c_int, _c_f, _p]),
}

# include/crw_hip_reach.h, likewise: one confusion matrix per group of columns -- accuracy against distance (optional: `has_reach()`)
REACH_SIGNATURES = {
    "crw_confusion_grouped_ws_bytes": (_c_sz, [_c_int, _c_int, _c_int, _c_int]),
    "crw_confusion_grouped": (_c_int, [_p, _c_int, _p, _c_int, _p, _c_int, _p, _c_int, _c_int, _c_sz, _p] + [_c_int] * 5 + [_p, _p, _p, _p, _c_sz, _p]),
}

# include/crw_hip_sweepmem.h, likewise: a memory bank in the parameter sweep -- crw_labelprop_propagate_long for G configurations (optional: `has_sweep_memory()`)
SWEEPMEM_SIGNATURES = {
    "crw_labelprop_propagate_long_batch": (_c_int, [_p, _p, _c_sz] + [_c_int] * 8 + [_p, _p, _p]),
}

# include/crw_hip_guard.h, likewise: the guarded Adam step -- refuse a non-finite gradient, clip by the norm, on the device (optional: `has_guard()`)
GUARD_SIGNATURES = {
    "crw_adam_guard_ws_bytes": (_c_sz, [ctypes.c_long]),
    "crw_adam_step_guarded": (_c_int, [_p, _p, _p, _p, ctypes.c_long, _c_f, _c_f, _c_f, _c_f, _c_int, _c_f, _p, _p, _c_sz, _p]),
}

# include/crw_hip_routes.h, likewise: the route log -- which selector branch launched (optional: `has_routes()`; host pointers)
ROUTES_SIGNATURES = {
    "crw_routes_clear": (_c_int, []),
    "crw_routes_read": (_c_int, [_p, _p, _c_int]),
}

# entry points added at ABI 8 without a bump: a library built before them still loads, `has_sweep()` tells
SWEEP_ENTRY_POINTS = ("crw_labelprop_topk_scores", "crw_labelprop_sweep_weights", "crw_labelprop_propagate_batch")

# likewise: the confidence entry points (`has_confidence()`)
CONFIDENCE_ENTRY_POINTS = ("crw_labelprop_confidence", "crw_merge_confidence", "crw_calibration_ws_bytes", "crw_calibration")

# likewise: the dense label map (`has_dense()`)
DENSE_ENTRY_POINTS = ("crw_labelmap_dense",)

# likewise: the dense label maps of a sweep's G configurations in one launch (`has_dense_batch()`)
DENSE_BATCH_ENTRY_POINTS = ("crw_labelmap_dense_batch",)

# likewise: layer horizons and thickness (`has_horizons()`)
HORIZONS_ENTRY_POINTS = ("crw_horizons_ws_bytes", "crw_horizons")

# likewise: label propagation from the scored frames, the 'sliding' context rule (`has_sliding()`)
SLIDING_ENTRY_POINTS = ("crw_labelprop_propagate_sliding", "crw_labelprop_propagate_sliding_batch")

# likewise: depth-ordered label maps (`has_ordered()`)
ORDERED_ENTRY_POINTS = ("crw_labelmap_ordered_workspace", "crw_labelmap_ordered", "crw_labelmap_ordered_batch")

# likewise: the ordered decode over two passes' rows, the order-preserving merge (`has_joint()`)
JOINT_ENTRY_POINTS = ("crw_labelmap_ordered_joint", "crw_labelmap_ordered_joint_batch")

# likewise: the posterior of the ordered decodes, confidence and horizon error bars (`has_posterior()`)
POSTERIOR_ENTRY_POINTS = ("crw_labelmap_posterior_workspace", "crw_labelmap_ordered_posterior", "crw_labelmap_ordered_joint_posterior")

# likewise: those posteriors for the G configurations of a sweep in one launch (`has_posterior_batch()`)
POSTERIOR_BATCH_ENTRY_POINTS = ("crw_labelmap_posterior_workspace_batch", "crw_labelmap_ordered_posterior_batch",
                                "crw_labelmap_ordered_joint_posterior_batch")

# likewise: conv3 -> conv4 -> conv5 of the CNN encoder in one launch (`has_conv_chain()`; without it the layers run one by one)
CONV_CHAIN_ENTRY_POINTS = tuple(CHAIN_SIGNATURES)

# likewise: the sliding rule with a per-frame origin, anchor_context='restart' (`has_anchor_restart()`)
ANCHOR_RESTART_ENTRY_POINTS = tuple(RESTART_SIGNATURES)

# likewise: the route log (`has_routes()`, `routes()`)
ROUTES_ENTRY_POINTS = tuple(ROUTES_SIGNATURES)

# likewise: context novelty (`has_novelty()`, `labelprop_novelty`)
NOVELTY_ENTRY_POINTS = tuple(NOVELTY_SIGNATURES)

# likewise: the sliding rule with a bank of long-term frames (`has_long_memory()`, `labelprop_topk(n_long=)`)
LONG_MEMORY_ENTRY_POINTS = tuple(LONGMEM_SIGNATURES)

# likewise: segment-centred normalisation and the biased long-memory lists (`has_align()`, `center_normalize`, `labelprop_topk(long_bias=)`)
ALIGN_ENTRY_POINTS = tuple(ALIGN_SIGNATURES)

# likewise: the grouped confusion matrix (`has_reach()`, `confusion_grouped`)
REACH_ENTRY_POINTS = tuple(REACH_SIGNATURES)

# likewise: the batched propagation with a bank of long-term frames (`has_sweep_memory()`, `labelprop_propagate_batch(n_long=)`)
SWEEP_MEMORY_ENTRY_POINTS = tuple(SWEEPMEM_SIGNATURES)

# likewise: the guarded Adam step (`has_guard()`, `adam_step_guarded`)
GUARD_ENTRY_POINTS = tuple(GUARD_SIGNATURES)

CONTEXTS = ("reference", "sliding")  # which frames the indices of a late frame address
ANCHOR_CONTEXTS = ("clamp", "restart")  # what a fully labelled anchor trace does to the frames behind it

# group -> its entry points.  `has_<group>()` tells whether the loaded library exports them, `_<group>_lib()` is lib() or the
# error that names the stale library
OPTIONAL_ENTRY_POINTS = {"sweep": SWEEP_ENTRY_POINTS, "confidence": CONFIDENCE_ENTRY_POINTS, "dense": DENSE_ENTRY_POINTS,
                         "dense_batch": DENSE_BATCH_ENTRY_POINTS, "horizons": HORIZONS_ENTRY_POINTS,
                         "sliding": SLIDING_ENTRY_POINTS, "ordered": ORDERED_ENTRY_POINTS, "joint": JOINT_ENTRY_POINTS,
                         "posterior": POSTERIOR_ENTRY_POINTS, "posterior_batch": POSTERIOR_BATCH_ENTRY_POINTS,
                         "conv_chain": CONV_CHAIN_ENTRY_POINTS, "anchor_restart": ANCHOR_RESTART_ENTRY_POINTS,
                         "routes": ROUTES_ENTRY_POINTS, "novelty": NOVELTY_ENTRY_POINTS, "long_memory": LONG_MEMORY_ENTRY_POINTS,
                         "align": ALIGN_ENTRY_POINTS, "reach": REACH_ENTRY_POINTS, "sweep_memory": SWEEP_MEMORY_ENTRY_POINTS,
                         "guard": GUARD_ENTRY_POINTS}

_lib = None
_present = {}  # group -> the loaded library exports every one of its entry points (filled by lib())


def lib():
    """Load the HIP library (once).  Raises if it has not been built: `python -c 'import
    __graft_entry__ as g; g.build()'` or `make -C radar-sounder-crw_amd/csrc`."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built -- the CRW hot path has no CPU/PyTorch fallback; "
                               "run `make -C radar-sounder-crw_amd/csrc` (hipcc --offload-arch=gfx950)")
        handle = ctypes.CDLL(LIB_PATH)
        missing = {n for names in OPTIONAL_ENTRY_POINTS.values() for n in names if not hasattr(handle, n)}
        for name, (res, args) in {**SIGNATURES, **CHAIN_SIGNATURES, **RESTART_SIGNATURES, **ROUTES_SIGNATURES,
                                   **NOVELTY_SIGNATURES, **LONGMEM_SIGNATURES, **ALIGN_SIGNATURES, **REACH_SIGNATURES, **SWEEPMEM_SIGNATURES,
                                   **GUARD_SIGNATURES}.items():
            if name in missing:
                continue
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        if handle.crw_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} was built for ABI {handle.crw_abi_version()}, include/crw_hip.h says {ABI_VERSION}: "
                               "stale library -- rebuild with `make -C radar-sounder-crw_amd/csrc`")
        _lib = handle
        _present.update((group, not missing & set(names)) for group, names in OPTIONAL_ENTRY_POINTS.items())
    return _lib


def _optional(group, what):
    """(has_<group>, _<group>_lib) of one group of OPTIONAL_ENTRY_POINTS; `what` words the group in has_<group>'s docstring."""
    names = OPTIONAL_ENTRY_POINTS[group]

    def has():
        lib()
        return _present[group]

    def checked_lib():
        handle = lib()
        if not _present[group]:
            raise RuntimeError(f"{LIB_PATH} is a stale libcrw_hip.so: it reports ABI {ABI_VERSION} but lacks {', '.join(names)} "
                               "(added at that ABI) -- rebuild with `make -C radar-sounder-crw_amd/csrc`")
        return handle

    has.__name__, checked_lib.__name__ = f"has_{group}", f"_{group}_lib"
    has.__doc__ = f"True when the loaded library exports {what} ({group.upper()}_ENTRY_POINTS)."
    return has, checked_lib


has_sweep, _sweep_lib = _optional("sweep", "the sweep entry points")
has_confidence, _confidence_lib = _optional("confidence", "the confidence entry points")
has_dense, _dense_lib = _optional("dense", "the dense label map's entry point")
has_dense_batch, _dense_batch_lib = _optional("dense_batch", "the batched dense label map's entry point")
has_horizons, _horizons_lib = _optional("horizons", "the horizon entry points")
has_sliding, _sliding_lib = _optional("sliding", "the sliding-context entry points")
has_ordered, _ordered_lib = _optional("ordered", "the depth-ordered label map's entry points")
has_joint, _joint_lib = _optional("joint", "the joint ordered label map's entry points")
has_posterior, _posterior_lib = _optional("posterior", "the ordered maps' posterior entry points")
has_posterior_batch, _posterior_batch_lib = _optional("posterior_batch", "the batched posterior entry points")
has_conv_chain, _conv_chain_lib = _optional("conv_chain", "the conv-trunk chain entry point")
has_anchor_restart, _anchor_restart_lib = _optional("anchor_restart", "the entry points that take a per-frame origin")
has_routes, _routes_lib = _optional("routes", "the route log's entry points")
has_novelty, _novelty_lib = _optional("novelty", "the context-novelty entry point")
has_long_memory, _long_memory_lib = _optional("long_memory", "the entry points that take n_long long-term frames")
has_align, _align_lib = _optional("align", "the segment-centred normalisation and the biased long-memory lists")
has_reach, _reach_lib = _optional("reach", "the grouped confusion matrix's entry points")
has_sweep_memory, _sweep_memory_lib = _optional("sweep_memory", "the batched propagation that takes n_long long-term frames")
has_guard, _guard_lib = _optional("guard", "the guarded Adam step's entry points")

MAX_ROUTES = 256  # csrc/crw_common.h


def routes_read():
    """{name: count} of the routes (the selector branches, named by CRW_ROUTE in csrc/) that launched since
    the last `routes_clear()`, in this process.  Host work only."""
    handle = _routes_lib()
    names, counts = (ctypes.c_char_p * MAX_ROUTES)(), (ctypes.c_long * MAX_ROUTES)()
    n = handle.crw_routes_read(ctypes.cast(names, _p), ctypes.cast(counts, _p), MAX_ROUTES)
    return {names[i].decode(): counts[i] for i in range(min(n, MAX_ROUTES)) if counts[i]}


def routes_clear():
    _routes_lib().crw_routes_clear()


class routes(dict):
    """`with crw_hip.routes() as hit:` -- the counters are cleared on entry; on exit `hit` holds {name: count} of the routes the
    block's calls took.  The names are decided on the host at launch, so no synchronisation is needed to read them."""

    def __enter__(self):
        self.clear()
        routes_clear()
        return self

    def __exit__(self, *exc):
        self.update(routes_read())
        return False


def check_context(context):
    if context not in CONTEXTS:
        raise ValueError(f"context must be one of {CONTEXTS} (got {context!r})")
    return context


class CrwError(RuntimeError):
    """A non-zero status from the C ABI.  `status` is the CRW_* code: CRW_EINVAL is the caller's data (shape / size / null
    pointer), CRW_EWORKSPACE and CRW_EHIP are failures of the HIP path itself (`hip_error` = the runtime's last error code)."""

    def __init__(self, what, status, hip_error):
        super().__init__(f"{what} failed: {_ERR.get(status, status)} (hipError {hip_error})")
        self.what, self.status, self.hip_error = what, status, hip_error

    @property
    def device_failure(self):
        return self.status != CRW_EINVAL


def _check(status, what):
    if status != CRW_OK:
        raise CrwError(what, status, lib().crw_last_hip_error())


def _dev(t, name, dtype=torch.float32):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on an MI355X device (got {t.device}); the HIP path has no CPU fallback")
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous {dtype}")
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# bench.py sets this to {} for its timed region: every conv / weight-gradient launch is then bracketed by two HIP events
# recorded on the stream the kernel is launched on, {(kind, layer_cin, layer_cout): [(start, end), ...]}.  None = off.
KERNEL_EVENTS = None


def _ev_begin():
    if KERNEL_EVENTS is None:
        return None
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _ev_end(e0, key):
    if e0 is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        KERNEL_EVENTS.setdefault(key, []).append((e0, e1))


def padded_nodes(N, chain=CHAIN_F32):
    return lib().crw_padded_nodes(N, chain)


# ------------------------------------------------------------------------------ training path
def affinity_fwd(emb, tau, want_stats=True):
    """emb [B,T,N,C] -> (A [B,T-1,N,N], ehat, norm, stats [4,B,T-1,N] | None).  stats = row max / row sum exp / column max /
    column sum exp of every A[b,t], from the epilogue of the affinity tiles (walk_fwd then needs no pass over A for them)."""
    B, T, N, C = emb.shape
    ehat = torch.empty_like(emb)
    norm = torch.empty(B, T, N, device=emb.device, dtype=torch.float32)
    A = torch.empty(B, T - 1, N, N, device=emb.device, dtype=torch.float32)
    stats = ws = None
    nbytes = 0
    if want_stats and T > 1:
        stats = torch.empty(4, B, T - 1, N, device=emb.device, dtype=torch.float32)
        nbytes = lib().crw_affinity_ws_bytes(B, T, N)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=emb.device)
    _check(lib().crw_affinity_fwd(_dev(emb, "emb"), B, T, N, C, float(tau), _dev(ehat, "ehat"), _dev(norm, "norm"),
                                  _dev(A, "A"), _dev(stats, "stats") if stats is not None else None,
                                  ctypes.c_void_p(ws.data_ptr()) if ws is not None else None, nbytes, _stream()), "crw_affinity_fwd")
    return A, ehat, norm, stats


def affinity_bwd(dA, ehat, norm, tau):
    B, T, N, C = ehat.shape
    ws = torch.empty_like(ehat)
    demb = torch.empty_like(ehat)
    _check(lib().crw_affinity_bwd(_dev(dA, "dA"), _dev(ehat, "ehat"), _dev(norm, "norm"), B, T, N, C, float(tau),
                                  _dev(ws, "ws"), _dev(demb, "demb"), _stream()), "crw_affinity_bwd")
    return demb


def walk_fwd(A, chain=CHAIN_F32, want_At=False, stats=None):
    """A [B,T-1,N,N] (+ optional stats of affinity_fwd) -> (loss 0-d, state buffer, At [B,T-2,N,N] or None)."""
    B, Tm1, N, _ = A.shape
    T = Tm1 + 1
    nbytes = lib().crw_walk_state_bytes(B, T, N, chain)
    state = torch.empty(nbytes, dtype=torch.uint8, device=A.device)
    loss = torch.empty((), dtype=torch.float32, device=A.device)
    At = torch.empty(B, max(T - 2, 0), N, N, device=A.device, dtype=torch.float32) if want_At else None
    if stats is not None and tuple(stats.shape) != (4, B, Tm1, N):
        raise RuntimeError(f"stats must be [4, {B}, {Tm1}, {N}] (got {tuple(stats.shape)})")
    _check(lib().crw_walk_fwd(_dev(A, "A"), _dev(stats, "stats") if stats is not None else None, B, T, N, chain,
                              ctypes.c_void_p(state.data_ptr()), nbytes,
                              _dev(At, "At") if (want_At and T > 2) else None, _dev(loss, "loss"), _stream()),
           "crw_walk_fwd")
    return loss, state, At


def walk_bwd(gloss, A, state, chain=CHAIN_F32):
    """dLoss/dA for the logits A the forward ran on (the softmaxes are recomputed from A and the statistics in `state`)."""
    B, Tm1, N, _ = A.shape
    T = Tm1 + 1
    nbytes = lib().crw_walk_scratch_bytes(B, T, N, chain)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=state.device)
    dA = torch.empty(B, T - 1, N, N, device=state.device, dtype=torch.float32)
    g = gloss.reshape(1).to(torch.float32).contiguous()
    _check(lib().crw_walk_bwd(_dev(g, "gloss"), _dev(A, "A"), B, T, N, chain, ctypes.c_void_p(state.data_ptr()), state.numel(),
                              ctypes.c_void_p(scratch.data_ptr()), nbytes, _dev(dA, "dA"), _stream()), "crw_walk_bwd")
    return dA


# ------------------------------------------------------------------------------ inference path
def normalize(emb):
    rows, C = emb.numel() // emb.shape[-1], emb.shape[-1]
    ehat = torch.empty_like(emb)
    _check(lib().crw_normalize(_dev(emb, "emb"), rows, C, _dev(ehat, "ehat"), None, _stream()), "crw_normalize")
    return ehat


MEMORY_ALIGNS = (None, "center")  # `memory_align=`: how a bank's features are brought to its item's


def check_memory_align(memory_align):
    if memory_align not in MEMORY_ALIGNS:
        raise ValueError(f"memory_align must be None or 'center' (got {memory_align!r})")
    return memory_align


def check_memory_bias(memory_bias):
    """`memory_bias=` -> float(memory_bias); a bias that is not finite is refused (include/crw_hip_align.h)"""
    b = float(memory_bias)
    if b != b or b in (float("inf"), float("-inf")):
        raise ValueError(f"memory_bias must be a finite number (got {memory_bias!r})")
    return b


def center_normalize(emb, segments, return_mean=False):
    """emb [..., C] raw features, rows = emb.numel() / C; segments: the row offsets [0, ..., rows] of S = len - 1 segments of
    consecutive rows (a sequence of ints: they travel by value, S <= 8; or an int32 tensor on emb's device).  Every segment is
    centred by its own per-channel mean (fp64 sums, the subtraction rounded once to fp32) and then L2-normalised as `normalize`
    does -- crw_center_normalize (include/crw_hip_align.h).  A one-row segment becomes the all-zero row.  -> ehat like emb
    (return_mean: (ehat, mean [S, C] float64)).  CPU tensors: the same definition in torch."""
    C = emb.shape[-1]
    rows = emb.numel() // C
    on_dev = torch.is_tensor(segments)
    S = (segments.numel() if on_dev else len(segments)) - 1
    if not emb.is_cuda:
        b = [int(x) for x in (segments.tolist() if on_dev else segments)]
        if S < 1 or b[0] != 0 or b[-1] != rows or any(y < x for x, y in zip(b, b[1:])):
            raise ValueError(f"segments must be row offsets 0 = b_0 <= ... <= b_S = {rows} (got {b})")
        x = emb.reshape(rows, C).to(torch.float64)
        mean = torch.zeros(S, C, dtype=torch.float64)
        y = torch.empty(rows, C, dtype=torch.float32)
        for s in range(S):
            if b[s + 1] > b[s]:
                mean[s] = x[b[s]:b[s + 1]].sum(0) / (b[s + 1] - b[s])
                y[b[s]:b[s + 1]] = (x[b[s]:b[s + 1]] - mean[s]).to(torch.float32)
        ehat = (y / y.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)).reshape(emb.shape)
        return (ehat, mean) if return_mean else ehat
    handle = _align_lib()
    nbytes = handle.crw_center_normalize_ws_bytes(rows, C, S)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=emb.device)
    ehat = torch.empty_like(emb)
    mean = torch.empty(max(S, 1), C, dtype=torch.float64, device=emb.device) if return_mean else None
    if on_dev:
        seg_dev, seg_host = _dev(segments, "segments", torch.int32), None
    else:
        seg_dev, seg_host = None, (ctypes.c_int32 * (S + 1))(*[int(x) for x in segments])
    _check(handle.crw_center_normalize(_dev(emb, "emb"), rows, C, seg_dev, seg_host, S, ctypes.c_void_p(ws.data_ptr()), nbytes, _dev(ehat, "ehat"),
                                       None if mean is None else ctypes.c_void_p(mean.data_ptr()), _stream()), "crw_center_normalize")
    return (ehat, mean) if return_mean else ehat


def check_anchor_context(anchor_context):
    if anchor_context not in ANCHOR_CONTEXTS:
        raise ValueError(f"anchor_context must be one of {ANCHOR_CONTEXTS} (got {anchor_context!r})")
    return anchor_context


def anchor_origins(anchors, nclasses, T, first_frame=1):
    """The policy of anchor_context='restart': origin [T] int32 (a CPU tensor) for the `origin=` arguments below.  A frame is an
    ORIGIN when it is frame 0, or when all N of its nodes are clamped by `anchors` [T, N] int8 (a class in [0, nclasses); frames
    before first_frame are never clamped, so they restart nothing); origin[n] is the latest origin < n, origin[0] = 0.  A partially
    anchored frame clamps and restarts nothing.  One host read when `anchors` is a device tensor."""
    a = anchors.detach().cpu().to(torch.int64)
    if a.dim() != 2 or a.shape[0] != T:
        raise ValueError(f"anchors must be [{T}, N] (got {tuple(anchors.shape)})")
    full = ((a >= 0) & (a < int(nclasses))).all(1)
    full[:max(int(first_frame), 1)] = False
    latest = torch.cummax(torch.where(full, torch.arange(T), torch.zeros((), dtype=torch.int64)), 0)[0]
    origin = torch.zeros(T, dtype=torch.int32)
    origin[1:] = latest[:-1].to(torch.int32)
    return origin


def check_origin(origin, T):
    """The chain rule of include/crw_hip_restart.h, checked on the host: origin [T] integers with origin[n] in {origin[n - 1], n - 1}
    and 0 <= origin[n] < n for n >= 1 (origin[0] is not read).  -> the values as a list."""
    if origin.dim() != 1 or origin.shape[0] != T or origin.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"origin must be [{T}] int32 (got {tuple(origin.shape)}, {origin.dtype})")
    o = origin.detach().cpu().tolist()
    for n in range(1, T):
        if not 0 <= o[n] < n or (n > 1 and o[n] not in (o[n - 1], n - 1)):
            raise ValueError(f"origin[{n}] = {o[n]} breaks the chain rule: it must be origin[{n - 1}] = {o[n - 1]} or {n - 1}")
    return o


def origin_stretches(o, T, first_frame=1):
    """[(a, e)]: the frames a + 1 .. e (those of first_frame .. T - 1 among them) share the origin a -- the sub-items ehat[a:e + 1]
    the segmented construction runs the entry points without origins on.  o: `check_origin`'s list."""
    out = []
    for n in range(max(int(first_frame), 1), T):
        if out and out[-1][0] == o[n]:
            out[-1][1] = n
        else:
            out.append([o[n], n])
    return [tuple(x) for x in out]


def anchors_restart_segmented():
    """CRW_ANCHORS_RESTART_SEGMENTED=1 (read per call): every `origin=` call below is built from the entry points WITHOUT origins, one
    call per stretch between origins on the sub-item that starts there -- the A/B arm and the device-side definition of the rule."""
    return os.environ.get("CRW_ANCHORS_RESTART_SEGMENTED") == "1"


def _origin_dev(origin, device):
    return origin.to(device=device, dtype=torch.int32).contiguous()


def _topk_origin(ehat, cxt_size, radius, temp, k, first_frame, grid_w, WV, I, raw, origin):
    """`labelprop_topk` / `labelprop_topk_scores` under the restart rule: crw_labelprop_topk_origin, or the segmented construction."""
    T, N, C = ehat.shape
    o = check_origin(origin, T)
    if anchors_restart_segmented():
        fn, what = (_sweep_lib().crw_labelprop_topk_scores, "crw_labelprop_topk_scores") if raw else \
            (lib().crw_labelprop_topk_grid, "crw_labelprop_topk_grid")
        for a, e in origin_stretches(o, T, first_frame):
            ff = max(int(first_frame) - a, 1)
            at = a + ff - int(first_frame)  # the stretch's first frame in the lists
            _check(fn(_dev(ehat[a:], "ehat"), e + 1 - a, N, C, int(cxt_size), int(radius), float(temp), int(k), ff, int(grid_w),
                      _dev(WV[at:], "W"), _dev(I[at:], "I", torch.int32), _stream()), what)
        return WV, I
    org = _origin_dev(origin, ehat.device)
    _check(_anchor_restart_lib().crw_labelprop_topk_origin(_dev(ehat, "ehat"), T, N, C, int(cxt_size), int(radius), float(temp), int(k),
                                                           int(first_frame), int(grid_w), _dev(org, "origin", torch.int32),
                                                           _dev(WV, "W"), _dev(I, "I", torch.int32), int(raw), _stream()),
           "crw_labelprop_topk_origin")
    return WV, I


LONG_ROUTES = {"auto": 0, "vector": 1, "matrix": 2}       # `labelprop_topk(n_long=, route=)`; the C codes pass as they are
LONG_GATHER_ROUTES = {"auto": 0, "general": 1, "ring": 2}  # `labelprop_gather(n_long=, route=)`


def check_n_long(n_long, T, first_frame, origin=None, grid_w=1):
    """what every `n_long=` argument must obey (include/crw_hip_longmem.h) -> int(n_long)"""
    n_long = int(n_long)
    if n_long == 1:  # frame 0 alone: nothing is asked that the entry points do not check themselves
        return 1
    if not 1 <= n_long <= T - 1:
        raise ValueError(f"n_long must be in 1 .. T - 1 = {T - 1} (got {n_long})")
    if not 1 <= int(first_frame) <= T - 1:
        raise ValueError(f"first_frame must be in 1 .. T - 1 = {T - 1} (got {first_frame})")
    if origin is not None:
        raise ValueError("n_long > 1 and origin are not combined: a restart's long-term frame is its origin alone")
    if grid_w != 1:
        raise ValueError("n_long > 1 is defined on N x 1 grids only")
    return n_long


def _topk_long(ehat, cxt_size, n_long, radius, temp, k, first_frame, WV, I, raw, route, origin=None, grid_w=1, long_bias=None):
    if origin is not None or grid_w != 1:
        raise ValueError("route= goes through crw_labelprop_topk_long: N x 1 grids, no origin")
    T, N, C = ehat.shape
    if long_bias is not None:  # include/crw_hip_align.h: the same call with the bias on the long-term keys
        _check(_align_lib().crw_labelprop_topk_long_bias(_dev(ehat, "ehat"), T, N, C, int(cxt_size), int(n_long), int(radius), float(temp),
                                                         int(k), int(first_frame), _dev(WV, "WV"), _dev(I, "I", torch.int32), int(raw),
                                                         LONG_ROUTES.get(route, route), check_memory_bias(long_bias), _stream()),
               "crw_labelprop_topk_long_bias")
        return WV, I
    _check(_long_memory_lib().crw_labelprop_topk_long(_dev(ehat, "ehat"), T, N, C, int(cxt_size), int(n_long), int(radius), float(temp),
                                                      int(k), int(first_frame), _dev(WV, "WV"), _dev(I, "I", torch.int32), int(raw),
                                                      LONG_ROUTES.get(route, route), _stream()), "crw_labelprop_topk_long")
    return WV, I


def labelprop_topk(ehat, cxt_size, radius, temp, knn, first_frame=1, grid_w=1, origin=None, n_long=1, route=None, long_bias=None):
    """grid_w: the N nodes of a frame form an (N / grid_w) x grid_w grid (1 = a radargram's column of patches).
    origin ([T] int32, `anchor_origins`): frame n scores against frame origin[n] and the frames between it and n only, as frame
    n - origin[n] of the item that starts there (include/crw_hip_restart.h); None: every frame scores from frame 0.
    n_long: the first n_long frames of ehat are long-term -- every frame scores against them and the cxt_size frames before it
    (include/crw_hip_longmem.h, crw_labelprop_topk_long; N x 1 grids, no origin).  1 with route None: frame 0 alone, the call as it
    has always been.  route (a key of LONG_ROUTES; tests and timing): crw_labelprop_topk_long on that route, at n_long = 1 as well.
    long_bias (a finite float; None: no such call): crw_labelprop_topk_long_bias (include/crw_hip_align.h) -- the number is added to
    the cosine of the in-band keys of the long-term frames before the division by temp; 0.0 gives crw_labelprop_topk_long's bits."""
    T, N, C = ehat.shape
    n_long = check_n_long(n_long, T, first_frame, origin, grid_w)
    W = torch.empty(T - first_frame, knn, N, device=ehat.device, dtype=torch.float32)
    I = torch.empty(T - first_frame, knn, N, device=ehat.device, dtype=torch.int32)
    if n_long > 1 or route is not None or long_bias is not None:
        return _topk_long(ehat, cxt_size, n_long, radius, temp, knn, first_frame, W, I, 0, route or "auto", origin, grid_w, long_bias)
    if origin is not None:
        return _topk_origin(ehat, cxt_size, radius, temp, knn, first_frame, grid_w, W, I, 0, origin)
    _check(lib().crw_labelprop_topk_grid(_dev(ehat, "ehat"), T, N, C, int(cxt_size), int(radius), float(temp), int(knn),
                                         int(first_frame), int(grid_w), _dev(W, "W"), _dev(I, "I", torch.int32), _stream()),
           "crw_labelprop_topk_grid")
    return W, I


def sliding_rows(I, N, cxt_size, first_frame=1):
    """The 'sliding' rule's translation as torch ops: I [..., F, knn, N], the indices of `labelprop_topk(_scores)` for frames
    first_frame .. first_frame + F - 1 at `cxt_size` -> the label rows they address when applied to the frames they were scored on:
    i where i < N or n <= cxt_size + 1, else i + (n - cxt_size - 1) * N.  Same dtype and device, a new tensor."""
    F = I.shape[-3]
    n = torch.arange(first_frame, first_frame + F, device=I.device, dtype=I.dtype)
    shift = ((n - (int(cxt_size) + 1)).clamp_(min=0) * int(N)).view(F, 1, 1)
    return torch.where(I >= N, I + shift, I)


ANCHOR_WEIGHT = float("-inf")  # CRW_LABELPROP_ANCHOR_WEIGHT: a slot-0 weight with these bits (0xFF800000) marks an anchored node


def check_anchors(anchors, T, N, M):
    """the shape, dtype and class-count rules of every `anchors=` argument"""
    if tuple(anchors.shape) != (T, N) or anchors.dtype != torch.int8:
        raise ValueError(f"anchors must be a [{T}, {N}] int8 tensor (got {tuple(anchors.shape)}, {anchors.dtype})")
    if M > 127:
        raise ValueError(f"anchors are int8: at most 127 classes (got {M})")


def mark_anchors(W, I, anchors, M, first_frame=1):
    """Write anchor marks into the lists of the sliding entry points, IN PLACE (include/crw_hip.h, crw_labelprop_propagate_sliding):
    for every node q of frame f >= first_frame with 0 <= anchors[f, q] < M, the slot-0 weight becomes -inf and the slot-0 index the
    class.  W [F, knn, N] or [G, F, knn, N] float32 and I likewise int32 (each on its own: a [G, ...] W may share one [F, knn, N] I),
    the lists of frames first_frame .. first_frame + F - 1; anchors [T, N] int8, T >= first_frame + F.  Any other value of `anchors`
    leaves the node free, rows before first_frame are ignored, no slot but 0 is touched.  Two selects on the slot-0 views: nothing
    is read back from the device and nothing is allocated per anchored frame; CPU tensors work as well.  -> (W, I)"""
    F, N = W.shape[-3], W.shape[-1]
    if I.shape[-3:] != W.shape[-3:] or W.dim() not in (3, 4) or I.dim() not in (3, 4):
        raise ValueError(f"W and I must be [F, knn, N] or [G, F, knn, N] lists of the same frames (got {tuple(W.shape)}, {tuple(I.shape)})")
    if anchors.dim() != 2 or anchors.shape[1] != N or anchors.shape[0] < first_frame + F:
        raise ValueError(f"anchors must be [T >= {first_frame + F}, {N}] (got {tuple(anchors.shape)})")
    a = anchors[first_frame:first_frame + F].to(device=W.device, dtype=torch.int32)    # [F, N]
    valid = (a >= 0) & (a < M)
    w0, i0 = W.select(-2, 0), I.select(-2, 0)                                              # [..., F, N] views of slot 0
    torch.where(valid, torch.full((), ANCHOR_WEIGHT, device=W.device, dtype=W.dtype), w0, out=w0)
    torch.where(valid, a.to(I.dtype), i0, out=i0)
    return W, I


_anchor_lists = {}  # library path -> the loaded library honours anchor marks


def has_anchor_lists():
    """True when the loaded library honours anchor marks in the lists of the sliding entry points.  Neither the ABI number nor a
    symbol tells: a library from before the marks has the same entry points and turns the -inf weight into NaN.  So this asks the
    library itself, once per library: one marked call at T = 2, N = 1, M = 2 (the node of frame 1 anchored to class 1) whose row
    must come back as the one-hot [0, 1].  False: `labelprop_gather(anchors=)` takes the segmented route."""
    if LIB_PATH not in _anchor_lists:
        ok = has_sliding() and torch.cuda.is_available()
        if ok:
            seed = torch.zeros(1, device="cuda")
            W, I = torch.full((1, 1, 1), ANCHOR_WEIGHT, device="cuda"), torch.ones(1, 1, 1, device="cuda", dtype=torch.int32)
            L, pred = torch.zeros(2, 2, device="cuda"), torch.zeros(1, 2, device="cuda")
            _check(lib().crw_labelprop_propagate_sliding(_dev(seed, "seed"), _dev(W, "W"), _dev(I, "I", torch.int32), 2, 1, 2, 1, 1, 1,
                                                         _dev(L, "L"), _dev(pred, "pred"), _stream()), "crw_labelprop_propagate_sliding")
            ok = L[1].tolist() == [0.0, 1.0] and pred[0].tolist() == [0.0, 1.0]
        _anchor_lists[LIB_PATH] = ok
    return _anchor_lists[LIB_PATH]


def anchors_segmented():
    """CRW_ANCHORS_SEGMENTED=1 (read per call), or a library without anchor marks: anchored propagation runs as segments
    (`_propagate_anchored`) instead of one launch on marked lists."""
    return os.environ.get("CRW_ANCHORS_SEGMENTED") == "1" or not has_anchor_lists()


def _propagate_anchored(seed, W, I, anchors, T, N, M, knn, first_frame, cxt_size, L, pred):
    """Anchored propagation as segments of crw_labelprop_propagate_sliding: the entry point up to the next frame that holds a
    clamped node, that frame's clamped rows of L and entries of pred overwritten, then again with seed = NULL and first_frame = that
    frame + 1 on the same L ("frames before first_frame are the caller's") and the W / I slices that start there.  One launch per
    segment -- K + 1 for K anchored frames; pred of a segment goes through a [N, end + 1] view of one scratch buffer, the entry
    point's layout.  The frames are found on the host: from `anchors` itself when it is a CPU tensor (it is then uploaded here, and
    nothing waits for the device), else by one read of the device tensor."""
    fn = _sliding_lib().crw_labelprop_propagate_sliding
    host = anchors if not anchors.is_cuda else anchors.cpu()  # (a device tensor: the one host read)
    frames = [f for f in ((host >= 0) & (host < M)).any(1).nonzero().reshape(-1).tolist() if f >= first_frame]
    a = anchors.to(device=L.device, dtype=torch.int64)[frames]                               # [K, N]
    valid = (a >= 0) & (a < M)
    onehot = (a[:, :, None] == torch.arange(M, device=a.device)).to(L.dtype)                 # [K, N, M]; a free node's row is unused
    cls = a.to(pred.dtype)
    ends = frames + ([T - 1] if not frames or frames[-1] != T - 1 else [])
    scratch = torch.empty(N * T, device=pred.device, dtype=pred.dtype) if ends[0] != T - 1 else None
    start = first_frame
    for k, end in enumerate(ends):
        Te = end + 1
        part = pred if Te == T else scratch[:N * Te].view(N, Te)                             # columns start .. end are written
        o = start - first_frame
        first = seed is not None and start == first_frame
        _check(fn(_dev(seed, "seed") if first else None, _dev(W[o:], "W"), _dev(I[o:], "I", torch.int32), Te, N, M, knn, start,
                  int(cxt_size), _dev(L, "L"), _dev(part, "pred"), _stream()), "crw_labelprop_propagate_sliding")
        if part is not pred:
            pred[:, start:Te] = part[:, start:Te]
            if first:
                pred[:, 0] = part[:, 0]
        if k < len(frames):  # selects in place, not masked assignments: nothing here waits for the device
            row, col = L[end * N:(end + 1) * N], pred[:, end]
            torch.where(valid[k, :, None], onehot[k], row, out=row)
            torch.where(valid[k], cls[k], col, out=col)
        start = end + 1
    return L, pred


def _propagate_origin_segmented(seed, W, I, o, T, N, M, knn, first_frame, cxt_size, L, pred):
    """The restart rule from crw_labelprop_propagate_sliding alone: per stretch (a, e) of `origin_stretches` one call on the sub-item
    L[a * N:(e + 1) * N] -- frame a is the sub-item's frame 0 and the caller's (seed = NULL; the seed itself only where a = 0 holds the
    call's first frame) -- with the list slices that start at the stretch's first frame, marks and all.  pred of a sub-item goes
    through a [N, e + 1 - a] view of one scratch buffer, the entry point's layout."""
    fn = _sliding_lib().crw_labelprop_propagate_sliding
    scratch = torch.empty(N * T, device=pred.device, dtype=pred.dtype)
    if seed is not None and o[first_frame] != 0:  # no stretch starts at frame 0: the seed's frame is written here
        L[:N] = (seed[:, None] == torch.arange(M, device=seed.device)).to(L.dtype)
        pred[:, 0] = seed
    for a, e in origin_stretches(o, T, first_frame):
        Ts, ff = e + 1 - a, max(first_frame - a, 1)
        at = a + ff - first_frame
        first = seed is not None and a == 0
        whole = a == 0 and Ts == T
        part = pred if whole else scratch[:N * Ts].view(N, Ts)
        _check(fn(_dev(seed, "seed") if first else None, _dev(W[at:], "W"), _dev(I[at:], "I", torch.int32), Ts, N, M, knn, ff,
                  int(cxt_size), _dev(L[a * N:], "L"), _dev(part, "pred"), _stream()), "crw_labelprop_propagate_sliding")
        if not whole:
            pred[:, a + ff:e + 1] = part[:, ff:]
            if first:
                pred[:, 0] = part[:, 0]
    return L, pred


def labelprop_gather(seed, W, I, T, N, M, first_frame=1, L=None, pred=None, cxt_size=None, context="reference", anchors=None,
                     origin=None, n_long=1, route=None):
    """cxt_size: the context size the lists were made with by `labelprop_topk` (same first_frame) -> crw_labelprop_propagate
    (chained frames in one workgroup, the frames beyond the context bound all at once); None: any lists, one workgroup.
    context='sliding' (needs cxt_size): the indices address the frames they were scored on -- crw_labelprop_propagate_sliding,
    bitwise `labelprop_gather(seed, W, sliding_rows(I, N, cxt_size, first_frame), ...)` with cxt_size None.
    anchors (needs context='sliding'): [T, N] int8, on the device or on the host, labelled nodes inside the item -- a value in [0, M) clamps the
    node's row of L to that class's one-hot before the next frame reads it, any other value (-1; M, 127, -128 likewise) leaves it
    free; rows of frames before first_frame are ignored.  ONE crw_labelprop_propagate_sliding call on a marked COPY of W and I
    (`mark_anchors`; the caller's lists are left as they are -- a caller that owns its lists marks them itself and passes no
    anchors).  CRW_ANCHORS_SEGMENTED=1 (read per call), or a library that does not know the marks (`has_anchor_lists()`): once per
    stretch between anchored frames instead (`_propagate_anchored`), the same bits.  None: the call is what it was.
    origin (needs context='sliding'; [T] int32, `anchor_origins`): the lists are `labelprop_topk(..., origin=origin)`'s and frame n
    reads the rows of the item that starts at origin[n] (include/crw_hip_restart.h) -- ONE crw_labelprop_propagate_origin call,
    anchors marked as above; CRW_ANCHORS_RESTART_SEGMENTED=1 (read per call): crw_labelprop_propagate_sliding once per stretch
    between origins on the sub-item that starts there, the same bits.
    n_long (needs context='sliding'; no origin): the lists are `labelprop_topk(..., n_long=n_long)`'s, the first n_long frames are
    long-term (include/crw_hip_longmem.h) -- ONE crw_labelprop_propagate_long call, anchors marked as above.  That entry point takes
    no seed: with one, its one-hot rows and pred[:, 0] are written here first; the rows of L before first_frame are the caller's.
    1 with route None: the call is what it was.  route (a key of LONG_GATHER_ROUTES; tests and timing): crw_labelprop_propagate_long
    on that route, at n_long = 1 as well."""
    knn = W.shape[1]
    check_context(context)
    n_long = check_n_long(n_long, T, first_frame, origin)
    long_memory = n_long > 1 or route is not None
    if long_memory and origin is not None:
        raise ValueError("route= goes through crw_labelprop_propagate_long: no origin")
    if long_memory and context != "sliding":
        raise ValueError("n_long needs context='sliding' (and cxt_size): under the reference rule a late frame never reads a label "
                         "later than frame cxt_size, so beyond cxt_size + 1 frames it would not read the bank's rows consistently")
    if context == "sliding" and cxt_size is None:
        raise ValueError("context='sliding' needs cxt_size (the context size the lists were made with)")
    if origin is not None:
        if context != "sliding":
            raise ValueError("origin needs context='sliding' (and cxt_size): the restart rule is defined on the frames the lists were "
                             "scored on")
        o = check_origin(origin, T)
    if anchors is not None:
        if context != "sliding":
            raise ValueError("anchors need context='sliding' (and cxt_size): under the reference rule a late frame never reads a "
                             "label later than frame cxt_size, so an anchor there would change only itself")
        check_anchors(anchors, T, N, M)
    if L is None:
        L = torch.empty(T * N, M, device=W.device, dtype=torch.float32)
    if pred is None:
        pred = torch.zeros(N, T, device=W.device, dtype=torch.float32)
    if anchors is not None:
        if origin is None and not long_memory and anchors_segmented():
            return _propagate_anchored(seed, W, I, anchors, T, N, M, knn, int(first_frame), cxt_size, L, pred)
        W, I = mark_anchors(W.clone(), I.clone(), anchors, M, int(first_frame))
    if long_memory:
        if seed is not None:  # frame 0 from the seed, as the entry points with a seed argument write it
            L[:N] = (seed[:, None] == torch.arange(M, device=seed.device)).to(L.dtype)
            pred[:, 0] = seed
        _check(_long_memory_lib().crw_labelprop_propagate_long(_dev(W, "W"), _dev(I, "I", torch.int32), T, N, M, knn, int(first_frame),
                                                               int(cxt_size), n_long, _dev(L, "L"), _dev(pred, "pred"),
                                                               LONG_GATHER_ROUTES.get(route or "auto", route), _stream()),
               "crw_labelprop_propagate_long")
        return L, pred
    if origin is not None:
        if anchors_restart_segmented():
            return _propagate_origin_segmented(seed, W, I, o, T, N, M, knn, int(first_frame), cxt_size, L, pred)
        org = _origin_dev(origin, W.device)
        _check(_anchor_restart_lib().crw_labelprop_propagate_origin(_dev(seed, "seed") if seed is not None else None, _dev(W, "W"),
                                                                    _dev(I, "I", torch.int32), T, N, M, knn, int(first_frame),
                                                                    int(cxt_size), _dev(org, "origin", torch.int32), _dev(L, "L"),
                                                                    _dev(pred, "pred"), _stream()), "crw_labelprop_propagate_origin")
        return L, pred
    if context == "sliding":
        _check(_sliding_lib().crw_labelprop_propagate_sliding(_dev(seed, "seed") if seed is not None else None, _dev(W, "W"),
                                                              _dev(I, "I", torch.int32), T, N, M, knn, int(first_frame), int(cxt_size),
                                                              _dev(L, "L"), _dev(pred, "pred"), _stream()),
               "crw_labelprop_propagate_sliding")
        return L, pred
    if cxt_size is not None:
        _check(lib().crw_labelprop_propagate(_dev(seed, "seed") if seed is not None else None, _dev(W, "W"),
                                             _dev(I, "I", torch.int32), T, N, M, knn, int(first_frame), int(cxt_size),
                                             _dev(L, "L"), _dev(pred, "pred"), _stream()), "crw_labelprop_propagate")
        return L, pred
    _check(lib().crw_labelprop_gather(_dev(seed, "seed") if seed is not None else None, _dev(W, "W"),
                                      _dev(I, "I", torch.int32), T, N, M, knn, int(first_frame), _dev(L, "L"),
                                      _dev(pred, "pred"), _stream()), "crw_labelprop_gather")
    return L, pred


def labelprop_topk_scores(ehat, cxt_size, radius, temp, kcap, first_frame=1, grid_w=1, out=None, origin=None, n_long=1, route=None,
                          long_bias=None):
    """`labelprop_topk` with the selected logits V [T-first_frame, kcap, N] instead of their softmax weights (empty slot -inf), and
    the same I: the lists of every knn <= kcap are their first knn entries (`labelprop_sweep_weights` makes the weights).
    out: (V, I) tensors of those shapes to write into.  origin, n_long, route, long_bias: as in `labelprop_topk` (the logits
    include the bias)."""
    T, N, C = ehat.shape
    n_long = check_n_long(n_long, T, first_frame, origin, grid_w)
    if out is not None:
        V, I = out
        if tuple(V.shape) != (T - first_frame, kcap, N) or tuple(I.shape) != tuple(V.shape):
            raise RuntimeError(f"out must be two {(T - first_frame, kcap, N)} tensors (got {tuple(V.shape)}, {tuple(I.shape)})")
    else:
        V = torch.empty(T - first_frame, kcap, N, device=ehat.device, dtype=torch.float32)
        I = torch.empty(T - first_frame, kcap, N, device=ehat.device, dtype=torch.int32)
    if n_long > 1 or route is not None or long_bias is not None:
        return _topk_long(ehat, cxt_size, n_long, radius, temp, kcap, first_frame, V, I, 1, route or "auto", origin, grid_w, long_bias)
    if origin is not None:
        return _topk_origin(ehat, cxt_size, radius, temp, kcap, first_frame, grid_w, V, I, 1, origin)
    _check(_sweep_lib().crw_labelprop_topk_scores(_dev(ehat, "ehat"), T, N, C, int(cxt_size), int(radius), float(temp), int(kcap),
                                                  int(first_frame), int(grid_w), _dev(V, "V"), _dev(I, "I", torch.int32), _stream()),
           "crw_labelprop_topk_scores")
    return V, I


NOVELTY_ROUTES = {"auto": 0, "vector": 1, "matrix": 2}  # `labelprop_novelty(route=)`; the C codes 0 / 1 / 2 pass as they are
NOVELTY_MAX_NODES = 4096


def novelty_top(N, top=None):
    """how many of a frame's N node novelties its score averages: max(1, N // 4) unless given"""
    top = max(1, N // 4) if top is None else int(top)
    if not 1 <= top <= N:
        raise ValueError(f"top must lie in 1 .. N = {N} (got {top})")
    return top


def labelprop_novelty(ehat, cxt_size, radius, top=None, first_frame=1, origin=None, route="auto"):
    """How well each node's best key in its propagation context matches it (include/crw_hip_novelty.h) -> (nov [T - first_frame, N],
    score [T - first_frame]) on the device, one launch.  nov[n, q] = 1 - max <ehat[n, q], key> over the in-band nodes (|p - q| <
    radius, an N x 1 grid) of the frames `labelprop_topk` scores frame n against -- frame origin[n] and the cxt_size frames before
    n that lie behind it (origin: `anchor_origins`, as in `labelprop_topk`; None: frame 0); score[n] = the mean of the `top`
    (default max(1, N // 4)) largest nov[n, :].  A one-frame peak of the score marks a frame whose nodes have nothing like them
    among their keys: `suggest_frames`.  route: 'auto', 'vector', 'matrix' (or the C codes 0, 1, 2)."""
    T, N, C = ehat.shape
    top = novelty_top(N, top)
    code = NOVELTY_ROUTES.get(route, route)
    if code not in (0, 1, 2):
        raise ValueError(f"route must be one of {tuple(NOVELTY_ROUTES)} (got {route!r})")
    org = None
    if origin is not None:
        check_origin(origin, T)
        org = _origin_dev(origin, ehat.device)
    nov = torch.empty(T - first_frame, N, device=ehat.device, dtype=torch.float32)
    score = torch.empty(T - first_frame, device=ehat.device, dtype=torch.float32)
    _check(_novelty_lib().crw_labelprop_novelty(_dev(ehat, "ehat"), T, N, C, int(cxt_size), int(radius), int(first_frame), top,
                                                None if org is None else _dev(org, "origin", torch.int32), _dev(nov, "nov"),
                                                _dev(score, "score"), code, _stream()), "crw_labelprop_novelty")
    return nov, score


def suggest_frames(score, cxt_size, budget, min_gap=2, first_frame=1, anchored=None):
    """Where to label next, from `labelprop_novelty`'s frame scores: -> [(frame, z, s)] in pick order.  Host work only (CPU tensors,
    numpy or lists; a device tensor is copied once), usable without a GPU.
    score [F]: entry i is frame first_frame + i.  In float64: z[n] = s[n] - median of the other scored frames within cxt_size of n
    (a young context, just after frame 0 or a restart, lifts s for several frames; an onset is a one-frame peak); then `budget`
    rounds of "largest z, lowest frame on ties, drop the frames within min_gap of it".  anchored: frames that are fully labelled
    already; they and their neighbours within min_gap are dropped first.  Fewer than `budget` picks when the frames run out.
    The z of items in which nothing emerges overlap those of weak onsets: a pick is a place to look, not a detection."""
    import numpy as np
    s = np.asarray(score.detach().cpu() if torch.is_tensor(score) else score, dtype=np.float64).reshape(-1)
    F, cxt, gap, first = len(s), int(cxt_size), int(min_gap), int(first_frame)
    if cxt < 1 or gap < 0 or int(budget) < 0 or first < 0:
        raise ValueError(f"cxt_size >= 1, min_gap >= 0, budget >= 0 and first_frame >= 0 (got {cxt_size}, {min_gap}, {budget}, {first_frame})")
    z = np.empty(F)
    for i in range(F):
        lo, hi = max(0, i - cxt), min(F - 1, i + cxt)
        nb = np.concatenate([s[lo:i], s[i + 1:hi + 1]])
        z[i] = s[i] - (np.median(nb) if nb.size else 0.0)
    left = np.ones(F, bool)

    def drop(frame):
        left[max(frame - gap - first, 0):max(frame + gap + 1 - first, 0)] = False

    for f in (anchored if anchored is not None else ()):
        drop(int(f))
    out = []
    for _ in range(int(budget)):
        if not left.any():
            break
        i = int(np.argmax(np.where(left, z, -np.inf)))         # the first maximum: the lowest frame on ties
        out.append((first + i, float(z[i]), float(s[i])))
        drop(first + i)
    return out


def labelprop_sweep_weights(V, knns, out=None):
    """V [F, kcap, N] of `labelprop_topk_scores`, knns: 1 ... 16 values in 1 ... kcap -> W [len(knns), F, max(knns), N]:
    W[i][:, :knns[i]] is bitwise the W of `labelprop_topk(..., knn=knns[i])`, the slots behind are 0.  out: a [len(knns), F,
    max(knns), N] view to write into."""
    F, kcap, N = V.shape
    knns = [int(k) for k in knns]
    if not knns:
        raise ValueError("knns is empty")
    arr = (ctypes.c_int * len(knns))(*knns)
    W = out if out is not None else torch.empty(len(knns), F, max(knns), N, device=V.device, dtype=torch.float32)
    if tuple(W.shape) != (len(knns), F, max(knns), N):
        raise RuntimeError(f"out must be {(len(knns), F, max(knns), N)} (got {tuple(W.shape)})")
    _check(_sweep_lib().crw_labelprop_sweep_weights(_dev(V, "V"), F, kcap, N, arr, len(knns), _dev(W, "W"), _stream()),
           "crw_labelprop_sweep_weights")
    return W


def sweep_memory_fits(N, M, n_long):
    """crw_labelprop_propagate_long_batch's one condition per geometry (include/crw_hip_sweepmem.h): the n_long long-term frames and
    a ring of two fit the 150 KiB of LDS"""
    return (int(n_long) + 2) * N * M * 4 <= 150 * 1024


def labelprop_propagate_batch(seed, W, I, T, N, M, first_frame=1, cxt_size=None, L=None, pred=None, context="reference", origin=None,
                              n_long=None):
    """G configurations' `labelprop_gather(..., cxt_size=cxt_size, context=context)` in one call: W [G, T-first_frame, knn, N]; I the same shape, or
    [T-first_frame, knn, N] shared by all -> (L [G, T*N, M], pred [G, N, T]), slice g bitwise what the per-configuration call
    gives on W[g] (shorter lists padded with zero weights).  seed None: L's frames before first_frame are filled by the caller.
    origin (needs context='sliding'): ONE [T] int32 origin array for the G configurations -- crw_labelprop_propagate_origin_batch;
    CRW_ANCHORS_RESTART_SEGMENTED=1 (read per call): the segmented `labelprop_gather(origin=)`, configuration by configuration.
    n_long (needs context='sliding'; no origin): the lists are `labelprop_topk_scores(..., n_long=n_long)`'s and the first n_long
    frames are long-term (include/crw_hip_sweepmem.h) -- ONE crw_labelprop_propagate_long_batch call.  That entry point takes no
    seed: with one, its one-hot rows and pred[:, :, 0] are written here first; the rows of L before first_frame are the caller's.
    Where the bank and a ring of two frames do not fit LDS (`sweep_memory_fits`), or N * M * 4 > 30 KiB: crw_labelprop_propagate_long,
    configuration by configuration, the same bits.  None: the call is what it was."""
    if cxt_size is None:
        raise ValueError("cxt_size (the context size the lists were made with) is required")
    check_context(context)
    if n_long is not None:
        if origin is not None:
            raise ValueError("n_long and origin are not combined: a restart's long-term frame is its origin alone")
        if context != "sliding":
            raise ValueError("n_long needs context='sliding' (and cxt_size): under the reference rule a late frame never reads a label "
                             "later than frame cxt_size, so beyond cxt_size + 1 frames it would not read the bank's rows consistently")
        n_long = int(n_long)
        if not 1 <= n_long <= T - 1:
            raise ValueError(f"n_long must be in 1 .. T - 1 = {T - 1} (got {n_long})")
    if origin is not None:
        if context != "sliding":
            raise ValueError("origin needs context='sliding' (and cxt_size): the restart rule is defined on the frames the lists were "
                             "scored on")
        check_origin(origin, T)
    G, F, knn = W.shape[0], W.shape[1], W.shape[2]
    if W.dim() != 4 or F != T - first_frame or W.shape[3] != N:
        raise RuntimeError(f"W must be [G, {T - first_frame}, knn, {N}] (got {tuple(W.shape)})")
    if tuple(I.shape) == tuple(W.shape):
        stride = F * knn * N
    elif tuple(I.shape) == tuple(W.shape[1:]):
        stride = 0
    else:
        raise RuntimeError(f"I must be {tuple(W.shape)} or {tuple(W.shape[1:])} (got {tuple(I.shape)})")
    if L is None:
        if seed is None:
            raise ValueError("without a seed, L (frames before first_frame filled) is required")
        L = torch.empty(G, T * N, M, device=W.device, dtype=torch.float32)
    if pred is None:
        pred = torch.zeros(G, N, T, device=W.device, dtype=torch.float32)
    if tuple(L.shape) != (G, T * N, M) or tuple(pred.shape) != (G, N, T):
        raise RuntimeError(f"L must be {(G, T * N, M)} and pred {(G, N, T)} (got {tuple(L.shape)}, {tuple(pred.shape)})")
    if n_long is not None:
        if seed is not None:  # frame 0 from the seed, as the entry points with a seed argument write it
            L[:, :N] = (seed[:, None] == torch.arange(M, device=seed.device)).to(L.dtype)
            pred[:, :, 0] = seed
        if not sweep_memory_fits(N, M, n_long) or N * M * 4 > 30 * 1024:  # the one-configuration routes, slice by slice
            for g in range(G):
                labelprop_gather(None, W[g], I[g] if stride else I, T, N, M, first_frame, L[g], pred[g], cxt_size, "sliding",
                                 n_long=n_long, route="auto")
            return L, pred
        _check(_sweep_memory_lib().crw_labelprop_propagate_long_batch(_dev(W, "W"), _dev(I, "I", torch.int32), stride, G, T, N, M, knn,
                                                                      int(first_frame), int(cxt_size), n_long, _dev(L, "L"),
                                                                      _dev(pred, "pred"), _stream()),
               "crw_labelprop_propagate_long_batch")
        return L, pred
    if origin is not None:
        if anchors_restart_segmented():
            for g in range(G):
                labelprop_gather(seed, W[g], I[g] if stride else I, T, N, M, first_frame, L[g], pred[g], cxt_size, "sliding", origin=origin)
            return L, pred
        org = _origin_dev(origin, W.device)
        _check(_anchor_restart_lib().crw_labelprop_propagate_origin_batch(_dev(seed, "seed") if seed is not None else None, _dev(W, "W"),
                                                                          _dev(I, "I", torch.int32), stride, G, T, N, M, knn,
                                                                          int(first_frame), int(cxt_size),
                                                                          _dev(org, "origin", torch.int32), _dev(L, "L"),
                                                                          _dev(pred, "pred"), _stream()),
               "crw_labelprop_propagate_origin_batch")
        return L, pred
    if context == "sliding":
        _check(_sliding_lib().crw_labelprop_propagate_sliding_batch(_dev(seed, "seed") if seed is not None else None, _dev(W, "W"),
                                                                    _dev(I, "I", torch.int32), stride, G, T, N, M, knn,
                                                                    int(first_frame), int(cxt_size), _dev(L, "L"), _dev(pred, "pred"),
                                                                    _stream()), "crw_labelprop_propagate_sliding_batch")
        return L, pred
    _check(_sweep_lib().crw_labelprop_propagate_batch(_dev(seed, "seed") if seed is not None else None, _dev(W, "W"),
                                                      _dev(I, "I", torch.int32), stride, G, T, N, M, knn, int(first_frame),
                                                      int(cxt_size), _dev(L, "L"), _dev(pred, "pred"), _stream()),
           "crw_labelprop_propagate_batch")
    return L, pred


def pelt_rbf(signal, pen, min_size=2, jump=5, gamma=None):
    """HOST function of the library (no GPU): PELT with the RBF kernel cost on a 1-D signal -> sorted breakpoints, the last one
    len(signal) -- pelt.pelt_rbf's arithmetic in C++ (csrc/pelt.cpp)."""
    import numpy as np
    x = np.ascontiguousarray(np.asarray(signal, dtype=np.float64).reshape(-1))
    n = len(x)
    out = np.empty(max(n, 1) + 1, dtype=np.int32)
    cnt = lib().crw_pelt_rbf(ctypes.c_void_p(x.ctypes.data), n, float(pen), int(min_size), int(jump),
                             -1.0 if gamma is None else float(gamma), ctypes.c_void_p(out.ctypes.data), len(out))
    if cnt < 1:
        raise CrwError("crw_pelt_rbf", -cnt, 0)
    return [int(v) for v in out[:cnt]]


def xent_metric(ehat):
    T, N, C = ehat.shape
    out = torch.empty(N, T - 1, device=ehat.device, dtype=torch.float32)
    _check(lib().crw_xent_metric(_dev(ehat, "ehat"), T, N, C, _dev(out, "xent"), _stream()), "crw_xent_metric")
    return out


# ------------------------------------------------------------------------------ evaluation
DT_F32, DT_I8 = 0, 1


class LabelError(CrwError, ValueError):
    """Labels that are no integers in [0, K) survived the mask (dropped[1] of crw_confusion): the caller's data."""

    def __init__(self, invalid, K):
        ValueError.__init__(self, f"{invalid} unmasked label(s) are not integers in [0, {K}) (NaN included)")
        self.what, self.status, self.hip_error, self.invalid = "crw_confusion", CRW_EINVAL, 0, invalid


def _dt(t):
    """The C ABI's dtype code of an operand in one of the kernels' dtypes (an absent one: DT_I8, never read)."""
    return DT_F32 if t is not None and t.dtype == torch.float32 else DT_I8


def _kernel_dtype(t):
    """Labels as one of the kernels' dtypes, the shape kept.  fp32 and int8 pass through; every other dtype becomes fp32, a value
    that fp32 cannot hold exactly becoming NaN (counted as invalid) rather than a neighbouring label."""
    if t.dtype == torch.bool:
        t = t.to(torch.int8)
    elif t.dtype not in (torch.float32, torch.int8):
        f = t.to(torch.float32)
        t = torch.where(f.to(t.dtype) == t, f, torch.full_like(f, float("nan")))
    return t


def _labels(t, name):
    """Flat contiguous labels as one of the kernels' dtypes (`_kernel_dtype`)."""
    return _kernel_dtype(t.reshape(-1)).contiguous()


def _report_args(K, aux, ignore_gt, ignore_pred, ignore_aux, bins=1):
    """The argument checks `confusion`, `horizons` and `calibration` (`bins`: its alone) share -> K as an int."""
    K = int(K)
    if not 2 <= K <= 16:
        raise ValueError(f"K must be in 2 ... 16 (got {K})")
    if not 1 <= bins <= 64:
        raise ValueError(f"bins must be in 1 ... 64 (got {bins})")
    if min(ignore_gt, ignore_pred, ignore_aux) < -1:
        raise ValueError("an ignore label is a class id >= 0, or -1 for none")
    if aux is None and ignore_aux != -1:
        raise ValueError("ignore_aux needs aux")
    return K


def _report_operands(names, ops, aux, size, noun):
    """The operands `names` (`ops`, gt first) and aux (None: absent) of a report are of one `size(t)` and live on one device."""
    ops = [*ops, aux] if aux is not None else ops
    if any(size(t) != size(ops[0]) for t in ops):
        raise ValueError(f"{names}{' and aux' if aux is not None else ''} must hold the same number of {noun} "
                         f"(got {', '.join(str(size(t)) for t in ops)})")
    if any(t.device != ops[0].device for t in ops):
        raise ValueError(f"{names} and aux must live on one device")


def _mask_valid(g, p, aux, K, ignore_gt, ignore_pred, ignore_aux):
    """The mask and validity rule of the report kernels (csrc/labelmap.h) on float64 labels g, p of one shape (aux: as given)
    -> (masked, valid), two bool tensors of that shape."""
    masked = torch.zeros(g.shape, dtype=torch.bool)
    if ignore_gt >= 0:
        masked |= g == ignore_gt
    if ignore_pred >= 0:
        masked |= p == ignore_pred
    if ignore_aux >= 0:
        masked |= aux.reshape(g.shape).to(torch.float64) == ignore_aux
    valid = (g == g.floor()) & (g >= 0) & (g < K) & (p == p.floor()) & (p >= 0) & (p < K)  # NaN fails every comparison
    return masked, valid


def confusion(gt, pred, K, aux=None, ignore_gt=-1, ignore_pred=-1, ignore_aux=-1):
    """Confusion counts of ``pred`` against ``gt`` (any shape, same number of labels) -> (counts [K, K] int64, dropped [2] int64) on
    the inputs' device: counts[g, p] = labels with ground truth g and prediction p; a label is masked (dropped[0]) where
    gt == ignore_gt, pred == ignore_pred or aux == ignore_aux (-1: none), and a surviving label that is no integer in [0, K) is
    counted in dropped[1] and in no bin.  Device tensors: one pass of crw_confusion, nothing synchronises; CPU tensors: the same
    counts from torch.bincount."""
    K = _report_args(K, aux, ignore_gt, ignore_pred, ignore_aux)
    _report_operands("gt, pred", (gt, pred), aux, torch.Tensor.numel, "labels")
    P = gt.numel()
    if not gt.is_cuda:
        return _confusion_cpu(gt, pred, K, aux, ignore_gt, ignore_pred, ignore_aux)
    g, p = _labels(gt, "gt"), _labels(pred, "pred")
    a = _labels(aux, "aux") if aux is not None else None
    if P == 0:  # an empty tensor has no address: nothing to mask
        a, ignore_aux = None, -1
    out = torch.empty(K * K + 2, dtype=torch.int64, device=gt.device)
    nbytes = lib().crw_confusion_ws_bytes(P, K)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=gt.device)
    _check(lib().crw_confusion(_ptr(g), _dt(g), _ptr(p), _dt(p), _ptr(a), _dt(a), P, K, int(ignore_gt), int(ignore_pred),
                               int(ignore_aux), _ptr(out), ctypes.c_void_p(out.data_ptr() + 8 * K * K), _ptr(ws), nbytes, _stream()), "crw_confusion")
    return out[:K * K].view(K, K), out[K * K:]


def _confusion_cpu(gt, pred, K, aux, ignore_gt, ignore_pred, ignore_aux):
    g, p = gt.reshape(-1).to(torch.float64), pred.reshape(-1).to(torch.float64)
    masked, valid = _mask_valid(g, p, aux, K, ignore_gt, ignore_pred, ignore_aux)
    keep = valid & ~masked
    # masked and invalid labels go to two extra bins, like the kernel's: no boolean-indexed copy of the maps
    idx = torch.where(keep, g * K + p, torch.where(masked, float(K * K), float(K * K + 1))).to(torch.int64)
    out = torch.bincount(idx, minlength=K * K + 2)
    return out[:K * K].view(K, K), out[K * K:]


# ------------------------------------------------------------------------------ horizons
HORIZON_STATS = 18           # per class: n_both, n_missing, n_spurious, then 5 numbers for each of top, bottom, count
HORIZON_MAX_ROWS = 32768
HORIZON_QUANTITIES = ("top", "bottom", "count")


def _pitch(t):
    """Elements between the rows of a 2-D window, or None when it has to be copied first."""
    rows, cols = t.shape
    if cols > 1 and t.stride(1) != 1:
        return None
    if rows <= 1:
        return cols
    return t.stride(0) if t.stride(0) >= cols else None


def horizons(gt, pred, K, aux=None, ignore_gt=-1, ignore_pred=-1, ignore_aux=-1, min_run=1, tol=2, want_picks=False, row_slabs=0,
             picks_out=None):
    """Layer horizons and thickness of ``pred`` against ``gt`` ([rows, cols] maps, or ``[rows, a:b]`` column windows of wider ones)
    -> (stats [K, 18] int64, dropped [2] int64[, picks [2, 3, K, cols] int32]) on the inputs' device.  Masks and validity are
    `confusion`'s (``dropped`` equals its).  A run is a maximal stretch of one class down one column of one map and qualifies from
    ``min_run`` rows on; per map (0 gt, 1 pred), class and column, picks = (top: first row of the first qualifying run, bottom: last
    row of the last one, count: pixels in qualifying runs -- the thickness), -1 / -1 / 0 when there is none.  stats[k] = n_both,
    n_missing (gt has k, pred does not), n_spurious, then for top, bottom and count over the n_both columns with d = pred - gt:
    sum |d|, sum d^2, max |d|, columns with |d| <= tol, sum d.  Device tensors: one pass of crw_horizons, nothing synchronises;
    windows that share one pitch are read where they lie (operands of differing pitch are made contiguous first).  ``row_slabs``:
    0 lets the library cut the rows, 1 ... 8 forces the number of slabs.  ``picks_out``: a contiguous int32 [2, 3, K, cols] tensor
    to write the picks into.  CPU tensors: the same integers from vectorised torch ops."""
    K = _report_args(K, aux, ignore_gt, ignore_pred, ignore_aux)
    if gt.dim() != 2:
        raise ValueError(f"gt must be a [rows, cols] map (got shape {tuple(gt.shape)})")
    _report_operands("gt, pred", (gt, pred), aux, lambda t: tuple(t.shape), "labels")
    min_run, tol, row_slabs = int(min_run), int(tol), int(row_slabs)
    if min_run < 1:
        raise ValueError(f"min_run must be at least 1 (got {min_run})")
    if tol < 0:
        raise ValueError(f"tol must be at least 0 (got {tol})")
    if not 0 <= row_slabs <= 8:
        raise ValueError(f"row_slabs must be 0 (the library chooses) or 1 ... 8 (got {row_slabs})")
    rows, cols = gt.shape
    if rows > HORIZON_MAX_ROWS:
        raise ValueError(f"rows must be at most {HORIZON_MAX_ROWS} (got {rows})")
    if picks_out is not None:
        want_picks = True
        if (picks_out.dtype != torch.int32 or tuple(picks_out.shape) != (2, 3, K, cols) or not picks_out.is_contiguous()
                or picks_out.device != gt.device):
            raise ValueError(f"picks_out must be a contiguous int32 [2, 3, {K}, {cols}] tensor on the maps' device")
    if not gt.is_cuda:
        stats, dropped, picks = _horizons_cpu(gt, pred, K, aux, ignore_gt, ignore_pred, ignore_aux, min_run, tol)
        if picks_out is not None:
            picks = picks_out.copy_(picks)
        return (stats, dropped, picks) if want_picks else (stats, dropped)
    # rows stay where they are when the dtype is one of the kernel's and the window's rows are contiguous
    ops = [_kernel_dtype(t) for t in (gt, pred, aux) if t is not None]
    pitches = [_pitch(t) for t in ops]
    if rows * cols == 0:
        ops, ld = ops[:2], cols  # an empty tensor has no address: nothing to mask
        ignore_aux = -1
    elif None in pitches or len(set(pitches)) > 1:
        ops, ld = [t.contiguous() for t in ops], cols
    else:
        ld = pitches[0]
    g, p = ops[0], ops[1]
    a = ops[2] if len(ops) > 2 else None
    out = torch.empty(K * HORIZON_STATS + 2, dtype=torch.int64, device=gt.device)
    picks = None
    if want_picks:
        picks = picks_out if picks_out is not None else torch.empty(2, 3, K, cols, dtype=torch.int32, device=gt.device)
    L = _horizons_lib()
    nbytes = L.crw_horizons_ws_bytes(rows, cols, K)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=gt.device)
    _check(L.crw_horizons(_ptr(g), _dt(g), _ptr(p), _dt(p), _ptr(a), _dt(a),
                          rows, cols, ld, K, int(ignore_gt), int(ignore_pred), int(ignore_aux), min_run, tol, row_slabs,
                          _ptr(picks) if picks is not None and picks.numel() else None, _ptr(out),
                          ctypes.c_void_p(out.data_ptr() + 8 * K * HORIZON_STATS), _ptr(ws), nbytes, _stream()), "crw_horizons")
    stats, dropped = out[:K * HORIZON_STATS].view(K, HORIZON_STATS), out[K * HORIZON_STATS:]
    return (stats, dropped, picks) if want_picks else (stats, dropped)


def _horizons_cpu(gt, pred, K, aux, ignore_gt, ignore_pred, ignore_aux, min_run, tol):
    rows, cols = gt.shape
    g, p = gt.to(torch.float64), pred.to(torch.float64)
    masked, valid = _mask_valid(g, p, aux, K, ignore_gt, ignore_pred, ignore_aux)
    keep = valid & ~masked
    dropped = torch.stack([masked.sum(), (~masked & ~valid).sum()]).to(torch.int64)
    picks = torch.empty(2, 3, K, cols, dtype=torch.int32)
    picks[:, :2], picks[:, 2] = -1, 0
    if rows and cols:
        r = torch.arange(rows)[:, None].expand(rows, cols)
        for m, lab in enumerate((g, p)):
            lab = torch.where(keep, lab, torch.full_like(lab, -1.0)).to(torch.int64)
            change = torch.ones(rows, cols, dtype=torch.bool)
            change[1:] = lab[1:] != lab[:-1]
            start = torch.cummax(torch.where(change, r, torch.zeros_like(r)), 0).values  # first row of the pixel's run
            last = torch.ones(rows, cols, dtype=torch.bool)
            last[:-1] = change[1:]
            end = torch.flip(torch.cummin(torch.flip(torch.where(last, r, torch.full_like(r, rows)), (0,)), 0).values, (0,))
            good = (lab >= 0) & (end - start + 1 >= min_run)  # pixels of qualifying runs
            hot = good[None] & (lab[None] == torch.arange(K)[:, None, None])  # [K, rows, cols]
            n = hot.sum(1)
            top = hot.to(torch.int8).argmax(1)
            bottom = rows - 1 - torch.flip(hot, (1,)).to(torch.int8).argmax(1)
            none = torch.full_like(n, -1)
            picks[m, 0], picks[m, 1], picks[m, 2] = torch.where(n > 0, top, none), torch.where(n > 0, bottom, none), n
    return _horizon_stats(picks, K, tol), dropped, picks


def _horizon_stats(picks, K, tol):
    """stats [K, 18] of picks [2, 3, K, cols] (CPU route)."""
    pk = picks.to(torch.int64)
    hg, hp = pk[0, 2] > 0, pk[1, 2] > 0
    both = hg & hp
    stats = torch.zeros(K, HORIZON_STATS, dtype=torch.int64)
    stats[:, 0], stats[:, 1], stats[:, 2] = both.sum(1), (hg & ~hp).sum(1), (hp & ~hg).sum(1)
    for q in range(3):
        d = torch.where(both, pk[1, q] - pk[0, q], torch.zeros_like(pk[0, q]))
        base = 3 + 5 * q
        stats[:, base] = d.abs().sum(1)
        stats[:, base + 1] = (d * d).sum(1)
        stats[:, base + 2] = d.abs().max(1).values if d.shape[1] else 0
        stats[:, base + 3] = (both & (d.abs() <= tol)).sum(1)
        stats[:, base + 4] = d.sum(1)
    return stats


# ------------------------------------------------------------------------------ confidence
CONF_KINDS = {"maxprob": 0, "margin": 1, "entropy": 2}


def _conf_kind(kind):
    if kind not in CONF_KINDS:
        raise ValueError(f"confidence kind must be one of {', '.join(CONF_KINDS)} (got {kind!r})")
    return CONF_KINDS[kind]


def labelprop_confidence(L, T, N, M, kind="maxprob", first_frame=1):
    """Soft labels L [T*N, M] (`labelprop_gather`'s, a probability row per node) -> conf [N, T] float32, the layout of pred:
    'maxprob' the largest probability, 'margin' the largest minus the second largest (either reads 1 where rounding carried it above 1), 'entropy' 1 + sum p ln p / ln M (0 ln 0 = 0,
    clamped to [0, 1]).  Columns >= first_frame are computed -- and column 0 when first_frame == 1 (the one-hot seed: 1) --, the
    others are 0.  Device tensors: one launch of crw_labelprop_confidence, nothing synchronises; CPU tensors: the same formulas
    in torch, fp32."""
    code = _conf_kind(kind)
    T, N, M, first_frame = int(T), int(N), int(M), int(first_frame)
    if not 2 <= M <= 16:
        raise ValueError(f"M must be in 2 ... 16 (got {M})")
    if T < 1 or N < 1 or not 1 <= first_frame <= T:
        raise ValueError(f"need T, N >= 1 and 1 <= first_frame <= T (got T={T}, N={N}, first_frame={first_frame})")
    if L.numel() != T * N * M or L.dtype != torch.float32:
        raise ValueError(f"L must be float32 [{T * N}, {M}] (got {L.dtype} {tuple(L.shape)})")
    if not L.is_cuda:
        return _labelprop_confidence_cpu(L, T, N, M, kind, first_frame)
    L = L.contiguous()
    conf = (torch.empty if first_frame == 1 else torch.zeros)(N, T, device=L.device, dtype=torch.float32)
    _check(_confidence_lib().crw_labelprop_confidence(_ptr(L), T, N, M, code, first_frame, _ptr(conf), _stream()),
           "crw_labelprop_confidence")
    return conf


def _labelprop_confidence_cpu(L, T, N, M, kind, first_frame):
    p = L.reshape(T, N, M)
    if kind == "maxprob":
        c = p.max(-1).values.clamp(max=1.0)  # rows sum to 1 within rounding only: an entry an ulp above 1 reads 1, like the kernel's
    elif kind == "margin":
        top = torch.topk(p, 2, dim=-1).values
        c = (top[..., 0] - top[..., 1]).clamp(max=1.0)
    else:
        plogp = torch.where(p > 0, p * torch.log(p), torch.zeros_like(p))
        c = (1.0 + plogp.sum(-1) / torch.log(torch.tensor(float(M)))).clamp(0.0, 1.0)
    c = c.t().contiguous()
    if first_frame > 1:
        c[:, :first_frame] = 0
    return c


def merge_confidence(fwd_lab, fwd_conf, rev_lab, rev_conf, out_lab=None, out_conf=None, want_took=False):
    """Per-pixel merge of a forward and a reverse pass by confidence -> (labels, confidence, took | None): the reverse pass's
    label and confidence where rev_conf > fwd_conf strictly, the forward pass's elsewhere -- on a tie, and where either confidence
    is NaN.  Labels: float32 or int8, one dtype for both passes, copied as they are; took (``want_took``): uint8, 1 where the
    reverse pass won.  out_lab / out_conf: contiguous tensors to write into; they may be fwd_lab / fwd_conf (in place).  Device
    tensors: one launch of crw_merge_confidence, nothing synchronises; CPU tensors: torch.where."""
    P = fwd_lab.numel()
    if any(t.numel() != P for t in (fwd_conf, rev_lab, rev_conf)):
        raise ValueError("the two label maps and the two confidence maps must cover the same pixels")
    if fwd_lab.dtype != rev_lab.dtype or fwd_lab.dtype not in (torch.float32, torch.int8):
        raise ValueError(f"labels must be float32 or int8, the same for both passes (got {fwd_lab.dtype}, {rev_lab.dtype})")
    if fwd_conf.dtype != torch.float32 or rev_conf.dtype != torch.float32:
        raise ValueError("confidences must be float32")
    if any(t.device != fwd_lab.device for t in (fwd_conf, rev_lab, rev_conf)):
        raise ValueError("labels and confidences must live on one device")
    if out_lab is None:
        out_lab = torch.empty(fwd_lab.shape, dtype=fwd_lab.dtype, device=fwd_lab.device)
    if out_conf is None:
        out_conf = torch.empty(fwd_lab.shape, dtype=torch.float32, device=fwd_lab.device)
    if (out_lab.numel() != P or out_conf.numel() != P or out_lab.dtype != fwd_lab.dtype or out_conf.dtype != torch.float32
            or not out_lab.is_contiguous() or not out_conf.is_contiguous() or out_lab.device != fwd_lab.device
            or out_conf.device != fwd_lab.device):
        raise ValueError("out_lab / out_conf must be contiguous, of the inputs' size, dtype and device")
    took = torch.empty(fwd_lab.shape, dtype=torch.uint8, device=fwd_lab.device) if want_took else None
    if not fwd_lab.is_cuda:
        take = rev_conf.reshape(-1) > fwd_conf.reshape(-1)
        lab = torch.where(take, rev_lab.reshape(-1), fwd_lab.reshape(-1))
        conf = torch.where(take, rev_conf.reshape(-1), fwd_conf.reshape(-1))
        out_lab.view(-1).copy_(lab)
        out_conf.view(-1).copy_(conf)
        if took is not None:
            took.view(-1).copy_(take)
        return out_lab, out_conf, took
    fl, fc, rl, rc = (t.contiguous() for t in (fwd_lab, fwd_conf, rev_lab, rev_conf))
    _check(_confidence_lib().crw_merge_confidence(_ptr(fl), _ptr(fc), _ptr(rl), _ptr(rc), _dt(fl),
                                                  P, _ptr(out_lab), _ptr(out_conf), _ptr(took) if took is not None else None,
                                                  _stream()), "crw_merge_confidence")
    return out_lab, out_conf, took


def calibration(gt, pred, conf, K, bins=10, aux=None, ignore_gt=-1, ignore_pred=-1, ignore_aux=-1):
    """Reliability histogram of a confidence map -> (counts [bins, 2] int64, conf_sum [bins] float64, dropped [3] int64) on the
    inputs' device.  `confusion`'s operands and its mask and validity rules (dropped[0] masked, dropped[1] invalid labels: the same
    numbers `confusion` gives on the same maps), and the surviving pixels binned by confidence: bin = min(bins - 1,
    floor(conf * bins)) in fp32; counts[b] = (pixels, pixels with gt == pred); conf_sum[b] = the sum of the bin's confidences; a
    surviving pixel whose confidence is NaN or outside [0, 1] is counted in dropped[2] and in no bin.  Device tensors: one pass
    of crw_calibration, nothing synchronises; CPU tensors: the same numbers from torch.bincount, conf_sum in float64."""
    K, bins = int(K), int(bins)
    K = _report_args(K, aux, ignore_gt, ignore_pred, ignore_aux, bins)
    _report_operands("gt, pred, conf", (gt, pred, conf), aux, torch.Tensor.numel, "pixels")
    P = gt.numel()
    if not conf.is_floating_point():
        raise ValueError(f"conf must be a floating-point map (got {conf.dtype})")
    c = conf.reshape(-1).to(torch.float32).contiguous()
    if not gt.is_cuda:
        return _calibration_cpu(gt, pred, c, K, bins, aux, ignore_gt, ignore_pred, ignore_aux)
    g, p = _labels(gt, "gt"), _labels(pred, "pred")
    a = _labels(aux, "aux") if aux is not None else None
    if P == 0:  # an empty tensor has no address: nothing to mask
        a, ignore_aux = None, -1
    out = torch.empty(3 * bins + 3, dtype=torch.int64, device=gt.device)  # counts [bins][2] | conf_sum [bins] (as bits) | dropped [3]
    nbytes = _confidence_lib().crw_calibration_ws_bytes(P, K, bins)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=gt.device)
    base = out.data_ptr()
    _check(lib().crw_calibration(_ptr(g), _dt(g), _ptr(p), _dt(p), _ptr(c), _ptr(a), _dt(a), P, K, bins, int(ignore_gt),
                                 int(ignore_pred), int(ignore_aux), ctypes.c_void_p(base), ctypes.c_void_p(base + 16 * bins),
                                 ctypes.c_void_p(base + 24 * bins), _ptr(ws), nbytes, _stream()), "crw_calibration")
    return out[:2 * bins].view(bins, 2), out[2 * bins:3 * bins].view(torch.float64), out[3 * bins:]


def _calibration_cpu(gt, pred, c, K, bins, aux, ignore_gt, ignore_pred, ignore_aux):
    g, p = gt.reshape(-1).to(torch.float64), pred.reshape(-1).to(torch.float64)
    masked, valid = _mask_valid(g, p, aux, K, ignore_gt, ignore_pred, ignore_aux)
    cvalid = (c >= 0) & (c <= 1)
    binned = ~masked & valid & cvalid
    b = torch.clamp(torch.floor(torch.where(binned, c, torch.zeros_like(c)) * bins), max=bins - 1).to(torch.int64)  # fp32 product
    row = torch.where(masked, bins, torch.where(~valid, bins + 1, torch.where(~cvalid, bins + 2, b)))
    n = torch.bincount(row, minlength=bins + 3)
    ok = torch.bincount(row, weights=(binned & (g == p)).to(torch.float64), minlength=bins + 3).to(torch.int64)
    s = torch.bincount(row, weights=torch.where(binned, c.to(torch.float64), torch.zeros(1, dtype=torch.float64)), minlength=bins + 3)
    return torch.stack([n[:bins], ok[:bins]], 1), s[:bins], n[bins:]


# ------------------------------------------------------------------------------ accuracy against distance
REACH_MAX_GROUPS = 64
REACH_EDGES = (1, 2, 3, 5, 9, 17, 33, 65, 129, 257)  # frame distances {0} {1} {2} {3-4} {5-8} ... {129-256} {257-}
REACH_DIRECTIONS = ("both", "forward", "backward")


def column_groups(cols, labelled, step, edges=None, segments=None, direction="both"):
    """How far is every column of a map from a labelled one?  -> (group uint8 [cols], frames int64 [cols]); host work, no GPU.
    The pixel distance of column c is min |c - l| over the labelled columns l of c's own segment (``segments``: offsets 0 = b_0 <
    ... < b_S = cols, default one segment: an item never reads another item's labels); ``direction`` 'forward' admits only
    l <= c, 'backward' only l >= c.  The frame distance is ceil(pixel distance / step), and the group is the number of ``edges``
    (strictly increasing integers >= 1; default `REACH_EDGES`: the groups {0} {1} {2} {3-4} {5-8} ...) that are <= it.  A column
    with no admissible labelled column has frames = -1 and the last group, len(edges) + 1: len(edges) + 2 groups in all."""
    cols, step = int(cols), int(step)
    if cols < 0:
        raise ValueError(f"cols must be at least 0 (got {cols})")
    if step < 1:
        raise ValueError(f"step must be at least 1 pixel column per frame (got {step})")
    if direction not in REACH_DIRECTIONS:
        raise ValueError(f"direction must be one of {REACH_DIRECTIONS} (got {direction!r})")
    edges = list(REACH_EDGES if edges is None else edges)
    if any(int(e) != e for e in edges) or any(e < 1 for e in edges) or any(b <= a for a, b in zip(edges, edges[1:])):
        raise ValueError(f"edges must be strictly increasing integers >= 1 (got {edges})")
    if len(edges) + 2 > REACH_MAX_GROUPS:
        raise ValueError(f"at most {REACH_MAX_GROUPS - 2} edges: {REACH_MAX_GROUPS} groups with the unreached one (got {len(edges)})")
    segments = [0, cols] if segments is None else [int(b) for b in segments]
    if cols and (len(segments) < 2 or segments[0] != 0 or segments[-1] != cols or any(b <= a for a, b in zip(segments, segments[1:]))):
        raise ValueError(f"segments must be offsets 0 = b_0 < ... < b_S = {cols} (got {segments})")
    if any(int(l) != l for l in labelled):
        raise ValueError("labelled columns must be integers")
    lab = sorted({int(l) for l in labelled})
    if lab and not 0 <= lab[0] <= lab[-1] < cols:
        raise ValueError(f"labelled columns {lab[0]} .. {lab[-1]} lie outside the map's {cols} columns")
    far = torch.iinfo(torch.int64).max
    dist = torch.full((cols,), far, dtype=torch.int64)
    at = torch.tensor(lab, dtype=torch.int64)
    for a, b in zip(segments, segments[1:]):
        own = at[(at >= a) & (at < b)]
        if not own.numel():
            continue
        c = torch.arange(a, b, dtype=torch.int64)
        nxt = torch.searchsorted(own, c)                               # the first labelled column >= c
        ahead = torch.where(nxt < own.numel(), own[nxt.clamp(max=own.numel() - 1)] - c, far)
        prv = torch.searchsorted(own, c, right=True) - 1               # the last labelled column <= c
        behind = torch.where(prv >= 0, c - own[prv.clamp(min=0)], far)
        dist[a:b] = behind if direction == "forward" else ahead if direction == "backward" else torch.minimum(ahead, behind)
    reached = dist != far
    frames = torch.where(reached, (dist + (step - 1)) // step, -1)
    group = torch.bucketize(frames, torch.tensor(edges, dtype=torch.int64), right=True)
    group = torch.where(reached, group, len(edges) + 1).to(torch.uint8)
    return group, frames


def confusion_grouped(gt, pred, K, col_group, groups, conf=None, aux=None, ignore_gt=-1, ignore_pred=-1, ignore_aux=-1):
    """`confusion` per group of columns of [rows, cols] maps (or ``[rows, a:b]`` column windows of wider ones) -> (counts [groups,
    K, K] int64, conf_sum [groups] float64 or None without ``conf``, dropped [4] int64) on the inputs' device.  ``col_group``: uint8
    [cols], the group of every column (`column_groups`); a pixel of a column whose entry is >= ``groups`` is counted in dropped[3]
    and examined no further.  Then `confusion`'s mask (dropped[0]) and validity (dropped[1]) rules; with ``conf``, a float map of
    the same shape, `calibration`'s test: NaN or a value outside [0, 1] is counted in dropped[2].  Every other pixel adds 1 to
    counts[g, gt, pred] and its confidence to conf_sum[g].  Device tensors: one pass of crw_confusion_grouped with a workspace of
    its own, nothing synchronises; windows that share one pitch are read where they lie.  CPU tensors: the same integers from
    torch.bincount, conf_sum in float64."""
    K, groups = _report_args(K, aux, ignore_gt, ignore_pred, ignore_aux), int(groups)
    if not 1 <= groups <= REACH_MAX_GROUPS:
        raise ValueError(f"groups must be in 1 ... {REACH_MAX_GROUPS} (got {groups})")
    if gt.dim() != 2:
        raise ValueError(f"gt must be a [rows, cols] map (got shape {tuple(gt.shape)})")
    maps = (gt, pred) if conf is None else (gt, pred, conf)
    _report_operands("gt, pred" + (", conf" if conf is not None else ""), maps, aux, lambda t: tuple(t.shape), "pixels")
    rows, cols = gt.shape
    if conf is not None and not conf.is_floating_point():
        raise ValueError(f"conf must be a floating-point map (got {conf.dtype})")
    if col_group.dtype != torch.uint8 or tuple(col_group.shape) != (cols,):
        raise ValueError(f"col_group must be uint8 [{cols}] (got {col_group.dtype} {tuple(col_group.shape)})")
    if not gt.is_cuda:
        return _confusion_grouped_cpu(gt, pred, K, col_group.cpu(), groups, conf, aux, ignore_gt, ignore_pred, ignore_aux)
    # rows stay where they are when the dtype is one of the kernel's and the window's rows are contiguous
    ops = [_kernel_dtype(gt), _kernel_dtype(pred)] + ([conf.to(torch.float32)] if conf is not None else [])
    ops += [_kernel_dtype(aux)] if aux is not None else []
    pitches = [_pitch(t) for t in ops]
    if rows * cols == 0:
        ld = cols
    elif None in pitches or len(set(pitches)) > 1:
        ops, ld = [t.contiguous() for t in ops], cols
    else:
        ld = pitches[0]
    g, p = ops[0], ops[1]
    c = ops[2] if conf is not None else None
    a = ops[-1] if aux is not None else None
    if rows * cols == 0:  # an empty tensor has no address: nothing to mask
        a, ignore_aux = None, -1
    grp = col_group.to(gt.device).contiguous()
    n = groups * K * K
    out = torch.empty(n + groups + 4, dtype=torch.int64, device=gt.device)  # counts | conf_sum (as bits) | dropped [4]
    L = _reach_lib()
    nbytes = L.crw_confusion_grouped_ws_bytes(rows, cols, K, groups)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=gt.device)
    base = out.data_ptr()
    _check(L.crw_confusion_grouped(_ptr(g), _dt(g), _ptr(p), _dt(p), _ptr(a), _dt(a), _ptr(c) if c is not None else None, rows, cols, ld,
                                   _ptr(grp), groups, K, int(ignore_gt), int(ignore_pred), int(ignore_aux), ctypes.c_void_p(base),
                                   ctypes.c_void_p(base + 8 * n) if c is not None else None, ctypes.c_void_p(base + 8 * (n + groups)),
                                   _ptr(ws), nbytes, _stream()), "crw_confusion_grouped")
    return out[:n].view(groups, K, K), out[n:n + groups].view(torch.float64) if c is not None else None, out[n + groups:]


def _confusion_grouped_cpu(gt, pred, K, col_group, groups, conf, aux, ignore_gt, ignore_pred, ignore_aux):
    rows, cols = gt.shape
    g, p = gt.reshape(-1).to(torch.float64), pred.reshape(-1).to(torch.float64)
    grp = col_group.to(torch.int64)[None].expand(rows, cols).reshape(-1)
    excluded = grp >= groups
    masked, valid = _mask_valid(g, p, aux, K, ignore_gt, ignore_pred, ignore_aux)
    masked, invalid = masked & ~excluded, ~masked & ~valid & ~excluded
    keep = ~excluded & ~masked & ~invalid
    n = groups * K * K
    if conf is not None:
        c = conf.reshape(-1).to(torch.float32)
        bad = keep & ~((c >= 0) & (c <= 1))
        keep = keep & ~bad
    # the dropped pixels go to four extra bins, like the kernel's: no boolean-indexed copy of the maps
    idx = torch.where(keep, (grp * K + g) * K + p, torch.where(masked, float(n), torch.where(invalid, float(n + 1), float(n + 3))))
    if conf is not None:
        idx = torch.where(bad, float(n + 2), idx)
    idx = idx.to(torch.int64)
    out = torch.bincount(idx, minlength=n + 4)
    conf_sum = None
    if conf is not None:
        zero = torch.zeros(1, dtype=torch.float64)
        conf_sum = torch.bincount(torch.where(keep, grp, 0), weights=torch.where(keep, c.to(torch.float64), zero), minlength=groups)[:groups]
    return out[:n].view(groups, K, K), conf_sum, out[n:]


# ------------------------------------------------------------------------------ dense label maps
DENSE_MAX_SIDE = 1 << 22


def dense_knots(n_in, n_out, flip=False):
    """Knots and weights of `labelmap_dense` along one axis of `n_out` pixels over `n_in` nodes, in integers (the half-pixel
    convention of F.interpolate(mode='bilinear', align_corners=False)) -> (i0 int64 [n_out], i1 int64 [n_out], w float32 [n_out]).
    a = (2x + 1) n_in - n_out over d = 2 n_out: exact knots, and the weight the correctly rounded fp32 quotient of two integers
    fp32 holds exactly (n_out <= 2^22) -- no source coordinate in floating point."""
    x = torch.arange(n_out, dtype=torch.int64)
    if flip:
        x = n_out - 1 - x
    a, d = (2 * x + 1) * n_in - n_out, 2 * n_out
    i0 = torch.div(a.clamp(min=0), d, rounding_mode="floor").clamp(max=n_in - 1)
    inner = (a > 0) & (i0 < n_in - 1)
    i1 = torch.where(inner, i0 + 1, i0)
    w = torch.where(inner, (a - i0 * d).to(torch.float32) / float(d), torch.zeros(n_out))
    return i0, i1, w


def _window(t, name, lead, rows, cols, dtype, device):
    """A [*lead, rows, cols] output of `labelmap_dense` (lead (): a map) or `labelmap_dense_batch` (lead (G,)): contiguous, or a
    column window map[..., a:b] of a wider row-major tensor -> (pitch between rows, elements between maps)."""
    shape = (*lead, rows, cols)
    if tuple(t.shape) != shape or t.dtype != dtype or t.device != device:
        raise ValueError(f"{name} must be {dtype} {list(shape)} on {device} (got {t.dtype} {tuple(t.shape)} on {t.device})")
    if cols > 1 and t.stride(-1) != 1:
        raise ValueError(f"{name} must be contiguous along its columns (stride {t.stride()}): a map, or a column window map[..., a:b]")
    ld = t.stride(-2) if rows > 1 else cols
    if ld < cols:
        raise ValueError(f"{name}: rows overlap (stride {t.stride()})")
    span = (rows - 1) * ld + cols
    map_stride = t.stride(0) if lead and lead[0] > 1 else span
    if map_stride < span:
        raise ValueError(f"{name}: maps overlap (stride {t.stride()})")
    return ld, map_stride


_ARGMAX = object()  # `_labelmap`'s order for the arg-max maps (None is a caller's order like any other: `check_order` refuses it)


def _source(src, lead, N, M, ncols, device, joint):
    """One source of `_labelmap`, (L, T, cols, col0, flip) -> the same with L contiguous and the numbers ints, checked."""
    L, T, cols, col0, flip = src
    T, cols, col0 = int(T), int(cols), int(col0)
    if T < 1 or not 1 <= cols <= DENSE_MAX_SIDE:
        raise ValueError(f"need T, N >= 1 and 1 <= rows, cols <= 2^22 (got T={T}, N={N}, cols={cols})")
    if L.numel() != (lead[0] if lead else 1) * T * N * M or L.dtype != torch.float32:
        raise ValueError(f"L must be float32 {[*lead, T * N, M]} (got {L.dtype} {tuple(L.shape)})")
    if joint and (col0 < 0 or col0 + ncols > cols):
        raise ValueError(f"the window's columns col0 ... col0 + ncols - 1 must lie in the source's 0 ... cols - 1 (got col0={col0}, "
                         f"ncols={ncols}, cols={cols})")
    if L.device != device:
        raise ValueError(f"the two sources must live on one device (got {device} and {L.device})")
    return L.contiguous(), T, cols, col0, bool(flip)


def _labelmap(sources, G, N, M, rows, cols, order, confidence, dtype, out, out_conf, workspace=None):
    """The six label-map functions behind their signatures.  sources: one (L, T, cols, 0, flip), or `labelmap_ordered_joint`'s two
    (L, T, cols, col0, flip) under a window of `cols` columns.  G None: one map, no leading axis, otherwise the `_batch` form;
    order _ARGMAX: `labelmap_dense`, otherwise `labelmap_ordered`'s decode under it (`workspace`: its alone)."""
    joint = len(sources) == 2
    code = -1 if confidence is None else _conf_kind(confidence)
    N, M, rows, cols = int(N), int(M), int(rows), int(cols)
    lead = () if G is None else (int(G),)
    if lead and not 1 <= lead[0] <= 65535:
        raise ValueError(f"G must be in 1 ... 65535 (got {lead[0]})")
    if not 2 <= M <= 16:
        raise ValueError(f"M must be in 2 ... 16 (got {M})")
    if order is not _ARGMAX:
        order = check_order(order, M)
    if joint and confidence is None:
        raise ValueError("the joint map needs a confidence kind: it takes, per pixel, the surer source's row")
    if N < 1 or not 1 <= rows <= DENSE_MAX_SIDE or not 1 <= cols <= DENSE_MAX_SIDE:
        raise ValueError(f"need T, N >= 1 and 1 <= rows, cols <= 2^22 (got T={sources[0][1]}, N={N}, rows={rows}, cols={cols})")
    device = sources[0][0].device
    sources = [_source(src, lead, N, M, cols, device, joint) for src in sources]
    if dtype not in (torch.float32, torch.int8):
        raise ValueError(f"dtype must be torch.float32 or torch.int8 (got {dtype})")
    if out_conf is not None and confidence is None:
        raise ValueError("out_conf needs a confidence kind")
    if out is None:
        out = torch.empty(*lead, rows, cols, dtype=dtype, device=device)
    if out_conf is None and confidence is not None:
        out_conf = torch.empty(*lead, rows, cols, dtype=torch.float32, device=device)
    ld, map_stride = _window(out, "out", lead, rows, cols, dtype, device)
    if out_conf is not None:
        cld, cstride = _window(out_conf, "out_conf", lead, rows, cols, torch.float32, device)
        if cld != ld and rows > 1:
            raise ValueError(f"out and out_conf must share one pitch (got {out.stride(-2)} and {out_conf.stride(-2)})")
        if cstride != map_stride:  # (equal by construction for one map)
            raise ValueError(f"out and out_conf must share one map stride (got {out.stride(0)} and {out_conf.stride(0)})")
    if device.type != "cuda":
        maps, confs = (out, out_conf) if lead else (out[None], None if out_conf is None else out_conf[None])
        for g in range(lead[0] if lead else 1):
            slices = [(L.view(-1, T * N, M)[g], T, width, col0, flip) for L, T, width, col0, flip in sources]
            if joint:
                lab, conf = _labelmap_joint_cpu(*slices, N, M, rows, cols, order, confidence)
            elif order is _ARGMAX:
                lab, conf = _labelmap_dense_cpu(*slices[0][:2], N, M, rows, cols, confidence, slices[0][4])
            else:
                lab, conf = _labelmap_ordered_cpu(*slices[0][:2], N, M, rows, cols, order, confidence, slices[0][4])
            maps[g].copy_(lab.to(dtype))
            if confs is not None:
                confs[g].copy_(conf)
        return out, out_conf
    # the C signatures: the source(s), [G,] geometry, [order, S,] windows, [map_stride,] [workspace, its bytes,] stream
    L, T, _, _, flip = sources[0]
    geometry = (T, N, M, rows, cols, int(flip))
    windows = (code, _ptr(out), _dt(out), _ptr(out_conf), ld)
    if order is _ARGMAX:
        if lead:
            _check(_dense_batch_lib().crw_labelmap_dense_batch(_ptr(L), *lead, *geometry, *windows, map_stride, _stream()),
                   "crw_labelmap_dense_batch")
        else:
            _check(_dense_lib().crw_labelmap_dense(_ptr(L), *geometry, *windows, _stream()), "crw_labelmap_dense")
        return out, out_conf
    clib = _joint_lib() if joint else _ordered_lib()
    if workspace is None:
        workspace = torch.empty(clib.crw_labelmap_ordered_workspace(*lead or (1,), rows, cols), dtype=torch.uint8, device=device)
    elif workspace.device != device or not workspace.is_contiguous():
        raise ValueError(f"workspace must be a contiguous tensor on {device} (got {workspace.device})")
    decode = ((ctypes.c_int * len(order))(*order), len(order))
    tail = (_ptr(workspace), workspace.numel() * workspace.element_size(), _stream())
    if joint:
        both = [v for Lk, Tk, width, col0, flipk in sources for v in (_ptr(Lk), Tk, width, col0, int(flipk))]
        if lead:
            _check(clib.crw_labelmap_ordered_joint_batch(*both, *lead, N, M, rows, cols, *decode, *windows, map_stride, *tail),
                   "crw_labelmap_ordered_joint_batch")
        else:
            _check(clib.crw_labelmap_ordered_joint(*both, N, M, rows, cols, *decode, *windows, *tail), "crw_labelmap_ordered_joint")
    elif lead:
        _check(clib.crw_labelmap_ordered_batch(_ptr(L), *lead, *geometry, *decode, *windows, map_stride, *tail), "crw_labelmap_ordered_batch")
    else:
        _check(clib.crw_labelmap_ordered(_ptr(L), *geometry, *decode, *windows, *tail), "crw_labelmap_ordered")
    return out, out_conf


def labelmap_dense(L, T, N, M, rows, cols, *, confidence=None, flip=False, dtype=torch.float32, out=None, out_conf=None):
    """Soft labels L [T*N, M] (a probability row per node, node (n, t) in row t*N + n) -> (labels [rows, cols], conf | None): the
    rows interpolated bilinearly to pixels -- image rows along the nodes n, columns along the frames t, half-pixel convention, the
    knots and weights of `dense_knots` -- and arg-maxed AFTER that (the lowest class on exact equality).  confidence: None, or a
    kind of `labelprop_confidence` -- conf is then float32 [rows, cols], that formula on the interpolated row.  flip: the map
    mirrored along its columns (the reverse pass's).  dtype: float32 (what `segment` returns) or int8 (what the drivers save).
    out / out_conf: tensors to write into; they may be column windows of wider maps (``map[:, a:b]``, one pitch for both), anything
    else that is not contiguous raises ValueError.  Device tensors: one launch of crw_labelmap_dense, nothing synchronises, the
    interpolated probabilities are never written; CPU tensors: the same integer knots, fp32 weights, arithmetic and tie rule in
    torch."""
    return _labelmap([(L, T, cols, 0, flip)], None, N, M, rows, cols, _ARGMAX, confidence, dtype, out, out_conf)


def labelmap_dense_batch(L, G, T, N, M, rows, cols, *, confidence=None, flip=False, dtype=torch.int8, out=None, out_conf=None):
    """`labelmap_dense` for the G configurations of a sweep's pass at once: L [G, T*N, M] (`labelprop_propagate_batch`'s soft
    labels) -> (labels [G, rows, cols], conf | None); slice g is `labelmap_dense(L[g], ...)` bit for bit, labels and confidence.
    dtype: int8 (what `segment_sweep` keeps) or float32.  out / out_conf: [G, rows, cols] tensors to write into; they may be the
    column windows ``maps[:, :, a:b]`` of wider [G, rows, width] tensors (one pitch and one map stride for both), anything else
    that is not contiguous raises ValueError.  Device tensors: ONE launch of crw_labelmap_dense_batch, nothing synchronises; CPU
    tensors: a loop of `labelmap_dense`'s CPU route over the configurations."""
    return _labelmap([(L, T, cols, 0, flip)], G, N, M, rows, cols, _ARGMAX, confidence, dtype, out, out_conf)


def _interpolated(L, T, N, M, rows, cols, flip):
    """The interpolated probabilities v [rows, cols, M] of the CPU route: `dense_knots`' knots and weights, fp32."""
    i0, i1, wr = dense_knots(N, rows)
    j0, j1, wc = dense_knots(T, cols, flip)
    P = L.view(T, N, M)
    wr, wc = wr[:, None, None], wc[None, :, None]
    corner = lambda i, j: P[j[None, :], i[:, None]]  # [rows, cols, M]
    top = (1 - wc) * corner(i0, j0) + wc * corner(i0, j1)
    bot = (1 - wc) * corner(i1, j0) + wc * corner(i1, j1)
    return (1 - wr) * top + wr * bot


def _interpolated_confidence(v, confidence):
    """conf [rows, cols] of v [rows, cols, M] (`labelprop_confidence`'s formulas), or None without a kind."""
    if confidence is None:
        return None
    rows, cols, M = v.shape
    return _labelprop_confidence_cpu(v.permute(1, 0, 2).reshape(rows * cols, M), cols, rows, M, confidence, 1)


def _labelmap_dense_cpu(L, T, N, M, rows, cols, confidence, flip):
    v = _interpolated(L, T, N, M, rows, cols, flip)
    return v.argmax(-1), _interpolated_confidence(v, confidence)  # the first of equal maxima: the lowest class


# ------------------------------------------------------------------------------ depth-ordered label maps
def check_order(order, M):
    """`order` of `labelmap_ordered` -> a list of S distinct classes of 0 ... M-1, 2 <= S <= M (ValueError otherwise)."""
    try:
        out = [int(k) for k in order]
    except TypeError:
        raise ValueError(f"order must be a sequence of classes, top to bottom (got {order!r})") from None
    if not 2 <= len(out) <= M:
        raise ValueError(f"order must name 2 ... M = {M} classes (got {len(out)}: {out})")
    if len(set(out)) != len(out) or min(out) < 0 or max(out) >= M:
        raise ValueError(f"order must hold distinct classes of 0 ... {M - 1} (got {out})")
    return out


def labelmap_ordered_workspace(G, rows, cols):
    """Bytes of back-pointer workspace `labelmap_ordered` (G = 1) / `labelmap_ordered_batch` need on the device."""
    return _ordered_lib().crw_labelmap_ordered_workspace(int(G), int(rows), int(cols))


def labelmap_ordered(L, T, N, M, rows, cols, order, *, confidence=None, flip=False, dtype=torch.float32, out=None, out_conf=None,
                     workspace=None):
    """`labelmap_dense`'s interpolated probabilities decoded under a layer order -> (labels [rows, cols], conf | None).
    order: S distinct classes of 0 ... M-1, top to bottom, 2 <= S <= M; a class outside it is never written.  Per pixel column, the
    labelling whose position in `order` never steps back down the column and whose summed probability is the largest: in fp32,
    D[0][s] = e[0][s], D[r][s] = e[r][s] + max_{s' <= s} D[r-1][s'] with e[r][s] the interpolated probability of class order[s],
    the LOWEST s' on equal prefix maxima, the LOWEST s on equal final scores.  A column may start and end in any state; a layer may
    be absent.  conf: `labelmap_dense`'s, bit for bit -- the confidence of the interpolated row, whatever the decode picked.
    flip / dtype / out / out_conf: as for `labelmap_dense`.  workspace: a device tensor of at least
    `labelmap_ordered_workspace(1, rows, cols)` bytes for the back-pointers (default: allocated per call; a short one raises
    CrwError CRW_EWORKSPACE).  Device tensors: one launch of crw_labelmap_ordered, nothing synchronises; CPU tensors: the same
    recurrence and tie rules in torch (a loop over rows, tensors over [S, cols]) on the CPU route's own interpolated values."""
    return _labelmap([(L, T, cols, 0, flip)], None, N, M, rows, cols, order, confidence, dtype, out, out_conf, workspace)


def labelmap_ordered_batch(L, G, T, N, M, rows, cols, order, *, confidence=None, flip=False, dtype=torch.int8, out=None,
                           out_conf=None, workspace=None):
    """`labelmap_ordered` for the G configurations of a sweep's pass at once (one `order` for all): L [G, T*N, M] -> (labels
    [G, rows, cols], conf | None); slice g is `labelmap_ordered(L[g], ...)` bit for bit.  out / out_conf / dtype: as for
    `labelmap_dense_batch`; workspace: at least `labelmap_ordered_workspace(G, rows, cols)` bytes.  Device tensors: ONE launch of
    crw_labelmap_ordered_batch; CPU tensors: a loop of `labelmap_ordered`'s CPU route."""
    return _labelmap([(L, T, cols, 0, flip)], G, N, M, rows, cols, order, confidence, dtype, out, out_conf, workspace)


def _ordered_decode(v, order):
    """The recurrence, tie rules and back-track of `labelmap_ordered` on interpolated values v [rows, cols, M] -> labels int64
    [rows, cols].  The ONE text of the CPU routes: `labelmap_ordered`'s and `labelmap_ordered_joint`'s."""
    rows, cols, _ = v.shape
    S = len(order)
    e = v[:, :, order].permute(0, 2, 1).contiguous()  # [rows, S, cols]
    D = e[0].clone()
    new = torch.ones(rows, S, cols, dtype=torch.bool)  # new[r, s]: state s is a new prefix maximum of D[r-1] (strict >)
    for r in range(1, rows):
        best = torch.cummax(D, 0).values
        new[r, 1:] = D[1:] > best[:-1]
        D = e[r] + best
    idx = torch.arange(S)[:, None]
    state = torch.where(D == D.max(0).values, idx, S).min(0).values  # the lowest state among equal maxima
    states = torch.empty(rows, cols, dtype=torch.int64)
    for r in range(rows - 1, 0, -1):
        states[r] = state
        state = torch.where(new[r] & (idx <= state[None]), idx, 0).max(0).values  # the highest new maximum <= state
    states[0] = state
    return torch.tensor(order)[states]


def _labelmap_ordered_cpu(L, T, N, M, rows, cols, order, confidence, flip):
    v = _interpolated(L, T, N, M, rows, cols, flip)  # `_labelmap_dense_cpu`'s values
    return _ordered_decode(v, order), _interpolated_confidence(v, confidence)


# ------------------------------------------------------------------------------ joint ordered label maps
def labelmap_ordered_joint(a, b, N, M, rows, ncols, order, *, confidence, dtype=torch.float32, out=None, out_conf=None,
                           workspace=None):
    """An order-preserving merge of two passes: `labelmap_ordered`'s decode over, per pixel, the interpolated row of the SURER
    source -> (labels [rows, ncols], conf [rows, ncols]).  a, b: the sources, each (L, T, cols, col0, flip) -- soft labels L
    [T*N, M] under a map of `cols` columns, of which the window is the columns col0 ... col0 + ncols - 1, mirrored with flip as
    `labelmap_dense` mirrors them (N, M, rows and `order` are shared; the two may be one tensor).  Per pixel, with v_k and conf_k
    what `labelmap_dense(L_k, T_k, N, M, rows, cols_k, confidence=confidence, flip=flip_k)` computes at column col0_k + x: b's row
    where conf_b > conf_a strictly, a's elsewhere (a tie, a NaN) -- `merge_confidence`'s rule --, then ONE dynamic programme down
    the column.  The labels never step back in `order` down a column, which a per-pixel merge of two ordered maps cannot promise;
    conf is `merge_confidence`'s of the two dense confidence maps, bit for bit.  confidence: the kind, mandatory.  dtype / out /
    out_conf / workspace (`labelmap_ordered_workspace(1, rows, ncols)` bytes): as for `labelmap_ordered`.  Device tensors: one
    launch of crw_labelmap_ordered_joint, nothing synchronises; CPU tensors: the same selection and `labelmap_ordered`'s CPU
    recurrence in torch."""
    return _labelmap([a, b], None, N, M, rows, ncols, order, confidence, dtype, out, out_conf, workspace)


def labelmap_ordered_joint_batch(a, b, G, N, M, rows, ncols, order, *, confidence, dtype=torch.int8, out=None, out_conf=None,
                                 workspace=None):
    """`labelmap_ordered_joint` for the G configurations of a sweep at once: each source's L is [G, T*N, M] -> (labels
    [G, rows, ncols], conf); slice g is `labelmap_ordered_joint` on the sources' slices g, bit for bit.  out / out_conf / dtype /
    workspace: as for `labelmap_ordered_batch`.  Device tensors: ONE launch of crw_labelmap_ordered_joint_batch; CPU tensors: a
    loop of the CPU route."""
    return _labelmap([a, b], G, N, M, rows, ncols, order, confidence, dtype, out, out_conf, workspace)


def _labelmap_joint_cpu(a, b, N, M, rows, ncols, order, confidence):
    vs, confs = [], []
    for L, T, cols, col0, flip in (a, b):
        v = _interpolated(L, T, N, M, rows, cols, flip)[:, col0:col0 + ncols]  # `_labelmap_dense_cpu`'s values in the window
        vs.append(v)
        confs.append(_interpolated_confidence(v, confidence))
    took = confs[1] > confs[0]  # `merge_confidence`'s comparison
    return _ordered_decode(torch.where(took[:, :, None], vs[1], vs[0]), order), torch.where(took, confs[1], confs[0])


# ------------------------------------------------------------------------------ posterior of the ordered label maps
POSTERIOR_FLOOR = 1e-4                      # the default floor under the evidence (seed frames are one-hot: L holds exact zeros)
POSTERIOR_FLOOR_RANGE = (2.0 ** -20, 0.25)


def check_floor(floor):
    """`floor` of the posterior calls -> a float in 2^-20 ... 0.25 (ValueError otherwise, a NaN included)."""
    floor = float(floor)
    if not POSTERIOR_FLOOR_RANGE[0] <= floor <= POSTERIOR_FLOOR_RANGE[1]:
        raise ValueError(f"floor must lie in 2^-20 ... 0.25 (got {floor})")
    return floor


def labelmap_posterior_workspace(rows, cols, S):
    """Bytes of workspace `labelmap_ordered_posterior` / `labelmap_ordered_joint_posterior` need on the device: the normalised
    forward messages, 4 * rows * S * (cols rounded up to 64)."""
    return _posterior_lib().crw_labelmap_posterior_workspace(int(rows), int(cols), int(S))


def labelmap_posterior_workspace_batch(G, rows, cols, S):
    """Bytes of workspace ONE launch of `labelmap_ordered_posterior_batch` / `labelmap_ordered_joint_posterior_batch` needs for G
    configurations: G times `labelmap_posterior_workspace(rows, cols, S)`."""
    return _posterior_batch_lib().crw_labelmap_posterior_workspace_batch(int(G), int(rows), int(cols), int(S))


POSTERIOR_BATCH_WS = 2 << 30  # bytes of workspace the batched posterior calls allocate at most (CRW_POSTERIOR_BATCH_WS, read per call)


def posterior_batch_chunks(G, rows, cols, S):
    """How the batched posterior calls issue G configurations when they allocate their own workspace: the configurations per
    launch, as few launches as fit CRW_POSTERIOR_BATCH_WS bytes (default 2 GiB) of workspace, at least one configuration each."""
    one = labelmap_posterior_workspace(rows, cols, S)
    text = os.environ.get("CRW_POSTERIOR_BATCH_WS", str(POSTERIOR_BATCH_WS))
    try:
        cap = int(text)
    except ValueError:
        cap = 0
    if cap < 1:
        raise ValueError(f"CRW_POSTERIOR_BATCH_WS must be a positive number of bytes (got {text!r})")
    per = min(int(G), max(1, cap // one)) if one else int(G)
    return [min(per, int(G) - g) for g in range(0, int(G), per)]


def _hz_window(out_hz, lead, S, cols, device):
    """out_hz [*lead, 3, S-1, cols]: contiguous, or the column window hz[..., a:b] of a wider tensor -> (pitch between its rows,
    elements between configurations)."""
    shape = (*lead, 3, S - 1, cols)
    if tuple(out_hz.shape) != shape or out_hz.dtype != torch.float32 or out_hz.device != device:
        raise ValueError(f"out_hz must be float32 {list(shape)} on {device} (got {out_hz.dtype} {tuple(out_hz.shape)} on {out_hz.device})")
    hz_ld = out_hz.stride(-2) if S > 2 else (out_hz.stride(-3) if out_hz.stride(-3) >= cols else cols)
    if (cols > 1 and out_hz.stride(-1) != 1) or hz_ld < cols or out_hz.stride(-3) != (S - 1) * hz_ld:
        raise ValueError(f"out_hz must be a {list(shape)} tensor or the column window hz[..., a:b] of a wider one (stride {out_hz.stride()})")
    hz_stride = out_hz.stride(0) if lead and lead[0] > 1 else 3 * (S - 1) * hz_ld
    if hz_stride < 3 * (S - 1) * hz_ld:
        raise ValueError(f"out_hz: configurations overlap (stride {out_hz.stride()})")
    return hz_ld, hz_stride


def _posterior(sources, G, N, M, rows, cols, order, labels, confidence, floor, out, out_hz, workspace):
    """The four posterior functions behind their signatures; sources as for `_labelmap`.  G None: one map, no leading axis,
    otherwise the `_batch` form."""
    joint = len(sources) == 2
    N, M, rows, cols = int(N), int(M), int(rows), int(cols)
    lead = () if G is None else (int(G),)
    if lead and not 1 <= lead[0] <= 65535:
        raise ValueError(f"G must be in 1 ... 65535 (got {lead[0]})")
    if not 2 <= M <= 16:
        raise ValueError(f"M must be in 2 ... 16 (got {M})")
    order = check_order(order, M)
    S = len(order)
    floor = check_floor(floor)
    if joint and confidence is None:
        raise ValueError("the joint posterior needs the confidence kind the joint map was decoded with")
    code = _conf_kind(confidence) if joint else -1
    if N < 1 or not 1 <= rows <= DENSE_MAX_SIDE or not 1 <= cols <= DENSE_MAX_SIDE:
        raise ValueError(f"need T, N >= 1 and 1 <= rows, cols <= 2^22 (got T={sources[0][1]}, N={N}, rows={rows}, cols={cols})")
    device = sources[0][0].device
    sources = [_source(src, lead, N, M, cols, device, joint) for src in sources]
    if labels.dtype not in (torch.float32, torch.int8):
        raise ValueError(f"labels must be torch.float32 or torch.int8 (got {labels.dtype})")
    ld, map_stride = _window(labels, "labels", lead, rows, cols, labels.dtype, device)
    if out is None:  # the labels' pitch (and map stride), which the window of `post` shares
        span = (rows - 1) * ld + cols
        out = torch.empty(((lead[0] - 1) * map_stride if lead else 0) + span, dtype=torch.float32, device=device)
        out = out.as_strided((*lead, rows, cols), (*((map_stride,) if lead else ()), ld, 1))
    old, ostride = _window(out, "out", lead, rows, cols, torch.float32, device)
    if old != ld and rows > 1:
        raise ValueError(f"labels and out must share one pitch (got {labels.stride(-2)} and {out.stride(-2)})")
    if ostride != map_stride:  # (equal by construction for one map)
        raise ValueError(f"labels and out must share one map stride (got {labels.stride(0)} and {out.stride(0)})")
    if out_hz is None:
        out_hz = torch.empty(*lead, 3, S - 1, cols, dtype=torch.float32, device=device)
    hz_ld, hz_stride = _hz_window(out_hz, lead, S, cols, device)
    if device.type != "cuda":
        posts, hzs, labs = (out, out_hz, labels) if lead else (out[None], out_hz[None], labels[None])
        for g in range(lead[0] if lead else 1):
            slices = [(L.view(-1, T * N, M)[g], T, width, col0, flip) for L, T, width, col0, flip in sources]
            if joint:
                vs = [_interpolated(L, T, N, M, rows, width, flip)[:, col0:col0 + cols] for L, T, width, col0, flip in slices]
                confs = [_interpolated_confidence(v, confidence) for v in vs]
                v = torch.where((confs[1] > confs[0])[:, :, None], vs[1], vs[0])  # `_labelmap_joint_cpu`'s selection
            else:
                L, T, _, _, flip = slices[0]
                v = _interpolated(L, T, N, M, rows, cols, flip)
            post, hz = _ordered_posterior(v, order, labs[g], floor)
            posts[g].copy_(post), hzs[g].copy_(hz)
        return out, out_hz
    clib = _posterior_batch_lib() if lead else _posterior_lib()
    if workspace is not None and (workspace.device != device or not workspace.is_contiguous()):
        raise ValueError(f"workspace must be a contiguous tensor on {device} (got {workspace.device})")
    decode = ((ctypes.c_int * S)(*order), S)
    if not lead:
        if workspace is None:
            workspace = torch.empty(clib.crw_labelmap_posterior_workspace(rows, cols, S), dtype=torch.uint8, device=device)
        tail = (floor, _ptr(labels), _dt(labels), ld, _ptr(out), _ptr(out_hz), hz_ld, _ptr(workspace),
                workspace.numel() * workspace.element_size(), _stream())
        if joint:
            both = [v for Lk, Tk, width, col0, flipk in sources for v in (_ptr(Lk), Tk, width, col0, int(flipk))]
            _check(clib.crw_labelmap_ordered_joint_posterior(*both, N, M, rows, cols, *decode, code, *tail), "crw_labelmap_ordered_joint_posterior")
        else:
            L, T, _, _, flip = sources[0]
            _check(clib.crw_labelmap_ordered_posterior(_ptr(L), T, N, M, rows, cols, int(flip), *decode, *tail), "crw_labelmap_ordered_posterior")
        return out, out_hz
    # the G configurations: one launch over the caller's workspace, or as few as fit CRW_POSTERIOR_BATCH_WS bytes of our own
    chunks = [lead[0]] if workspace is not None else posterior_batch_chunks(lead[0], rows, cols, S)
    if workspace is None:
        workspace = torch.empty(clib.crw_labelmap_posterior_workspace_batch(chunks[0], rows, cols, S), dtype=torch.uint8, device=device)
    g0 = 0
    for n in chunks:  # (a slice of n configurations is the batch call on the operands' slices: the strides stay)
        sl = slice(g0, g0 + n)
        tail = (floor, _ptr(labels[sl]), _dt(labels), ld, map_stride, _ptr(out[sl]), _ptr(out_hz[sl]), hz_ld, hz_stride, _ptr(workspace),
                workspace.numel() * workspace.element_size(), _stream())
        if joint:
            both = [v for Lk, Tk, width, col0, flipk in sources for v in (_ptr(Lk.view(lead[0], -1)[sl]), Tk, width, col0, int(flipk))]
            _check(clib.crw_labelmap_ordered_joint_posterior_batch(*both, n, N, M, rows, cols, *decode, code, *tail),
                   "crw_labelmap_ordered_joint_posterior_batch")
        else:
            L, T, _, _, flip = sources[0]
            _check(clib.crw_labelmap_ordered_posterior_batch(_ptr(L.view(lead[0], -1)[sl]), n, T, N, M, rows, cols, int(flip), *decode, *tail),
                   "crw_labelmap_ordered_posterior_batch")
        g0 += n
    return out, out_hz


def labelmap_ordered_posterior(L, T, N, M, rows, cols, order, labels, *, flip=False, floor=POSTERIOR_FLOOR, out=None, out_hz=None,
                               workspace=None):
    """The confidence that belongs to `labelmap_ordered`'s map -> (post float32 [rows, cols], hz float32 [3, S-1, cols]).  Over the
    monotone paths of a pixel column (positions in `order` that never step back; any start, any end), with the evidence the decode
    adds up -- the interpolated probabilities e[r][s], here floored, f = max(e, floor) with 2^-20 <= floor <= 0.25, and MULTIPLIED
    down the path -- as independent per-row evidence: post[r][c] is the posterior probability of the label that `labels` holds at
    (r, c) (0 for a label outside `order`), and for the boundary B_k of layer k = 1 ... S-1 (the first row at position >= k, `rows`
    if none) hz[0][k-1] is the pick b^_k read from `labels`, hz[1][k-1] its posterior mean E[B_k] and hz[2][k-1] the error bar of
    the pick, sqrt(E[(B_k - b^_k)^2]).  labels: the map a decode wrote, int8 or float32 [rows, cols], an INPUT (it may be a column
    window of a wider map).  out / out_hz: tensors to write into; out shares the labels' pitch, out_hz may be the window
    ``hz[:, :, a:b]`` of a [3, S-1, width] tensor.  workspace: at least `labelmap_posterior_workspace(rows, cols, S)` bytes
    (default: allocated per call).  Device tensors: one launch of crw_labelmap_ordered_posterior (a normalised forward-backward in
    fp32, include/crw_hip.h), nothing synchronises; CPU tensors: the same recurrences in torch on the CPU route's interpolated
    values."""
    return _posterior([(L, T, cols, 0, flip)], None, N, M, rows, cols, order, labels, None, floor, out, out_hz, workspace)


def labelmap_ordered_joint_posterior(a, b, N, M, rows, ncols, order, labels, *, confidence, floor=POSTERIOR_FLOOR, out=None,
                                     out_hz=None, workspace=None):
    """`labelmap_ordered_posterior` over the evidence `labelmap_ordered_joint` decodes: per pixel the interpolated row of the surer
    of the two sources a, b (each (L, T, cols, col0, flip); `confidence`: the kind, mandatory) -> (post [rows, ncols], hz
    [3, S-1, ncols]).  With both sources the same tensor and geometry it equals `labelmap_ordered_posterior` bit for bit."""
    return _posterior([a, b], None, N, M, rows, ncols, order, labels, confidence, floor, out, out_hz, workspace)


def labelmap_ordered_posterior_batch(L, G, T, N, M, rows, cols, order, labels, *, flip=False, floor=POSTERIOR_FLOOR, out=None, out_hz=None,
                                     workspace=None):
    """`labelmap_ordered_posterior` for the G configurations of a sweep's pass at once (one order, one floor, one geometry): L
    [G, T*N, M], labels [G, rows, cols] (int8 as `labelmap_ordered_batch` writes them, or float32; they may be the column windows
    ``maps[:, :, a:b]`` of wider maps) -> (post float32 [G, rows, cols], hz float32 [G, 3, S-1, cols]); slice g is
    `labelmap_ordered_posterior(L[g], ..., labels[g])` bit for bit.  out shares the labels' pitch and map stride; out_hz may be the
    window ``hz[:, :, :, a:b]`` of a [G, 3, S-1, width] tensor.  workspace: at least `labelmap_posterior_workspace_batch(G, rows,
    cols, S)` bytes, then ONE launch of crw_labelmap_ordered_posterior_batch (the configuration is a grid dimension of the one-map
    kernel).  Without it the call allocates at most CRW_POSTERIOR_BATCH_WS bytes (read per call, default 2 GiB; a sweep's window of
    410 x 3200 x 4 is 21 MB per configuration) and issues the configurations in as few launches as fit (`posterior_batch_chunks`),
    at least one configuration each; the outputs do not depend on the split.  CPU tensors: a loop of the one-map CPU route."""
    return _posterior([(L, T, cols, 0, flip)], G, N, M, rows, cols, order, labels, None, floor, out, out_hz, workspace)


def labelmap_ordered_joint_posterior_batch(a, b, G, N, M, rows, ncols, order, labels, *, confidence, floor=POSTERIOR_FLOOR, out=None,
                                           out_hz=None, workspace=None):
    """`labelmap_ordered_joint_posterior` for the G configurations of a sweep at once: each source's L is [G, T*N, M], labels
    [G, rows, ncols] -> (post [G, rows, ncols], hz [G, 3, S-1, ncols]); slice g is the one-map call on the sources' slices g, bit
    for bit.  out / out_hz / workspace and the split over launches: as for `labelmap_ordered_posterior_batch`."""
    return _posterior([a, b], G, N, M, rows, ncols, order, labels, confidence, floor, out, out_hz, workspace)


def _ordered_posterior(v, order, labels, floor):
    """The recurrences of crw_labelmap_ordered_posterior (include/crw_hip.h) in fp32 torch on interpolated values v [rows, cols, M]
    and a label map [rows, cols] -> (post [rows, cols], hz [3, S-1, cols]).  The ONE text of the two CPU routes."""
    rows, cols, _ = v.shape
    S = len(order)
    f = v[:, :, order].permute(0, 2, 1).clamp(min=floor).contiguous()  # [rows, S, cols]
    A = torch.empty(rows, S, cols)
    prev = torch.zeros(S, cols)
    prev[0] = 1
    for r in range(rows):
        a = f[r] * prev.cumsum(0)
        prev = A[r] = a * (1 / a.sum(0))
    lab = labels.to(torch.float32)
    pos = torch.full((rows, cols), -1, dtype=torch.int64)
    for s, k in enumerate(order):
        pos[lab == k] = s
    ks = torch.arange(1, S)[:, None, None]
    reached = pos[None] >= ks  # [S-1, rows, cols]
    pick = torch.where(reached.any(1), reached.to(torch.int8).argmax(1), rows).to(torch.float32)  # the first row at position >= k
    b = torch.ones(S, cols)
    m1, m2 = torch.zeros(S - 1, cols), torch.zeros(S - 1, cols)
    post = torch.empty(rows, cols)
    for r in range(rows - 1, -1, -1):
        g = A[r] * b
        Z = g.sum(0)
        inv = torch.where(Z >= 2.0 ** -126, 1 / Z, torch.zeros(()))
        g = g * inv
        post[r] = torch.where(pos[r] >= 0, g.gather(0, pos[r].clamp(min=0)[None])[0], torch.zeros(())).clamp(max=1)
        p = A[r].cumsum(0)[:-1] * b[1:] * inv  # the boundary enters at row r + 1
        m1 += (r + 1) * p
        m2 += (r + 1 - pick) ** 2 * p
        b = (f[r] * (b * (1 / b[0]))).flip(0).cumsum(0).flip(0)
    m2 += pick ** 2 * g.flip(0).cumsum(0).flip(0)[1:]  # P(B_k = 0) = sum_{s >= k} gamma[0][s]
    return post, torch.stack([pick, m1, m2.sqrt()])


def gemm_f32(A, B, C=None, transA=False, transB=False, beta=False):
    batch, n, _ = A.shape
    if C is None:
        C = torch.empty_like(A)
    _check(lib().crw_gemm_f32(_dev(A, "A"), _dev(B, "B"), _dev(C, "C"), n, batch, int(transA), int(transB), int(beta),
                              _stream()), "crw_gemm_f32")
    return C


def gemm_bf16(A, B, C=None, transA=False, transB=False, beta=False, split=1, ws=None, convert=True):
    """bf16 matrix-core product of fp32 [batch,n,n] operands (n % 128 == 0); returns (C, ws)."""
    batch, n, _ = A.shape
    if C is None:
        C = torch.empty_like(A)
    nbytes = lib().crw_gemm_bf16_ws_bytes(n, batch, split)
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=A.device)
    _check(lib().crw_gemm_bf16(_dev(A, "A"), _dev(B, "B"), _dev(C, "C"), n, batch, int(transA), int(transB),
                               int(beta), int(split), ctypes.c_void_p(ws.data_ptr()), ws.numel(), int(convert),
                               _stream()), "crw_gemm_bf16")
    return C, ws


# ------------------------------------------------------------------------------ encoder conv stack
_BF = torch.bfloat16


def _bf(t, name):
    return _dev(t, name, _BF) if t is not None else None


def enc_pack_weights(w, split):
    """fp32 conv weight [cout,cin,3,3] -> (fwd_hi, fwd_lo, bwd_hi, bwd_lo) bf16 planes (lo = None for split 1)."""
    cout, cin = w.shape[:2]
    mk = lambda a, b: torch.empty(9, a, b, dtype=_BF, device=w.device)
    fh, bh = mk(cout, cin), mk(cin, cout)
    fl, bl = (mk(cout, cin), mk(cin, cout)) if split == 3 else (None, None)
    _check(lib().crw_enc_pack_weights(_dev(w.contiguous(), "w"), cout, cin, _bf(fh, "fh"), _bf(fl, "fl"), _bf(bh, "bh"),
                                      _bf(bl, "bl"), _stream()), "crw_enc_pack_weights")
    return fh, fl, bh, bl


def enc_pack_input(x, split):
    """fp32 NCHW [P,C,10,10] -> channels-last planes [P,100,C]."""
    P, C, H, W = x.shape
    if (H, W) != (10, 10):
        raise RuntimeError(f"the HIP conv stack handles 10x10 feature maps (16x16 patches), got {H}x{W}")
    xh = torch.empty(P, 100, C, dtype=_BF, device=x.device)
    xl = torch.empty_like(xh) if split == 3 else None
    _check(lib().crw_enc_pack_input(_dev(x.contiguous(), "x"), P, C, _bf(xh, "xh"), _bf(xl, "xl"), _stream()),
           "crw_enc_pack_input")
    return xh, xl


def enc_conv3x3(mode, split, xh, xl, wh, wl, cout, bias=None, mask=None, planes=True, f32=False, gap=False,
                dgap=None, lo_plane=True, chain=None):
    """mode 0: relu(conv + bias) ; mode 1: backward-data with optional ReLU mask.  -> (yh, yl, yf, gap).
    dgap (mode 1): the input gradient is dgap/100 gated by xh (forward activation plane), xl ignored.
    chain (a `ConvFwdChain`): this call is one layer of conv3 -> conv4 -> conv5 and is served from the chain's one launch."""
    if chain is not None:
        if mode != 0 or split != 3 or mask is not None or not planes or f32 or dgap is not None:
            raise RuntimeError("a ConvFwdChain serves the mode-0, split-3 calls of conv3, conv4 and conv5 only")
        return chain.layer(xh, xl, wh, wl, cout, bias, gap, lo_plane)
    P, _, cin = xh.shape
    dev = xh.device
    yh = torch.empty(P, 100, cout, dtype=_BF, device=dev) if planes else None
    yl = torch.empty_like(yh) if (planes and split == 3 and lo_plane) else None
    yf = torch.empty(P, 100, cout, dtype=torch.float32, device=dev) if f32 else None
    gp = torch.empty(P, cout, dtype=torch.float32, device=dev) if gap else None
    ev = _ev_begin()
    _check(lib().crw_enc_conv3x3(mode, split, P, cin, cout, _bf(xh, "xh"), _bf(xl, "xl"), _bf(wh, "wh"), _bf(wl, "wl"),
                                 _dev(bias, "bias") if bias is not None else None, _bf(mask, "mask"), _bf(yh, "yh"),
                                 _bf(yl, "yl"), _dev(yf, "yf") if f32 else None, _dev(gp, "gap") if gap else None,
                                 _dev(dgap, "dgap") if dgap is not None else None, _stream()), "crw_enc_conv3x3")
    _ev_end(ev, ("fwd", cin, cout) if mode == 0 else ("bwd", cout, cin))
    return yh, yl, yf, gp


def conv_chain_on():
    """Does the CNN trunk run conv3 -> conv4 -> conv5 in one launch?  Yes when the library has the chain kernel, unless
    CRW_CONV_CHAIN=0 (read at every call: the per-layer route is the chain's A/B partner) or KERNEL_EVENTS is collecting:
    bench.py's per-kernel roofline brackets and names the per-layer launches."""
    return KERNEL_EVENTS is None and os.environ.get("CRW_CONV_CHAIN", "1") != "0" and has_conv_chain()


def enc_conv_fwd_chain(x3h, x3l, packed, biases):
    """relu(conv + bias) of conv3, conv4, conv5 on hi/lo planes in one launch -> (y3h, y3l, y4h, y4l, y5h, gap): bit for bit
    what three mode-0 `enc_conv3x3` calls at split 3 return (conv5 with gap=True, lo_plane=False).  packed: per layer the
    forward planes (hi, lo, ...) of `enc_pack_weights`; biases: per layer [cout] fp32."""
    P, dev = x3h.shape[0], x3h.device
    mk = lambda c: torch.empty(P, 100, c, dtype=_BF, device=dev)
    y3h, y3l, y4h, y4l, y5h = mk(64), mk(64), mk(128), mk(128), mk(128)
    gap = torch.empty(P, 128, dtype=torch.float32, device=dev)
    w = [a for pk, b in zip(packed, biases) for a in (_bf(pk[0], "w_hi"), _bf(pk[1], "w_lo"), _dev(b, "bias"))]
    _check(_conv_chain_lib().crw_enc_conv_fwd_chain(3, P, _bf(x3h, "x3h"), _bf(x3l, "x3l"), *w, _bf(y3h, "y3h"), _bf(y3l, "y3l"),
                                                    _bf(y4h, "y4h"), _bf(y4l, "y4l"), _bf(y5h, "y5h"), _dev(gap, "gap"), _stream()),
           "crw_enc_conv_fwd_chain")
    return y3h, y3l, y4h, y4l, y5h, gap


class ConvFwdChain:
    """conv3 -> conv4 -> conv5 of one forward pass in one launch, handed out layer by layer: the caller makes its three mode-0
    `enc_conv3x3` calls as ever and passes this object as `chain`.  The first call launches `enc_conv_fwd_chain` for all three
    layers; every call returns its own layer's (yh, yl, None, gap) -- the same tensors, bit for bit, that the call would have
    computed from the operands it names, which must be the chain's own (the previous call's planes, this layer's weights and bias)."""

    def __init__(self, x3h, x3l, packed, biases):
        self.inputs, self.packed, self.biases = [(x3h, x3l)], packed, biases
        self.out = None

    def layer(self, xh, xl, wh, wl, cout, bias, gap, lo_plane):
        i = len(self.inputs) - 1
        last = i == 2
        if (i > 2 or xh is not self.inputs[i][0] or xl is not self.inputs[i][1] or wh is not self.packed[i][0]
                or wl is not self.packed[i][1] or bias is not self.biases[i] or cout != (64, 128, 128)[i] or bool(gap) != last
                or bool(lo_plane) == last):
            raise RuntimeError(f"ConvFwdChain: call {i} does not name the operands of layer conv{3 + i} of this chain")
        if self.out is None:
            self.out = enc_conv_fwd_chain(self.inputs[0][0], self.inputs[0][1], self.packed, self.biases)
        y3h, y3l, y4h, y4l, y5h, gp = self.out
        yh, yl = ((y3h, y3l), (y4h, y4l), (y5h, None))[i]
        self.inputs.append((yh, yl))
        return yh, yl, None, (gp if last else None)


def linear128_wgrad(dy, x):
    """dw [128,128] = dy.T @ x for dy, x [P,128] with P % 128 == 0 (split over P, deterministic)."""
    P = x.shape[0]
    dw = torch.empty(128, 128, dtype=torch.float32, device=x.device)
    nbytes = lib().crw_linear128_wgrad_ws_bytes(P)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    _check(lib().crw_linear128_wgrad(_dev(dy.contiguous(), "dy"), _dev(x.contiguous(), "x"), _dev(dw, "dw"), P,
                                     ctypes.c_void_p(ws.data_ptr()), nbytes, _stream()), "crw_linear128_wgrad")
    return dw


def adam_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """One Adam step in place on the flat fp32 buffers p (parameters), m, v with the flat gradient g (torch.optim.Adam defaults)."""
    _check(lib().crw_adam_step(_dev(p, "p"), _dev(g, "g"), _dev(m, "m"), _dev(v, "v"), p.numel(), float(lr), float(beta1),
                               float(beta2), float(eps), int(step), _stream()), "crw_adam_step")


# the control block of crw_adam_step_guarded (include/crw_hip_guard.h): 64 bytes of device memory, zeroed once by the caller
GUARD_CTL_BYTES = 64
GUARD_CTL_FORMAT = "<qqdfi"  # int64 applied; int64 skipped; double norm; float scale; int32 last_applied; the rest is reserved
GUARD_CTL_FIELDS = ("applied", "skipped", "norm", "scale", "last_applied")


def adam_guard_ws_bytes(n):
    """bytes of the workspace crw_adam_step_guarded wants for n elements (the per-block fp64 partials and the decision record)"""
    return _guard_lib().crw_adam_guard_ws_bytes(int(n))


def check_max_norm(max_norm):
    """`max_grad_norm=` -> float (None -> 0.0, no clip); a negative or NaN bound is refused (include/crw_hip_guard.h)"""
    x = 0.0 if max_norm is None else float(max_norm)
    if not x >= 0.0:
        raise ValueError(f"max_grad_norm must be None or a number >= 0 (got {max_norm!r})")
    return x


def guard_ctl_unpack(ctl):
    """the 64 bytes of a control block (a uint8 tensor anywhere, or bytes) -> {field: value} in GUARD_CTL_FIELDS' order"""
    import struct
    raw = bytes(ctl.detach().cpu().contiguous().view(torch.uint8).tolist()) if isinstance(ctl, torch.Tensor) else bytes(ctl)
    if len(raw) != GUARD_CTL_BYTES:
        raise ValueError(f"a control block is {GUARD_CTL_BYTES} bytes (got {len(raw)})")
    return dict(zip(GUARD_CTL_FIELDS, struct.unpack_from(GUARD_CTL_FORMAT, raw)))


def adam_step_guarded(p, g, m, v, step, lr, ctl, ws, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=None):
    """crw_adam_step_guarded (include/crw_hip_guard.h): the Adam step of `adam_step`, refused on the device when g holds a NaN or an
    infinity and scaled when its norm exceeds max_norm (None / 0: no clip).  ctl: the 64-byte control block (uint8, on the device,
    zeroed once), ws: at least `adam_guard_ws_bytes(p.numel())` bytes (uint8, on the device).  Nothing is read back."""
    max_norm = check_max_norm(max_norm)
    if ctl.numel() != GUARD_CTL_BYTES:
        raise ValueError(f"ctl must hold {GUARD_CTL_BYTES} bytes (got {ctl.numel()})")
    _check(_guard_lib().crw_adam_step_guarded(_dev(p, "p"), _dev(g, "g"), _dev(m, "m"), _dev(v, "v"), p.numel(), float(lr), float(beta1),
                                              float(beta2), float(eps), int(step), max_norm, _dev(ctl, "ctl", torch.uint8),
                                              _dev(ws, "ws", torch.uint8), ws.numel(), _stream()), "crw_adam_step_guarded")


def enc_pack_input_map(x, split):
    """fp32 NCHW [P,C,H,W] -> bf16 planes [P, H*W, C] (hi, lo | None)."""
    P, C, H, W = x.shape
    xh = torch.empty(P, H * W, C, dtype=_BF, device=x.device)
    xl = torch.empty_like(xh) if split == 3 else None
    _check(lib().crw_enc_pack_input_map(_dev(x.contiguous(), "x"), P, C, H, W, _bf(xh, "xh"), _bf(xl, "xl"), _stream()),
           "crw_enc_pack_input_map")
    return xh, xl


def enc_conv3x3_map(split, xh, xl, wh, wl, cout, H, W, bias=None, planes=True, gap=False, lo_plane=True, mode=0, mask=None,
                    f32=False):
    """mode 0: relu(conv3x3 + bias) on feature maps [P, H*W, cin] of any size -> (yh, yl, gap [P, cout] mean | None);
    mode 1: backward-data with the backward weight planes, optional ReLU mask map and fp32 copy -> (yh, yl, yf)."""
    P, hw, cin = xh.shape
    assert hw == H * W
    dev = xh.device
    yh = torch.empty(P, hw, cout, dtype=_BF, device=dev) if planes else None
    yl = torch.empty_like(yh) if (planes and split == 3 and lo_plane) else None
    yf = torch.empty(P, hw, cout, dtype=torch.float32, device=dev) if f32 else None
    ntile = ((H + 9) // 10) * ((W + 9) // 10)
    gp = torch.empty(P, ntile, cout, dtype=torch.float32, device=dev) if gap else None
    ev = _ev_begin()
    _check(lib().crw_enc_conv3x3_map(mode, split, P, H, W, cin, cout, _bf(xh, "xh"), _bf(xl, "xl"), _bf(wh, "wh"), _bf(wl, "wl"),
                                     _dev(bias, "bias") if bias is not None else None, _bf(mask, "mask"), _bf(yh, "yh"),
                                     _bf(yl, "yl"), _dev(yf, "yf") if f32 else None, _dev(gp, "gap") if gap else None, _stream()),
           "crw_enc_conv3x3_map")
    _ev_end(ev, ("fwd_map", cin, cout) if mode == 0 else ("bwd_map", cout, cin))
    if mode == 1:
        return yh, yl, yf
    return yh, yl, (gp.sum(1) / float(hw) if gap else None)


def enc_wgrad_map(split, dyh, dyl, xh, xl, H, W):
    """weight / bias gradient of a 3x3 layer on feature maps [P, H*W, C] -> (dw [cout,cin,3,3], db [cout])."""
    P, hw, cout = dyh.shape
    cin = xh.shape[2]
    assert hw == H * W
    dw = torch.empty(cout, cin, 3, 3, dtype=torch.float32, device=xh.device)
    db = torch.empty(cout, dtype=torch.float32, device=xh.device)
    units = P * ((H + 9) // 10) * ((W + 9) // 10)
    nbytes = lib().crw_enc_wgrad_ws_bytes(units, cin, cout, split)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=xh.device)
    ev = _ev_begin()
    _check(lib().crw_enc_conv3x3_wgrad_map(split, P, H, W, cin, cout, _bf(dyh, "dyh"), _bf(dyl, "dyl"), _bf(xh, "xh"),
                                           _bf(xl, "xl"), _dev(dw, "dw"), _dev(db, "db"), ctypes.c_void_p(ws.data_ptr()), nbytes,
                                           _stream()), "crw_enc_conv3x3_wgrad_map")
    _ev_end(ev, ("wgrad_map", cin, cout))
    return dw, db


def enc_gap_bwd(dgap, yh, split):
    """dY = dgap / npix where yh != 0, for planes [P, npix, C] of any map size."""
    P, npix, C = yh.shape
    dh = torch.empty_like(yh)
    dl = torch.empty_like(yh) if split == 3 else None
    _check(lib().crw_enc_gap_bwd(_dev(dgap.contiguous(), "dgap"), _bf(yh, "yh"), P, C, npix, _bf(dh, "dh"), _bf(dl, "dl"),
                                 _stream()), "crw_enc_gap_bwd")
    return dh, dl


def enc_wgrad(split, dyh, dyl, xh, xl, dgap=None):
    """dgap: dY = dgap/100 gated by dyh (forward activation plane) -- fused ReLU + GAP backward."""
    P, _, cout = dyh.shape
    cin = xh.shape[2]
    dw = torch.empty(cout, cin, 3, 3, dtype=torch.float32, device=xh.device)
    db = torch.empty(cout, dtype=torch.float32, device=xh.device)
    nbytes = lib().crw_enc_wgrad_ws_bytes(P, cin, cout, split)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=xh.device)
    ev = _ev_begin()
    _check(lib().crw_enc_conv3x3_wgrad(split, P, cin, cout, _bf(dyh, "dyh"), _bf(dyl, "dyl"), _bf(xh, "xh"),
                                       _bf(xl, "xl"), _dev(dgap, "dgap") if dgap is not None else None,
                                       _dev(dw, "dw"), _dev(db, "db"), ctypes.c_void_p(ws.data_ptr()),
                                       nbytes, _stream()), "crw_enc_conv3x3_wgrad")
    _ev_end(ev, ("wgrad", cin, cout))
    return dw, db


def enc_front_pack(w2, split):
    """conv2 weight [32,8,5,5] -> (fwd_hi, fwd_lo, bwd_hi, bwd_lo) bf16 planes."""
    fh = torch.empty(7, 32, 32, dtype=_BF, device=w2.device)
    bh = torch.empty(25, 8, 32, dtype=_BF, device=w2.device)
    fl, bl = (torch.empty_like(fh), torch.empty_like(bh)) if split == 3 else (None, None)
    _check(lib().crw_enc_front_pack(_dev(w2.contiguous(), "w2"), _bf(fh, "fh"), _bf(fl, "fl"), _bf(bh, "bh"),
                                    _bf(bl, "bl"), _stream()), "crw_enc_front_pack")
    return fh, fl, bh, bl


def enc_front_fwd(split, x, w1, b1, w2f, b2, save=False):
    """x [P,cin,16,16] -> planes [P,100,32] (conv1-ReLU-pool-conv2-ReLU-pool).  save=True (training): also returns the
    record (pool1 planes + pooling codes) that lets enc_front_bwd skip the recomputation: (yh, yl, saved)."""
    P, cin = x.shape[:2]
    yh = torch.empty(P, 100, 32, dtype=_BF, device=x.device)
    yl = torch.empty_like(yh) if split == 3 else None
    saved = torch.empty(lib().crw_enc_front_saved_bytes(P), dtype=torch.uint8, device=x.device) if save else None
    ev = _ev_begin()
    _check(lib().crw_enc_front_fwd(split, _dev(x, "x"), P, cin, _dev(w1.contiguous(), "w1"), _dev(b1, "b1"),
                                   _bf(w2f[0], "w2h"), _bf(w2f[1], "w2l"), _dev(b2, "b2"), _bf(yh, "yh"), _bf(yl, "yl"),
                                   ctypes.c_void_p(saved.data_ptr()) if save else None, _stream()), "crw_enc_front_fwd")
    _ev_end(ev, ("front_fwd", cin, 32))
    return (yh, yl, saved) if save else (yh, yl)


def enc_front_fwd_map(split, x, w1, b1, w2f, b2):
    """front end on patches of any size: x [P,cin,H,W] -> planes [P, (H-6)*(W-6), 32] (hi, lo | None)."""
    P, cin, H, W = x.shape
    yh = torch.empty(P, (H - 6) * (W - 6), 32, dtype=_BF, device=x.device)
    yl = torch.empty_like(yh) if split == 3 else None
    _check(lib().crw_enc_front_fwd_map(split, _dev(x.contiguous(), "x"), P, cin, H, W, _dev(w1.contiguous(), "w1"),
                                       _dev(b1, "b1"), _bf(w2f[0], "w2h"), _bf(w2f[1], "w2l"), _dev(b2, "b2"),
                                       _bf(yh, "yh"), _bf(yl, "yl"), _stream()), "crw_enc_front_fwd_map")
    return yh, yl


def enc_front_bwd(split, x, w1, b1, w2f, b2, w2b, dy, saved=None):
    """-> (dw1, db1, dw2, db2).  saved: the record of enc_front_fwd(save=True) for the same patches (no recomputation)."""
    P, cin = x.shape[:2]
    dev = x.device
    dw1 = torch.empty(8, cin, 5, 5, device=dev)
    db1 = torch.empty(8, device=dev)
    dw2 = torch.empty(32, 8, 5, 5, device=dev)
    db2 = torch.empty(32, device=dev)
    nbytes = lib().crw_enc_front_ws_bytes(P, cin)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if saved is not None and saved.numel() < lib().crw_enc_front_saved_bytes(P):
        raise RuntimeError("saved record too small for this patch count")
    ev = _ev_begin()
    _check(lib().crw_enc_front_bwd(split, _dev(x, "x"), P, cin, _dev(w1.contiguous(), "w1"), _dev(b1, "b1"),
                                   _bf(w2f[0], "w2h"), _bf(w2f[1], "w2l"), _dev(b2, "b2"), _bf(w2b[0], "w2bh"),
                                   _bf(w2b[1], "w2bl"), _dev(dy.contiguous(), "dy"),
                                   ctypes.c_void_p(saved.data_ptr()) if saved is not None else None, _dev(dw1, "dw1"),
                                   _dev(db1, "db1"), _dev(dw2, "dw2"), _dev(db2, "db2"), ctypes.c_void_p(ws.data_ptr()), nbytes,
                                   _stream()), "crw_enc_front_bwd")
    _ev_end(ev, ("front_bwd", cin, 32))
    return dw1, db1, dw2, db2


def enc_front_bwd_map(split, x, w1, b1, w2f, b2, w2b, dy):
    """front-end backward on patches of any size: x [P,cin,H,W], dy [P,(H-6)*(W-6),32] fp32 -> (dw1, db1, dw2, db2)."""
    P, cin, H, W = x.shape
    dev = x.device
    dw1 = torch.empty(8, cin, 5, 5, device=dev)
    db1 = torch.empty(8, device=dev)
    dw2 = torch.empty(32, 8, 5, 5, device=dev)
    db2 = torch.empty(32, device=dev)
    units = P * ((H - 6 + 9) // 10) * ((W - 6 + 9) // 10)
    nbytes = lib().crw_enc_front_ws_bytes(units, cin)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _check(lib().crw_enc_front_bwd_map(split, _dev(x.contiguous(), "x"), P, cin, H, W, _dev(w1.contiguous(), "w1"), _dev(b1, "b1"),
                                       _bf(w2f[0], "w2h"), _bf(w2f[1], "w2l"), _dev(b2, "b2"), _bf(w2b[0], "w2bh"),
                                       _bf(w2b[1], "w2bl"), _dev(dy.contiguous(), "dy"), _dev(dw1, "dw1"), _dev(db1, "db1"),
                                       _dev(dw2, "dw2"), _dev(db2, "db2"), ctypes.c_void_p(ws.data_ptr()), nbytes, _stream()),
           "crw_enc_front_bwd_map")
    return dw1, db1, dw2, db2


# ------------------------------------------------------------------------------ Resnet encoder kernels (crw_rn_*)
RN_FWD, RN_BWD, RN_STEM_FWD, RN_STEM_BWD = 0, 1, 2, 3


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def rn_padded(P):
    return lib().crw_rn_padded_patches(int(P))


def rn_pack_conv(w):
    """conv / linear weight [cout,cin,kh,kw] (or [cout,cin]) fp32 -> (fwd_hi, fwd_lo, bwd_hi, bwd_lo) bf16 planes."""
    w = w.detach()
    if w.dim() == 2:
        w = w[:, :, None, None]
    cout, cin, kh, kw = w.shape
    mk = lambda: torch.empty(cout * cin * kh * kw, dtype=_BF, device=w.device)
    fh, fl, bh, bl = mk(), mk(), mk(), mk()
    _check(lib().crw_rn_pack_conv(_dev(w.contiguous(), "w"), cout, cin, kh, kw, _bf(fh, "fh"), _bf(fl, "fl"), _bf(bh, "bh"),
                                  _bf(bl, "bl"), _stream()), "crw_rn_pack_conv")
    return fh, fl, bh, bl


def rn_stem_cols(w):
    """columns of one row of the stem's input gradient: 3 * (w + 2) rounded up to 64"""
    return lib().crw_rn_stem_cols(int(w))


def rn_pack_stem(w1, h, w):
    """model.conv1 weight [64,3,7,7] -> (fwd_hi, fwd_lo [64*256], toeplitz_hi, toeplitz_lo [(h+2)*rn_stem_cols(w)*ld])."""
    ld = lib().crw_rn_stem_toeplitz_ld(w)
    fh = torch.empty(64 * 256, dtype=_BF, device=w1.device)
    fl = torch.empty_like(fh)
    th = torch.empty((h + 2) * rn_stem_cols(w) * ld, dtype=_BF, device=w1.device)
    tl = torch.empty_like(th)
    _check(lib().crw_rn_pack_stem(_dev(w1.detach().contiguous(), "w1"), h, w, _bf(fh, "fh"), _bf(fl, "fl"), _bf(th, "th"),
                                  _bf(tl, "tl"), _stream()), "crw_rn_pack_stem")
    return fh, fl, th, tl


def rn_conv(mode, P, src, dst, N, k, stride, pad, a, b, bias=None, stats=False):
    """a = (hi, lo) planes on the source map src = (Hs, Ws, Cs); b = (hi, lo) weight planes; dst = (Hd, Wd).
    -> (out fp32 [Ppad, G*N], part | None)."""
    Hs, Ws, Cs = src
    Hd, Wd = dst
    G = Hd if mode == RN_STEM_BWD else Hd * Wd
    Ppad = rn_padded(P)
    dev = a[0].device
    out = torch.empty(Ppad, G * N, dtype=torch.float32, device=dev)
    part = torch.empty(lib().crw_rn_conv_part_floats(P, G, N), dtype=torch.float32, device=dev) if stats else None
    ev = _ev_begin()
    _check(lib().crw_rn_conv(mode, P, Hs, Ws, Cs, Hd, Wd, N, k[0], k[1], stride, pad, _bf(a[0], "a_hi"), _bf(a[1], "a_lo"),
                             _bf(b[0], "b_hi"), _bf(b[1], "b_lo"), _dev(bias, "bias") if bias is not None else None,
                             _dev(out, "out"), _ptr(part), _stream()), "crw_rn_conv")
    _ev_end(ev, ("rn_conv", mode, Hs, Ws, Cs, Hd, Wd, N, k[0], stride, pad))
    return out, part


def rn_wgrad(mode, P, xin, xout, k, stride, pad, x, d):
    """x = (hi, lo) input planes on xin = (Hin, Win, Cin), d = (hi, lo) dZ planes on xout = (Hout, Wout, Cout)
    -> dw [cout, cin, kh, kw] ([64,3,7,7] for the stem)."""
    Hin, Win, Cin = xin
    Hout, Wout, Cout = xout
    dev = x[0].device
    geo = (mode, P, Hin, Win, Cin, Hout, Wout, Cout, k[0], k[1], stride, pad)
    nbytes = lib().crw_rn_wgrad_ws_bytes(*geo)
    if nbytes == 0:
        raise RuntimeError(f"crw_rn_wgrad: unsupported geometry {geo}")
    ws = _ws(nbytes, dev)
    dw = torch.empty((64, 3, 7, 7) if mode == RN_STEM_FWD else (Cout, Cin, k[0], k[1]), dtype=torch.float32, device=dev)
    ev = _ev_begin()
    _check(lib().crw_rn_wgrad(*geo, _bf(x[0], "x_hi"), _bf(x[1], "x_lo"), _bf(d[0], "d_hi"), _bf(d[1], "d_lo"), _dev(dw, "dw"),
                              _ptr(ws), nbytes, _stream()), "crw_rn_wgrad")
    _ev_end(ev, ("rn_wgrad", mode, Hin, Win, Cin, Hout, Wout, Cout, k[0], stride, pad))
    return dw


def rn_bn_stats(part, P, G, bn, momentum, update_running=True):
    """per-tile statistics of a convolution output -> coef [4, C]; updates bn.running_mean / running_var in place."""
    C = bn.weight.numel()
    dev = part.device
    coef = torch.empty(4, C, dtype=torch.float32, device=dev)
    nbytes = lib().crw_rn_bn_stats_ws_bytes(C)
    ws = _ws(nbytes, dev)
    rm = bn.running_mean if (update_running and bn.running_mean is not None) else None
    rv = bn.running_var if rm is not None else None
    _check(lib().crw_rn_bn_stats(_dev(part, "part"), P, G, C, _dev(bn.weight.detach(), "gamma"), _dev(bn.bias.detach(), "beta"),
                                 _ptr(rm), _ptr(rv), float(momentum), float(bn.eps), _dev(coef, "coef"), _ptr(ws), nbytes,
                                 _stream()), "crw_rn_bn_stats")
    return coef


def rn_bn_apply(Z, coef, P, npix, C, Zd=None, coef_d=None, res=None, relu=True):
    Ppad = rn_padded(P)
    yh = torch.empty(Ppad, npix * C, dtype=_BF, device=Z.device)
    yl = torch.empty_like(yh)
    _check(lib().crw_rn_bn_apply(_dev(Z, "Z"), _dev(coef, "coef"), _ptr(Zd), _ptr(coef_d), _ptr(res[0]) if res else None,
                                 _ptr(res[1]) if res else None, P, npix, C, int(relu), _bf(yh, "yh"), _bf(yl, "yl"), _stream()),
           "crw_rn_bn_apply")
    return yh, yl


def rn_bn_pool(Z, coef, P, H, W, C):
    Ppad = rn_padded(P)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    yh = torch.empty(Ppad, Ho * Wo * C, dtype=_BF, device=Z.device)
    yl = torch.empty_like(yh)
    amax = torch.empty(Ppad, Ho * Wo * C, dtype=torch.uint8, device=Z.device)
    _check(lib().crw_rn_bn_pool(_dev(Z, "Z"), _dev(coef, "coef"), P, H, W, C, _bf(yh, "yh"), _bf(yl, "yl"), _ptr(amax), _stream()),
           "crw_rn_bn_pool")
    return (yh, yl), amax


def rn_bn_bwd(g1, g2, mask_hi, Z, coef, P, npix, C, Zd=None, coef_d=None, want_g=False):
    """-> (dz (hi, lo), dzd (hi, lo) | None, g fp32 | None, dgamma, dbeta, dgamma_d | None, dbeta_d | None)"""
    Ppad = rn_padded(P)
    dev = Z.device
    mk = lambda: torch.empty(Ppad, npix * C, dtype=_BF, device=dev)
    dzh, dzl = mk(), mk()
    dzdh, dzdl = (mk(), mk()) if Zd is not None else (None, None)
    gout = torch.empty(Ppad, npix * C, dtype=torch.float32, device=dev) if want_g else None
    vec = lambda: torch.empty(C, dtype=torch.float32, device=dev)
    dg, db = vec(), vec()
    dgd, dbd = (vec(), vec()) if Zd is not None else (None, None)
    nbytes = lib().crw_rn_bn_bwd_ws_bytes(P, npix, C)
    ws = _ws(nbytes, dev)
    _check(lib().crw_rn_bn_bwd(_dev(g1, "g1"), _ptr(g2), _bf(mask_hi, "mask"), _dev(Z, "Z"), _dev(coef, "coef"), _ptr(Zd),
                               _ptr(coef_d), P, npix, C, _bf(dzh, "dzh"), _bf(dzl, "dzl"), _ptr(dzdh), _ptr(dzdl), _ptr(gout),
                               _ptr(dg), _ptr(db), _ptr(dgd), _ptr(dbd), _ptr(ws), nbytes, _stream()), "crw_rn_bn_bwd")
    return (dzh, dzl), ((dzdh, dzdl) if Zd is not None else None), gout, dg, db, dgd, dbd


def rn_pool_bwd(d1, d2, amax, Z, coef, P, H, W, C):
    Ppad = rn_padded(P)
    dev = Z.device
    dzh = torch.empty(Ppad, H * W * C, dtype=_BF, device=dev)
    dzl = torch.empty_like(dzh)
    dg = torch.empty(C, dtype=torch.float32, device=dev)
    db = torch.empty_like(dg)
    nbytes = lib().crw_rn_pool_bwd_ws_bytes(P, H, W, C)
    ws = _ws(nbytes, dev)
    _check(lib().crw_rn_pool_bwd(_dev(d1, "d1"), _ptr(d2), _ptr(amax), _dev(Z, "Z"), _dev(coef, "coef"), P, H, W, C, _bf(dzh, "dzh"),
                                 _bf(dzl, "dzl"), _ptr(dg), _ptr(db), _ptr(ws), nbytes, _stream()), "crw_rn_pool_bwd")
    return (dzh, dzl), dg, db


def rn_stem_fwd(x, fc0, bn0, Hm, Wm, momentum, update_running=True):
    """x [P,cin,h,w] -> (map (hi, lo) [Ppad, Hm*Wm*4], stem record [32])."""
    P, cin, h, w = x.shape
    Ppad = rn_padded(P)
    dev = x.device
    mh = torch.empty(Ppad, Hm * Wm * 4, dtype=_BF, device=dev)
    ml = torch.empty_like(mh)
    stem = torch.empty(32, dtype=torch.float32, device=dev)
    nbytes = lib().crw_rn_stem_ws_bytes()
    ws = _ws(nbytes, dev)
    rm = bn0.running_mean if (update_running and bn0.running_mean is not None) else None
    rv = bn0.running_var if rm is not None else None
    _check(lib().crw_rn_stem_fwd(_dev(x, "x"), P, cin, h, w, Hm, Wm, _dev(fc0.weight.detach().reshape(3, cin).contiguous(), "w0"),
                                 _dev(fc0.bias.detach(), "b0"), _dev(bn0.weight.detach(), "gamma"), _dev(bn0.bias.detach(), "beta"),
                                 _ptr(rm), _ptr(rv), float(momentum), float(bn0.eps), _bf(mh, "mh"), _bf(ml, "ml"), _dev(stem, "stem"),
                                 _ptr(ws), nbytes, _stream()), "crw_rn_stem_fwd")
    return (mh, ml), stem


def rn_stem_bwd(dX0, x, stem, w0, b0):
    P, cin, h, w = x.shape
    dev = x.device
    dw0 = torch.empty(3, cin, 1, 1, dtype=torch.float32, device=dev)
    db0, dg, db = (torch.empty(3, dtype=torch.float32, device=dev) for _ in range(3))
    nbytes = lib().crw_rn_stem_ws_bytes()
    ws = _ws(nbytes, dev)
    _check(lib().crw_rn_stem_bwd(_dev(dX0, "dX0"), _dev(x, "x"), _dev(stem, "stem"), _dev(w0.reshape(3, cin).contiguous(), "w0"),
                                 _dev(b0, "b0"), P, cin, h, w, _dev(dw0, "dw0"), _dev(db0, "db0"), _dev(dg, "dg"), _dev(db, "db"),
                                 _ptr(ws), nbytes, _stream()), "crw_rn_stem_bwd")
    return dw0, db0, dg, db


def rn_stem_stats(x, fc0, bn0, momentum):
    """bn0's batch statistics from the moments of the patches -> stem record [32] (updates bn0's running statistics)"""
    P, cin, h, w = x.shape
    stem = torch.empty(32, dtype=torch.float32, device=x.device)
    nbytes = lib().crw_rn_stem_ws_bytes()
    ws = _ws(nbytes, x.device)
    _check(lib().crw_rn_stem_stats(_dev(x, "x"), P, cin, h, w, _dev(fc0.weight.detach().reshape(3, cin).contiguous(), "w0"),
                                   _dev(fc0.bias.detach(), "b0"), _dev(bn0.weight.detach(), "gamma"), _dev(bn0.bias.detach(), "beta"),
                                   _ptr(bn0.running_mean), _ptr(bn0.running_var), float(momentum), float(bn0.eps), _dev(stem, "stem"),
                                   _ptr(ws), nbytes, _stream()), "crw_rn_stem_stats")
    return stem


def rn_pack_stem16(w1):
    wf = torch.empty(28672, dtype=_BF, device=w1.device)
    wt = torch.empty_like(wf)
    _check(lib().crw_rn_pack_stem16(_dev(w1.detach().contiguous(), "w1"), _bf(wf, "wf"), _bf(wt, "wt"), _stream()), "crw_rn_pack_stem16")
    return wf, wt


def rn_stem16_fwd(x, stem, wf):
    """-> (Z1 [Ppad, 81*64] fp32 (rows of the padding patches zero), part [rows, 64, 2])"""
    P, cin = x.shape[:2]
    Z1 = torch.zeros(rn_padded(P), 81 * 64, dtype=torch.float32, device=x.device)
    part = torch.empty(lib().crw_rn_stem16_rows(), 64, 2, dtype=torch.float32, device=x.device)
    _check(lib().crw_rn_stem16_fwd(_dev(x, "x"), P, cin, _dev(stem, "stem"), _bf(wf, "wf"), _dev(Z1, "Z1"), _dev(part, "part"),
                                   _stream()), "crw_rn_stem16_fwd")
    return Z1, part


def rn_stem_band_ok(h, w):
    return bool(lib().crw_rn_stem_band_ok(int(h), int(w)))


def rn_stem_band_fwd(x, stem, wf, H1, W1):
    """the stem's forward product for patches of any size -> (Z1 [Ppad, H1*W1*64] fp32, part [rows, 64, 2])"""
    P, cin, h, w = x.shape
    Z1 = torch.zeros(rn_padded(P), H1 * W1 * 64, dtype=torch.float32, device=x.device)
    part = torch.empty(lib().crw_rn_stem16_rows(), 64, 2, dtype=torch.float32, device=x.device)
    _check(lib().crw_rn_stem_band_fwd(_dev(x, "x"), P, cin, h, w, _dev(stem, "stem"), _bf(wf, "wf"), _dev(Z1, "Z1"), _dev(part, "part"),
                                      _stream()), "crw_rn_stem_band_fwd")
    return Z1, part


def rn_bn_stats_rows(part, count, bn, momentum):
    rows, C = part.shape[0], bn.weight.numel()
    coef = torch.empty(4, C, dtype=torch.float32, device=part.device)
    nbytes = lib().crw_rn_bn_stats_ws_bytes(C)
    ws = _ws(nbytes, part.device)
    _check(lib().crw_rn_bn_stats_rows(_dev(part, "part"), rows, float(count), C, _dev(bn.weight.detach(), "gamma"),
                                      _dev(bn.bias.detach(), "beta"), _ptr(bn.running_mean), _ptr(bn.running_var), float(momentum),
                                      float(bn.eps), _dev(coef, "coef"), _ptr(ws), nbytes, _stream()), "crw_rn_bn_stats_rows")
    return coef


def rn_stem16_wgrad(x, stem, dz):
    P, cin = x.shape[:2]
    dw = torch.empty(64, 3, 7, 7, dtype=torch.float32, device=x.device)
    nbytes = lib().crw_rn_stem16_ws_bytes()
    ws = _ws(nbytes, x.device)
    _check(lib().crw_rn_stem16_wgrad(_dev(x, "x"), P, cin, _dev(stem, "stem"), _bf(dz[0], "dz_hi"), _bf(dz[1], "dz_lo"), _dev(dw, "dw"),
                                     _ptr(ws), nbytes, _stream()), "crw_rn_stem16_wgrad")
    return dw


def rn_stem16_bwd(x, stem, w0, b0, wt, dz):
    P, cin = x.shape[:2]
    dev = x.device
    dw0 = torch.empty(3, cin, 1, 1, dtype=torch.float32, device=dev)
    db0, dg, db = (torch.empty(3, dtype=torch.float32, device=dev) for _ in range(3))
    nbytes = lib().crw_rn_stem16_ws_bytes()
    ws = _ws(nbytes, dev)
    _check(lib().crw_rn_stem16_bwd(_dev(x, "x"), P, cin, _dev(stem, "stem"), _dev(w0.reshape(3, cin).contiguous(), "w0"), _dev(b0, "b0"),
                                   _bf(wt, "wt"), _bf(dz[0], "dz_hi"), _bf(dz[1], "dz_lo"), _dev(dw0, "dw0"), _dev(db0, "db0"),
                                   _dev(dg, "dg"), _dev(db, "db"), _ptr(ws), nbytes, _stream()), "crw_rn_stem16_bwd")
    return dw0, db0, dg, db


def rn_split(x, P, C):
    Ppad = rn_padded(P)
    hi = torch.empty(Ppad, C, dtype=_BF, device=x.device)
    lo = torch.empty_like(hi)
    _check(lib().crw_rn_split(_dev(x, "x"), P, C, _bf(hi, "hi"), _bf(lo, "lo"), _stream()), "crw_rn_split")
    return hi, lo


def rn_colsum(x):
    rows, C = x.shape
    out = torch.empty(C, dtype=torch.float32, device=x.device)
    nbytes = lib().crw_rn_colsum_ws_bytes(C)
    ws = _ws(nbytes, x.device)
    _check(lib().crw_rn_colsum(_dev(x, "x"), rows, C, _dev(out, "out"), _ptr(ws), nbytes, _stream()), "crw_rn_colsum")
    return out


# ---- the whole encoder from native code (crw_rn_train_fwd / _bwd) ------------------------------------------------------------
RN_NPARAM, RN_NBN = 42, 13


class RnTimingRec(ctypes.Structure):
    _fields_ = [("kind", _c_int), ("mode", _c_int), ("g", _c_int * 6), ("k", _c_int), ("stride", _c_int), ("pad", _c_int),
                ("ms", _c_f)]


def _ptr_array(tensors, n):
    if len(tensors) != n:
        raise RuntimeError(f"expected {n} tensors, got {len(tensors)}")
    for t in tensors:
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("Resnet parameters / buffers must be contiguous float32 tensors on the MI355X")
    return (ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors])


def rn_train_fwd(x, params, run_mean, run_var, momentum, eps, keep=True):
    """x [P,cin,h,w]; params: the 42 parameter tensors in named_parameters() order; run_mean / run_var: the 13 BatchNorm buffer
    pairs in module order (updated in place) -> (out [P,128], workspace kept for rn_train_bwd).  keep=False: no backward pass
    follows (crw_rn_train_fwd_nograd) -> (out, None)."""
    P, cin, h, w = x.shape
    nbytes = lib().crw_rn_train_ws_bytes(P, cin, h, w)
    if nbytes == 0:
        raise RuntimeError(f"crw_rn_train_fwd: unsupported input {tuple(x.shape)}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(P, 128, dtype=torch.float32, device=x.device)
    fn = lib().crw_rn_train_fwd if keep else lib().crw_rn_train_fwd_nograd
    _check(fn(_dev(x, "x"), P, cin, h, w, _ptr_array(params, RN_NPARAM), _ptr_array(run_mean, RN_NBN),
              _ptr_array(run_var, RN_NBN), float(momentum), float(eps), _dev(out, "out"), _ptr(ws), nbytes,
              _stream()), "crw_rn_train_fwd" if keep else "crw_rn_train_fwd_nograd")
    return out, (ws if keep else None)


def rn_eval_fwd(x, params, run_mean, run_var, eps):
    """the forward with every BatchNorm on its running statistics (module.eval()); nothing is updated -> out [P,128]"""
    P, cin, h, w = x.shape
    nbytes = lib().crw_rn_train_ws_bytes(P, cin, h, w)
    if nbytes == 0:
        raise RuntimeError(f"crw_rn_eval_fwd: unsupported input {tuple(x.shape)}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(P, 128, dtype=torch.float32, device=x.device)
    _check(lib().crw_rn_eval_fwd(_dev(x, "x"), P, cin, h, w, _ptr_array(params, RN_NPARAM), _ptr_array(run_mean, RN_NBN),
                                 _ptr_array(run_var, RN_NBN), float(eps), _dev(out, "out"), _ptr(ws), nbytes, _stream()),
           "crw_rn_eval_fwd")
    return out


def rn_grad_views(params):
    """the 42 gradient tensors of crw_rn_train_bwd as views of one flat buffer + the two pointer arrays of the call.  Built at
    FORWARD time by the autograd function: the host is ahead of the GPU there, while at the start of the backward pass the GPU has
    just run the walk's few small kernels and would wait ~50 us for these 42 views."""
    sizes = [p.numel() for p in params]
    starts, tot = [], 0
    for n in sizes:
        starts.append(tot)
        tot += (n + 3) // 4 * 4  # 16-byte aligned views
    flat = torch.empty(tot, dtype=torch.float32, device=params[0].device)
    grads = [flat[o:o + n].view(p.shape) for o, n, p in zip(starts, sizes, params)]
    return grads, _ptr_array(params, RN_NPARAM), _ptr_array(grads, RN_NPARAM)


def rn_train_bwd(dout, x, params, ws, prepared=None):
    """-> the 42 gradients (views of one flat buffer), in the order of `params`; prepared: rn_grad_views(params) made earlier"""
    P, cin, h, w = x.shape
    grads, pp, gp = prepared if prepared is not None else rn_grad_views(params)
    _check(lib().crw_rn_train_bwd(_dev(dout, "dout"), _dev(x, "x"), P, cin, h, w, pp, gp, _ptr(ws), ws.numel(), _stream()),
           "crw_rn_train_bwd")
    return grads


def rn_timing(enable):
    _check(lib().crw_rn_timing_enable(int(enable)), "crw_rn_timing_enable")


def rn_timing_read(max_records=100000):
    buf = (RnTimingRec * max_records)()
    n = lib().crw_rn_timing_read(buf, max_records)
    return [buf[i] for i in range(min(n, max_records))]
