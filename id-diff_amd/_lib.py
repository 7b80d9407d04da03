"""ctypes binding of libidiff_hip.so (C ABI declared in include/idiff_hip.h).

PyTorch is used for device memory and streams only: every wrapper below takes
CUDA(=HIP) fp32/fp64 tensors, checks device / dtype / contiguity / shape on
the host, passes ``tensor.data_ptr()`` and the current stream handle to the
library and raises ``RuntimeError`` if the call reports an error.  There is no
CPU path: a missing library or a CPU tensor is an error, never a fallback.
"""
import ctypes
import os
import subprocess
from typing import NamedTuple, Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# IDIFF_LIB_VARIANT=<name>: a diagnostic / A-B build made by csrc/build.sh with IDIFF_VARIANT=<name> (scripts/_variant.py); the
# production library is never overwritten by such a build and never reports variant flags (checked in lib())
_VARIANT = os.environ.get("IDIFF_LIB_VARIANT", "")
_LIB_PATH = os.path.join(_HERE, "csrc", f"libidiff_hip.{_VARIANT}.so" if _VARIANT else "libidiff_hip.so")
_lib = None

ACT = {None: 0, "none": 0, "linear": 0, "silu": 1, "swish": 1, "elu": 2, "relu": 3, "lrelu": 4}

c_i, c_i64, c_f, c_d, c_p = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_void_p


class Epilogue(ctypes.Structure):
    """Mirror of ``idiff_epilogue`` (include/idiff_hip.h)."""
    _fields_ = [("bias", c_p), ("rowbias", c_p), ("ld_rowbias", c_i64), ("rows_per_group", c_i), ("act", c_i),
                ("residual", c_p), ("ld_residual", c_i64), ("out_scale", c_f), ("rowscale", c_p), ("colstats", c_p)]


_SIGNATURES = {
    "idiff_abi_version": (c_i, []),
    "idiff_last_error": (ctypes.c_char_p, []),
    "idiff_source_stamp": (ctypes.c_char_p, []),
    "idiff_variant_flags": (ctypes.c_char_p, []),
    "idiff_set_option": (c_i, [ctypes.c_char_p, c_i]),
    "idiff_gemm_pairs_ok": (c_i, [c_i, c_i, c_i, c_i]),
    "idiff_gemm_pairs_scale_f32": (c_i, [c_p, c_i64, c_i, c_i, c_p, c_p]),
    "idiff_gemm_pairs_f32": (c_i, [c_p, c_i64, c_i64, c_p, c_i64, c_i64, c_p, c_i, c_p, c_p, c_i64, c_i64, c_i, c_i, c_i, c_i, c_p, c_p]),
    "idiff_pairs_act_scale_f32": (c_i, [c_p, c_i, c_i, c_p, c_i, c_i, c_i, c_i, c_p, c_p]),
    "idiff_gemm_pairs_2src_f32": (c_i, [c_p, c_p, c_i64, c_i, c_p, c_p, c_i64, c_p, c_p, c_i64, c_i, c_i, c_i, c_p, c_p]),
    "idiff_set_thread_option": (c_i, [ctypes.c_char_p, c_i, c_i]),
    "idiff_upfirdn2d_f32": (c_i, [c_p, c_p, c_p] + [c_i] * 14 + [c_p]),
    "idiff_upfirdn2d_route": (ctypes.c_char_p, [c_p, c_p] + [c_i] * 14),
    "idiff_upfirdn2d_gn_f32": (c_i, [c_p, c_p, c_p, c_i, c_p] + [c_i] * 14 + [c_p]),
    "idiff_upfirdn2d_gn_ok": (c_i, [c_p, c_p, c_i, c_p] + [c_i] * 14),
    "idiff_fused_bias_act_f32": (c_i, [c_p, c_p, c_p, c_p, c_i64, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "idiff_upfirdn2d_f16": (c_i, [c_p, c_p, c_p] + [c_i] * 14 + [c_p]),
    "idiff_upfirdn2d_f64": (c_i, [c_p, c_p, c_p] + [c_i] * 14 + [c_p]),
    "idiff_fused_bias_act_f16": (c_i, [c_p, c_p, c_p, c_p, c_i64, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "idiff_fused_bias_act_f64": (c_i, [c_p, c_p, c_p, c_p, c_i64, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "idiff_gemm_f32": (c_i, [c_p, c_i64, c_i64, c_p, c_i64, c_i64, c_p, c_i64, c_i64, c_i, c_i, c_i, c_i,
                             ctypes.POINTER(Epilogue), c_p]),
    "idiff_gemm_2src_f32": (c_i, [c_p, c_p, c_i64, c_i, c_p, c_i64, c_p, c_i64, c_i, c_i, c_i, ctypes.POINTER(Epilogue), c_p]),
    "idiff_gemm_2src_ld_f32": (c_i, [c_p, c_i64, c_p, c_i64, c_i, c_p, c_i64, c_p, c_i64, c_i, c_i, c_i, ctypes.POINTER(Epilogue), c_p]),
    "idiff_gemm_2src_ld_ok": (c_i, [c_i, c_i]),
    "idiff_conv2d_nhwc_f32": (c_i, [c_p, c_p, c_p] + [c_i] * 10 + [ctypes.POINTER(Epilogue), c_p]),
    "idiff_gemm_route": (ctypes.c_char_p, [c_p, c_i64, c_i64, c_p, c_i64, c_i64, c_p, c_i64, c_i64, c_i, c_i, c_i, c_i,
                                           ctypes.POINTER(Epilogue), c_i]),
    "idiff_conv2d_route": (ctypes.c_char_p, [c_p, c_p, c_p] + [c_i] * 10 + [ctypes.POINTER(Epilogue)]),
    "idiff_gemm_colstats_split": (c_i, [c_i, c_i, c_i, c_i64, c_i64, c_i]),
    "idiff_conv2d_colstats_split": (c_i, [c_i] * 10),
    "idiff_conv2d_winograd_ok": (c_i, [c_i] * 5),
    "idiff_winograd_weight_floats": (c_i64, [c_i, c_i]),
    "idiff_winograd_pack_f32": (c_i, [c_p, c_p, c_i, c_i, c_p]),
    "idiff_conv2d_winograd_f32": (c_i, [c_p, c_p, c_p] + [c_i] * 5 + [ctypes.POINTER(Epilogue), c_p]),
    "idiff_conv2d_winograd_colstats_split": (c_i, [c_i] * 5),
    "idiff_conv2d_winograd43_ok": (c_i, [c_i] * 5),
    "idiff_conv2d_winograd43_colstats_split": (c_i, [c_i] * 5),
    "idiff_winograd43_weight_floats": (c_i64, [c_i, c_i]),
    "idiff_winograd43_pack_f32": (c_i, [c_p, c_p, c_i, c_i, c_p]),
    "idiff_conv2d_winograd43_f32": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, ctypes.POINTER(Epilogue), c_p]),
    "idiff_conv2d_winograd43h_ok": (c_i, [c_i] * 5),
    "idiff_winograd43h_weight_floats": (c_i64, [c_i, c_i]),
    "idiff_winograd43h_pack_f32": (c_i, [c_p, c_p, c_i, c_i, c_p]),
    "idiff_conv2d_winograd43h_f32": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, ctypes.POINTER(Epilogue), c_p]),
    "idiff_conv2d_wino1d_ok": (c_i, [c_i] * 5),
    "idiff_conv2d_wino1d_resup_ok": (c_i, [c_i] * 5),
    "idiff_conv2d_wino1d_resup_f32": (c_i, [c_p, c_p, c_p] + [c_i] * 5 + [ctypes.POINTER(Epilogue), c_p, ctypes.POINTER(ctypes.c_float), c_p]),
    "idiff_conv2d_wino1d_colstats_split": (c_i, [c_i] * 5),
    "idiff_wino1d_weight_floats": (c_i64, [c_i, c_i]),
    "idiff_wino1d_pack_f32": (c_i, [c_p, c_p, c_i, c_i, c_p]),
    "idiff_conv2d_wino1d_f32": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, ctypes.POINTER(Epilogue), c_p]),
    "idiff_conv2d_wino1d_gn_ok": (c_i, [c_i] * 6),
    "idiff_conv2d_wino1d_normload_ok": (c_i, [c_i] * 5),
    "idiff_conv2d_wino1d_normload_f32": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, ctypes.POINTER(Epilogue), c_p, c_i, c_p]),
    "idiff_conv2d_wino1d_normload_2src_ok": (c_i, [c_i] * 6),
    "idiff_conv2d_wino1d_normload_2src_f32": (c_i, [c_p, c_i, c_p, c_i, c_p, c_p, c_i, c_i, c_i, c_i, ctypes.POINTER(Epilogue), c_p, c_i, c_p]),
    "idiff_groupnorm_coef_f32": (c_i, [c_p, c_i, c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_p, c_p, c_p, c_p]),
    "idiff_conv2d_wino1d_gn_f32": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, ctypes.POINTER(Epilogue), c_i, c_p, c_p, c_f, c_i, c_p]),
    "idiff_groupnorm_finalize_f32": (c_i, [c_p, c_i, c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_p, c_p]),
    "idiff_groupnorm_nsplit": (c_i, [c_i, c_i, c_i]),
    "idiff_groupnorm_stats_f32": (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_f, c_p, c_p, c_p]),
    "idiff_groupnorm_apply_f32": (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_i64, c_i, c_p, c_p]),
    "idiff_groupnorm_apply_colstats_f32": (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_p, c_i, c_p, c_i, c_f, c_p, c_p, c_p, c_i64,
                                                 c_i, c_p, c_p]),
    "idiff_groupnorm_apply_route": (ctypes.c_char_p, [c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p]),
    "idiff_groupnorm_apply_colstats_route": (ctypes.c_char_p, [c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_p, c_i, c_p, c_i, c_p, c_p, c_p]),
    "idiff_softmax_rows_f32": (c_i, [c_p, c_p, c_i64, c_i, c_f, c_p]),
    "idiff_softmax_rows_route": (ctypes.c_char_p, [c_p, c_p, c_i64, c_i, c_f]),
    "idiff_attention256_ok": (c_i, [c_i, c_i, c_i]),
    "idiff_attention256_f32": (c_i, [c_p, c_i64, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_f, c_p]),
    "idiff_attention_heads_ok": (c_i, [c_i, c_i, c_i, c_i]),
    "idiff_attention_heads_f32": (c_i, [c_p, c_i64, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p]),
    "idiff_attention256_route": (ctypes.c_char_p, [c_p, c_i64, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i]),
    "idiff_attention_heads_route": (ctypes.c_char_p, [c_p, c_i64, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i]),
    "idiff_affine_act_f32": (c_i, [c_p, c_p, c_i64, c_f, c_f, c_i, c_p, c_i64, c_p]),
    "idiff_add_scale_f32": (c_i, [c_p, c_p, c_p, c_i64, c_f, c_p]),
    "idiff_affine_act_route": (ctypes.c_char_p, [c_p, c_p, c_i64, c_p, c_i64]),
    "idiff_add_scale_route": (ctypes.c_char_p, [c_p, c_p, c_p, c_i64]),
    "idiff_concat_cols_route": (ctypes.c_char_p, [c_p, c_i, c_p, c_i, c_p, c_i64]),
    "idiff_fourier_embed_f32": (c_i, [c_p, c_p, c_p, c_i, c_i, c_p]),
    "idiff_positional_embed_f32": (c_i, [c_p, c_p, c_i, c_i, c_f, c_i, c_p]),
    "idiff_concat_cols_f32": (c_i, [c_p, c_i, c_p, c_i, c_p, c_i64, c_p]),
    "idiff_nchw_to_nhwc_f32": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "idiff_nhwc_to_nchw_f32": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p]),
    "idiff_resample2x_nhwc_f32": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "idiff_perturb_f32": (c_i, [c_p, c_p, c_p, c_p, c_p, c_i64, c_i64, c_p]),
    "idiff_perturb_randn_f32": (c_i, [c_p, c_p, c_p, c_p, c_i64, c_i64, c_i64, ctypes.c_uint64, c_p, c_p]),
    "idiff_spectrum_workspace_bytes": (c_i64, [c_i, c_i, c_i]),
    "idiff_spectrum_f32": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p]),
    "idiff_colmean_f64": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p, c_p]),
    "idiff_centered_gram_f64": (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_p]),
    "idiff_centered_gram_rows_f64": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p]),
    "idiff_symmetrize_upper_f64": (c_i, [c_p, c_i, c_p]),
    "idiff_symtridiag_scratch_doubles": (c_i64, [c_i]),
    "idiff_symband_ld": (c_i, []),
    "idiff_symband_f64": (c_i, [c_p, c_i, c_p, c_p]),
    "idiff_symtridiag_f64": (c_i, [c_p, c_i, c_i, c_p, c_p, c_p, c_p]),
    "idiff_symtridiag_plan": (c_i, [c_i]),
    "idiff_tridiag_eigvals_f64": (c_i, [c_p, c_p, c_i, c_i, c_p, c_p]),
    "idiff_sym_lowvecs_scratch_doubles": (c_i64, [c_i, c_i]),
    "idiff_sym_lowvecs_f64": (c_i, [c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
    "idiff_sym_topvecs_scratch_doubles": (c_i64, [c_i, c_i, c_i]),
    "idiff_sym_topvecs_f64": (c_i, [c_p, c_i, c_i, c_i, c_d, c_d, c_d, c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
    "idiff_knn_workspace_bytes": (c_i64, [c_i, c_i, c_i]),
    "idiff_knn_f32": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p, c_p]),
    "idiff_apsp_tile": (c_i, []),
    "idiff_knn_graph_f64": (c_i, [c_p, c_p, c_i, c_i, c_p, c_p]),
    "idiff_apsp_f64": (c_i, [c_p, c_i, c_p]),
    "idiff_double_center_scratch_doubles": (c_i64, [c_i]),
    "idiff_double_center_f64": (c_i, [c_p, c_i, c_p, c_p, c_p, c_p]),
    "idiff_component_labels_f64": (c_i, [c_p, c_i, c_p, c_p, c_p, c_p]),
    "idiff_component_bridges_workspace_bytes": (c_i64, [c_i]),
    "idiff_component_bridges_f64": (c_i, [c_p, c_i, c_i, c_p, c_i, c_p, c_i64, c_p, c_p, c_p, c_p]),
    "idiff_minplus_f64": (c_i, [c_p, c_i64, c_p, c_i64, c_p, c_i64, c_i, c_i, c_i, c_p]),
    "idiff_symmetrize_min_f64": (c_i, [c_p, c_i, c_p]),
    "idiff_knn_cross_workspace_bytes": (c_i64, [c_i, c_i]),
    "idiff_knn_cross_f64": (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p]),
    "idiff_isomap_project_scratch_doubles": (c_i64, [c_i]),
    "idiff_isomap_project_f64": (c_i, [c_p, c_p, c_i, c_i, c_p, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_p]),
    "idiff_render_squares_f32": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_p]),
    "idiff_render_gaussians_f32": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_p]),
    "idiff_ksphere_union_ok": (c_i, [c_i, c_i, c_i]),
    "idiff_ksphere_union_score_f32": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    "idiff_local_pca_ok": (c_i, [c_i, c_i, c_i, c_i]),
    "idiff_local_pca_chunk": (c_i, []),
    "idiff_local_pca_f64": (c_i, [c_p, c_i, c_i, c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p]),
    "idiff_simplex_skewness_ok": (c_i, [c_i, c_i, c_i, c_i]),
    "idiff_simplex_skewness_f64": (c_i, [c_p, c_i, c_i, c_p, c_p, c_i, c_i, c_p, c_i, c_p, c_p, c_p]),
    "idiff_empirical_score_ok": (c_i, [c_i64, c_i]),
    "idiff_empirical_score_f32": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i64, c_i, c_p]),
    "idiff_empirical_jacobian_ok": (c_i, [c_i64, c_i]),
    "idiff_empirical_jacobian_f64": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i64, c_i, c_p]),
    "idiff_empirical_flipd_ok": (c_i, [c_i64, c_i, c_i]),
    "idiff_empirical_flipd_workspace_doubles": (c_i64, [c_i64, c_i, c_i]),
    "idiff_empirical_flipd_splits": (c_i, [c_i64, c_i64, c_i]),
    "idiff_empirical_flipd_f64": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i64, c_i64, c_i64, c_i, c_i, c_i, c_p]),
    "idiff_gemm_nn_ok": (c_i, [c_i, c_i, c_i]),
    "idiff_gemm_nn_f32": (c_i, [c_p, c_i64, c_p, c_i64, c_p, c_i64, c_p, c_i64, c_i, c_i, c_i, c_p]),
    "idiff_gemm_tn_ok": (c_i, [c_i, c_i, c_i]),
    "idiff_gemm_tn_f32": (c_i, [c_p, c_i64, c_p, c_i64, c_p, c_i64, c_p, c_i, c_i, c_i, c_p]),
    "idiff_dsm_loss_grad_f32": (c_i, [c_p, c_p, c_p, c_p, c_i64, c_p, c_p, c_i, c_i, c_i, c_p]),
    "idiff_grad_sumsq_f32": (c_i, [c_p, c_i64, c_p, c_p, c_p]),
    "idiff_adam_step_f32": (c_i, [c_p, c_p, c_p, c_p, c_i64, c_p, c_d, c_d, c_d, c_d, c_d, c_d, c_i64, c_p]),
    "idiff_fcn_train_input_f32": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i64, c_i, c_i, c_p]),
    "idiff_sampler_step_f32": (c_i, [c_p, c_i64, c_p, c_i64, c_p, c_i64, c_p, c_i64, c_p, c_i64, c_i64, c_i, c_d, c_d, c_d, c_p, c_d, c_d,
                                     ctypes.c_uint64, c_i64, c_i, c_f, c_p]),
    "idiff_sampler_noise_norm_f32": (c_i, [c_p, c_i64, c_i64, c_i, ctypes.c_uint64, c_i64, c_p, c_p, c_p]),
    "idiff_jvp_layer_ok": (c_i, [c_i, c_i, c_i]),
    "idiff_jvp_seed_f32": (c_i, [c_p, c_i64, c_p, c_i64, c_p, c_i64, c_i64, c_i, c_i, c_i, c_p]),
    "idiff_jvp_layer_f32": (c_i, [c_p, c_i64, c_i64, c_p, c_i64, c_p, c_i64, c_p, c_i64, c_i64, c_i, c_i, c_i, c_i, c_p]),
    "idiff_rk_stage_f64": (c_i, [c_p, c_i64, c_p, c_i64, c_i64, c_p, c_i, c_p, c_i64, c_p, c_i64, c_i64, c_i, c_i, c_f, c_p]),
    "idiff_rk_error_f64": (c_i, [c_p, c_i64, c_i64, c_p, c_p, c_i64, c_p, c_i64, c_i64, c_i, c_d, c_d, c_p, c_p, c_p]),
    "idiff_flow_rhs_f64": (c_i, [c_p, c_i64, c_p, c_i64, c_d, c_d, c_p, c_i64, c_i64, c_i, c_i, c_p, c_i64, c_p, c_i64, c_p, c_p]),
    "idiff_jvp_trace_f64": (c_i, [c_p, c_i64, c_i64, c_p, c_i64, c_p, c_i, c_i, c_i, c_p]),
    "idiff_stein_rows_ok": (c_i, [c_i64, c_i64]),
    "idiff_stein_rows_f64": (c_i, [c_p, c_i64, c_i64, c_p, c_p, c_i64, c_i64, c_p, c_i64, c_p, c_p, c_i64, c_i64, c_i64, c_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def library_path():
    return _LIB_PATH


def build(verbose=False):
    """Compile csrc/*.hip for gfx950 with hipcc (works without a GPU)."""
    out = subprocess.run(["bash", os.path.join(_HERE, "csrc", "build.sh")], capture_output=True, text=True)
    if out.returncode != 0:
        raise RuntimeError("building libidiff_hip.so failed:\n" + out.stdout + out.stderr)
    if verbose:
        print(out.stdout.strip())
    return _LIB_PATH


def source_stamp():
    """The stamp csrc/build.sh computes: sha256 over csrc/*.hip, csrc/*.h (sorted) and include/idiff_hip.h."""
    import hashlib
    csrc = os.path.join(_HERE, "csrc")
    names = sorted(f for f in os.listdir(csrc) if f.endswith(".hip") or f.endswith(".h"))
    h = hashlib.sha256()
    for f in [os.path.join(csrc, n) for n in names] + [os.path.join(os.path.dirname(_HERE), "include", "idiff_hip.h")]:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def lib():
    """The loaded library; raises (never falls back) when it is missing or stale."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                f"{_LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(id-diff_amd has no CPU or PyTorch fallback).")
        handle = ctypes.CDLL(_LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError here == header/library mismatch
            fn.restype, fn.argtypes = res, args
        if handle.idiff_abi_version() != 1:
            raise RuntimeError("libidiff_hip.so ABI version mismatch; rebuild it")
        built, tree = handle.idiff_source_stamp().decode(), source_stamp()
        if built != tree:
            raise RuntimeError(f"{_LIB_PATH} was built from other sources (stamp {built}, tree {tree}): rebuild it with "
                               "`python -c 'import __graft_entry__ as g; g.build()'`")
        flags = handle.idiff_variant_flags().decode()
        if flags and not _VARIANT:
            raise RuntimeError(f"{_LIB_PATH} is a diagnostic build (compiled with {flags!r}): its kernels may be wrong by construction. "
                               "Rebuild the product library with `python -c 'import __graft_entry__ as g; g.build()'`")
        if _VARIANT:
            import sys
            print(f"[id-diff_amd] DIAGNOSTIC library {os.path.basename(_LIB_PATH)} (flags: {flags or 'none'}) -- not the product",
                  file=sys.stderr, flush=True)
        _lib = handle
    return _lib


def set_option(name, value):
    """Flip a library debug switch (``IDIFF_NO_WINOGRAD`` ...); returns the previous value."""
    prev = lib().idiff_set_option(name.encode(), int(value))
    if prev < 0:
        raise KeyError(f"unknown libidiff_hip option {name!r}")
    return prev if prev > 1 else bool(prev)


class thread_option:
    """``with thread_option("IDIFF_CHASE_WAVEFRONT", 1): ...`` -- the switch for the launches THIS host thread makes inside the
    block, and for nobody else's (idiff_set_thread_option: launchers read their switches on the calling thread).  This is
    what the fail-soft re-solve uses: flipping the process-wide switch around a launch would also redirect an eigensolve
    that another host thread launches in that window."""

    def __init__(self, name, value):
        self.name, self.value = name.encode(), int(value)

    def __enter__(self):
        if lib().idiff_set_thread_option(self.name, self.value, 1) != 0:
            raise KeyError(f"unknown libidiff_hip option {self.name.decode()!r}")
        return self

    def __exit__(self, *exc):
        lib().idiff_set_thread_option(self.name, 0, 0)
        return False


def _check(rc, what):
    if rc != 0:
        msg = lib().idiff_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t, name, dtype=torch.float32, contiguous=True):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name}: expected a tensor on the MI355X (cuda device), got {t.device}; "
                           "id-diff_amd has no CPU path")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if contiguous and not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor")
    return t


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def make_epilogue(bias=None, rowbias=None, rows_per_group=1, act=None, residual=None, out_scale=1.0,
                  ld_rowbias=None, ld_residual=None, rowscale=None, colstats=None):
    ep = Epilogue()
    ep.bias = _ptr(bias)
    ep.rowbias = _ptr(rowbias)
    ep.ld_rowbias = (rowbias.stride(0) if ld_rowbias is None else ld_rowbias) if rowbias is not None else 0
    ep.rows_per_group = int(rows_per_group)
    ep.act = ACT[act]
    ep.residual = _ptr(residual)
    ep.ld_residual = (residual.shape[-1] if ld_residual is None else ld_residual) if residual is not None else 0
    ep.out_scale = float(out_scale)
    ep.rowscale = _ptr(rowscale)
    ep.colstats = _ptr(colstats)
    # the struct only carries raw addresses: keep the tensors alive until the launch that consumes `ep` is enqueued
    ep._keepalive = (bias, rowbias, residual, rowscale, colstats)
    return ep


def with_groupnorm(ep, groups, gamma, beta, eps, act):
    """Ask the contraction that consumes ``ep`` to apply the GroupNorm (``groups`` groups, ``gamma`` / ``beta`` [N], ``eps``) and the
    activation that read its output in its own tail.  The request rides BESIDE the C struct (idiff_epilogue is shared by every
    contraction and does not know it): conv2d_wino1d serves it through idiff_conv2d_wino1d_gn_f32, every other wrapper refuses it."""
    _dev(gamma, "gamma"); _dev(beta, "beta")
    ep.groupnorm = (int(groups), gamma, beta, float(eps), ACT[act])
    return ep


class NormLoad(NamedTuple):
    """The loader-norm request of with_normload.  ``x2 is None``: one source."""
    coef: torch.Tensor
    act: int
    x2: Optional[torch.Tensor]
    C1: Optional[int]


def with_normload(ep, coef, act, x2=None, C1=None):
    """Ask the convolution that consumes ``ep`` to apply the GroupNorm (+ ``act``: "silu" or None) in FRONT of it in its own loader:
    ``coef`` [B, Cin, 2] from groupnorm_coef, the input handed to the launch is the norm's RAW input.  With ``x2`` and ``C1`` (both or
    neither) the convolution is one of cat[x, x2] along the channels that is never made: the launch's ``x`` is the first source
    [B, H*W, C1], ``x2`` the second [B, H*W, Cin - C1].  Rides beside the C struct as with_groupnorm's request does (``ep.normload``);
    conv2d_wino1d serves it through idiff_conv2d_wino1d_normload_f32 / _2src_f32, every other wrapper refuses it."""
    _dev(coef, "coef")
    if (x2 is None) != (C1 is None):
        raise RuntimeError("with_normload: a second source x2 and the first one's channel count C1 come together or not at all")
    if x2 is not None:
        _dev(x2, "x2")
    ep.normload = NormLoad(coef, ACT[act], x2, None if C1 is None else int(C1))
    return ep


class ResidualUp2(NamedTuple):
    """The upsampled-residual request of with_residual_up2."""
    lo: torch.Tensor
    taps: tuple


def polyphase_up2(k, pad0, pad1):
    """The 16 polyphase weights w[a][b][u][v] (flattened) of upfirdn2d(x, k, up=2, pad=(pad0, pad1)) with a 4 x 4 kernel ``k``: output pixel
    (2 i + a, 2 j + b) = sum over u, v of x[i - 1 + a + u][j - 1 + b + v] * w[a][b][u][v], samples outside x counting as zero.  Pure host
    arithmetic in fp64 on the kernel as given: zero insertion leaves every second sample, so of the four taps of the FLIPPED kernel along
    an axis a phase meets two, t = a + 2 u, at input offset (a + t - pad0) / 2 = a + u - 1."""
    k = [[float(v) for v in row] for row in (k.tolist() if hasattr(k, "tolist") else k)]
    if len(k) != 4 or any(len(row) != 4 for row in k):
        raise RuntimeError("polyphase_up2: a 4 x 4 kernel is expected")
    if (pad0, pad1) != (2, 1):
        raise RuntimeError(f"polyphase_up2: pads (2, 1) are expected (upsample_2d with a 4-tap kernel), got ({pad0}, {pad1})")
    flipped = lambda t, s: k[3 - t][3 - s]
    return tuple(flipped(a + 2 * u, b + 2 * v) for a in (0, 1) for b in (0, 1) for u in (0, 1) for v in (0, 1))


def with_residual_up2(ep, lo, taps):
    """Ask the convolution that consumes ``ep`` to add the residual ``lo`` [B, (H/2) * (W/2), Cout] (fp32, 16-byte aligned, pitch Cout)
    upsampled x2 by the FIR whose 16 polyphase weights are ``taps`` (polyphase_up2), where a plain residual would be added: the
    full-resolution residual is never written.  Rides beside the C struct as with_groupnorm's request does (``ep.residual_up2``);
    conv2d_wino1d serves it through idiff_conv2d_wino1d_resup_f32 (ask conv2d_wino1d_resup_ok), every other wrapper refuses it."""
    _dev(lo, "lo")
    taps = tuple(float(t) for t in taps)
    if len(taps) != 16:
        raise RuntimeError(f"with_residual_up2: 16 polyphase weights are expected, got {len(taps)}")
    if ep.residual:
        raise RuntimeError("with_residual_up2: the epilogue already carries a residual")
    ep.residual_up2 = ResidualUp2(lo, taps)
    return ep


def _ep_ref(epilogue, what):
    """The epilogue argument of a launch that has no fused GroupNorm: such a request is an error, never dropped."""
    if epilogue is None:
        return None
    if getattr(epilogue, "normload", None) is not None:
        raise RuntimeError(f"{what}: the epilogue asks for a GroupNorm in the loader (with_normload), which only conv2d_wino1d serves")
    if getattr(epilogue, "groupnorm", None) is not None:
        raise RuntimeError(f"{what}: the epilogue asks for a fused GroupNorm (with_groupnorm), which only conv2d_wino1d serves")
    if getattr(epilogue, "residual_up2", None) is not None:
        raise RuntimeError(f"{what}: the epilogue asks for an upsampled residual (with_residual_up2), which only conv2d_wino1d serves")
    return ctypes.byref(epilogue)


# ------------------------------------------------------------------------------------------- native ops
# the dtypes of the reference's native-op dispatch (AT_DISPATCH_FLOATING_TYPES_AND_HALF) -> entry-point suffix
OP_DTYPES = {torch.float32: "f32", torch.float16: "f16", torch.float64: "f64"}


def op_suffix(t, name):
    """Entry-point suffix for a native-op tensor; any other dtype is refused as the reference's dispatch refuses it."""
    try:
        return OP_DTYPES[t.dtype]
    except KeyError:
        raise RuntimeError(f"{name}: dtype {t.dtype} is not one of float32 / float16 / float64 (the reference's native ops "
                           "dispatch on floating types and half, op/upfirdn2d_kernel.cu:311)") from None


def upfirdn2d_raw(x, k, out, major, in_h, in_w, minor, up_x, up_y, down_x, down_y, px0, px1, py0, py1):
    kh, kw = k.shape
    sfx = op_suffix(x, "upfirdn2d")
    if k.dtype != x.dtype or out.dtype != x.dtype:
        raise RuntimeError(f"upfirdn2d: input {x.dtype}, kernel {k.dtype} and output {out.dtype} must share one dtype")
    fn = getattr(lib(), "idiff_upfirdn2d_" + sfx)
    _check(fn(x.data_ptr(), k.data_ptr(), out.data_ptr(), major, in_h, in_w, minor, kh, kw,
              up_x, up_y, down_x, down_y, px0, px1, py0, py1, _stream()), "idiff_upfirdn2d_" + sfx)


def upfirdn2d_route(x, out, major, in_h, in_w, minor, kh, kw, up_x, up_y, down_x, down_y, px0, px1, py0, py1):
    """Name of the kernel ``upfirdn2d_raw`` would launch for these arguments (fp32 entry point), None if it refuses them.
    x / out: tensors or raw addresses (only their 16-byte alignment matters); nothing is launched."""
    addr = lambda t: t if isinstance(t, int) else t.data_ptr()
    name = lib().idiff_upfirdn2d_route(addr(x), addr(out), major, in_h, in_w, minor, kh, kw, up_x, up_y, down_x, down_y,
                                       px0, px1, py0, py1)
    return None if name is None else name.decode()


def upfirdn2d_gn(x, k, coef, act, out, major, in_h, in_w, minor, up_x, up_y, down_x, down_y, px0, px1, py0, py1):
    """upfirdn2d_raw (fp32, NHWC) of act(a x + b): ``x`` is a GroupNorm's RAW input, ``coef`` [major, minor, 2] from
    groupnorm_reader_coef, ``act`` "silu" or None.  Served on the two NHWC resampling kernels of the score networks
    (upfirdn2d_gn_ok); anything else is refused, nothing launched."""
    kh, kw = k.shape
    for t, name in ((x, "input"), (k, "kernel"), (coef, "coef"), (out, "output")):
        _dev(t, name)
    if coef.numel() != major * minor * 2:
        raise RuntimeError(f"upfirdn2d_gn: coef holds {coef.numel()} floats, [major, minor, 2] = {major * minor * 2} expected")
    _check(lib().idiff_upfirdn2d_gn_f32(x.data_ptr(), k.data_ptr(), coef.data_ptr(), ACT[act], out.data_ptr(), major, in_h, in_w, minor,
                                        kh, kw, up_x, up_y, down_x, down_y, px0, px1, py0, py1, _stream()), "idiff_upfirdn2d_gn_f32")


def upfirdn2d_gn_ok(x, coef, act, out, major, in_h, in_w, minor, kh, kw, up_x, up_y, down_x, down_y, px0, px1, py0, py1):
    """True where upfirdn2d_gn serves these arguments; x / coef / out: tensors or raw addresses (only their alignment matters).  Off
    under IDIFF_NO_FUSED_GN_FIR.  Launches nothing."""
    addr = lambda t: t if isinstance(t, int) else t.data_ptr()
    return bool(lib().idiff_upfirdn2d_gn_ok(addr(x), addr(coef), ACT[act], addr(out), major, in_h, in_w, minor, kh, kw, up_x, up_y,
                                            down_x, down_y, px0, px1, py0, py1))


def upfirdn2d_out_size(in_size, up, down, pad0, pad1, k):
    return (in_size * up + pad0 + pad1 - k) // down + 1


def fused_bias_act(x, bias, ref, act, grad, alpha, scale):
    sfx = op_suffix(x, "fused_bias_act")
    _dev(x, "input", dtype=x.dtype)
    out = torch.empty_like(x)
    has_b = bias is not None and bias.numel() > 0
    has_r = ref is not None and ref.numel() > 0
    if has_b:
        _dev(bias, "bias", dtype=x.dtype)
        if x.ndim < 2 or bias.numel() != x.shape[1]:
            raise RuntimeError(f"bias has {bias.numel()} entries but input dim 1 is {tuple(x.shape)}")
    if has_r:
        _dev(ref, "refer", dtype=x.dtype)
        if ref.shape != x.shape:
            raise RuntimeError("refer must have the shape of input")
    step_b = 1
    for d in x.shape[2:]:
        step_b *= d
    _check(getattr(lib(), "idiff_fused_bias_act_" + sfx)(x.data_ptr(), _ptr(bias if has_b else None), _ptr(ref if has_r else None),
                                                         out.data_ptr(), x.numel(), step_b, bias.numel() if has_b else 0, act, grad,
                                                         alpha, scale, _stream()), "idiff_fused_bias_act_" + sfx)
    return out


# ------------------------------------------------------------------------------------------- contractions
def gemm(a, bt, out=None, epilogue=None, M=None, N=None, K=None, lda=None, ldb=None, ldc=None,
         batch=1, stride_a=0, stride_b=0, stride_c=0):
    """out[b] = epilogue(a[b] @ bt[b].T); 2-D tensors by default, explicit geometry for batched views."""
    explicit = M is not None  # strided views of larger buffers: the caller supplies the geometry
    _dev(a, "a", contiguous=not explicit); _dev(bt, "bt", contiguous=not explicit)
    if M is None:
        M, K = a.shape
        N = bt.shape[0]
        if bt.shape[1] != K:
            raise RuntimeError(f"gemm: inner dimensions differ: {tuple(a.shape)} x {tuple(bt.shape)}^T")
        lda, ldb = a.stride(0), bt.stride(0)
    if out is None:
        out = torch.empty((M, N) if batch == 1 else (batch, M, N), device=a.device, dtype=torch.float32)
        ldc = N
        stride_c = M * N
    elif ldc is None:
        ldc = out.stride(-2)
    _dev(out, "out", contiguous=not explicit)
    ep = _ep_ref(epilogue, "gemm")
    _check(lib().idiff_gemm_f32(a.data_ptr(), lda, stride_a, bt.data_ptr(), ldb, stride_b, out.data_ptr(), ldc, stride_c,
                                M, N, K, batch, ep, _stream()), "idiff_gemm_f32")
    return out


def gemm_pairs_ok(M, N, K, batch=1):
    """True when gemm_pairs serves this shape (IDIFF_NO_PAIRS / IDIFF_NO_SPLIT / IDIFF_NO_PIPE turn it off)."""
    return bool(lib().idiff_gemm_pairs_ok(M, N, K, batch))


def gemm_pairs_scale(w):
    """Device tensor {s, 1 / s}: the power of two a weight [rows, K] is multiplied by before its cut into fp16 pairs (once per weight)."""
    _dev(w, "w")
    out = torch.empty(2, device=w.device, dtype=torch.float32)
    _check(lib().idiff_gemm_pairs_scale_f32(w.data_ptr(), w.stride(0), w.shape[0], w.shape[1], out.data_ptr(), _stream()),
           "idiff_gemm_pairs_scale_f32")
    return out


def gemm_pairs(a, bt, w_scale, out, epilogue=None, weight_is_a=False, M=None, N=None, K=None, lda=None, ldb=None, ldc=None,
               batch=1, stride_a=0, stride_b=0, stride_c=0, act_scale=None):
    """out[b] = epilogue(a[b] @ bt[b].T) on fp16 pairs (three matrix instructions per block instead of six).  One operand is a
    weight -- ``bt``, or ``a`` with ``weight_is_a`` -- whose ``w_scale`` comes from gemm_pairs_scale; the other an activation of
    order one (a GroupNorm's output): see idiff_gemm_pairs_f32.  2-D tensors by default, explicit geometry for batched views."""
    explicit = M is not None
    _dev(a, "a", contiguous=not explicit); _dev(bt, "bt", contiguous=not explicit); _dev(out, "out", contiguous=not explicit)
    _dev(w_scale, "w_scale")
    if M is None:
        M, K = a.shape
        N = bt.shape[0]
        if bt.shape[1] != K or out.shape[0] != M or out.shape[1] != N:
            raise RuntimeError(f"gemm_pairs: shapes {tuple(a.shape)} x {tuple(bt.shape)}^T -> {tuple(out.shape)}")
        lda, ldb, ldc = a.stride(0), bt.stride(0), out.stride(0)
    ep = _ep_ref(epilogue, "gemm_pairs")
    _check(lib().idiff_gemm_pairs_f32(a.data_ptr(), lda, stride_a, bt.data_ptr(), ldb, stride_b, w_scale.data_ptr(), int(bool(weight_is_a)),
                                      _ptr(act_scale), out.data_ptr(), ldc, stride_c, M, N, K, batch, ep, _stream()), "idiff_gemm_pairs_f32")
    return out


def pairs_act_scale(stats1, C1, stats2, C2, B, HW):
    """Device tensor whose first two floats are {s, 1 / s}, s the power of two that brings the root mean square of a tensor (or of
    cat[x1, x2]) into [0.71, 1.41), from the column sums ``stats = (ws, nsplit)`` its producing contraction(s) wrote."""
    out = torch.empty(8, device=stats1[0].device, dtype=torch.float32)
    _check(lib().idiff_pairs_act_scale_f32(stats1[0].data_ptr(), stats1[1], C1, _ptr(stats2[0]) if stats2 is not None else None,
                                           stats2[1] if stats2 is not None else 0, C2, B, HW, out.data_ptr(), _stream()),
           "idiff_pairs_act_scale_f32")
    return out


def gemm_pairs_2src(a1, a2, act_scale, bt, w_scale, out, epilogue=None):
    """out = epilogue([a1 | a2] @ bt.T) on fp16 pairs; ``act_scale`` from pairs_act_scale over both sources, ``w_scale`` from
    gemm_pairs_scale(bt)."""
    _dev(a1, "a1"); _dev(a2, "a2"); _dev(bt, "bt"); _dev(out, "out"); _dev(act_scale, "act_scale"); _dev(w_scale, "w_scale")
    M, K1 = a1.shape
    K = K1 + a2.shape[1]
    if a2.shape[0] != M or a1.stride(0) != a2.stride(0) or bt.shape[1] != K:
        raise RuntimeError(f"gemm_pairs_2src: shapes {tuple(a1.shape)} | {tuple(a2.shape)} x {tuple(bt.shape)}^T")
    ep = _ep_ref(epilogue, "gemm_pairs_2src")
    _check(lib().idiff_gemm_pairs_2src_f32(a1.data_ptr(), a2.data_ptr(), a1.stride(0), K1, act_scale.data_ptr(), bt.data_ptr(), bt.stride(0),
                                           w_scale.data_ptr(), out.data_ptr(), out.stride(0), M, bt.shape[0], K, ep, _stream()),
           "idiff_gemm_pairs_2src_f32")
    return out


def gemm_normed(cache, a, w, out, epilogue=None, pairs=True):
    """out = epilogue(a @ w.T) for ``a`` [M, K] = the output of a GroupNorm (order one by construction) and a weight ``w`` [N, K]:
    on fp16 pairs where that form serves the shape, else on gemm's six bf16 products.  ``cache``: a dict that lives as long as
    the weights (the executor's pack), holding each weight's power-of-two scale."""
    M, K = a.shape
    if not pairs or not gemm_pairs_ok(M, w.shape[0], K):     # `pairs`: the caller's range verdict (models/base.py: pairs_admissible)
        return gemm(a, w, out=out, epilogue=epilogue)
    return gemm_pairs(a, w, _pairs_scale_of(cache, w), out, epilogue=epilogue)


def _pairs_scale_of(cache, w):
    sc = cache.setdefault("pairs_scale", {})
    if id(w) not in sc:
        sc[id(w)] = (gemm_pairs_scale(w), w)                  # the weight itself keeps the id unique while the entry lives
    return sc[id(w)][0]


def gemm_weight_times_normed_t(cache, w, x, out, B, HW, C, pairs=True):
    """out[b] = w [C, C] @ x[b]^T for x [B, HW, C] = the output of a GroupNorm: V^T of an attention block, K-contiguous for P.V."""
    kw = dict(M=C, N=HW, K=C, lda=C, ldb=C, ldc=HW, batch=B, stride_a=0, stride_b=HW * C, stride_c=C * HW)
    if not pairs or not gemm_pairs_ok(C, HW, C, B):
        return gemm(w, x, out=out, **kw)
    return gemm_pairs(w, x, _pairs_scale_of(cache, w), out, weight_is_a=True, **kw)


def gemm_2src(a1, a2, bt, out, epilogue=None):
    """out = epilogue([a1 | a2] @ bt.T) for two sources [M, K1] and [M, K2], each with its own row pitch (concatenation never
    formed).  K1 % 32 == 0, K2 % 4 == 0."""
    _dev(a1, "a1"); _dev(a2, "a2"); _dev(bt, "bt"); _dev(out, "out")
    M, K1 = a1.shape
    K = K1 + a2.shape[1]
    if a2.shape[0] != M or bt.shape[1] != K:
        raise RuntimeError(f"gemm_2src: shapes {tuple(a1.shape)} | {tuple(a2.shape)} x {tuple(bt.shape)}^T")
    ep = _ep_ref(epilogue, "gemm_2src")
    _check(lib().idiff_gemm_2src_ld_f32(a1.data_ptr(), a1.stride(0), a2.data_ptr(), a2.stride(0), K1, bt.data_ptr(), bt.stride(0),
                                        out.data_ptr(), out.stride(0), M, bt.shape[0], K, ep, _stream()), "idiff_gemm_2src_ld_f32")
    return out


def gemm_2src_ld_ok(K1, K2):
    """Whether the executor takes gemm_2src for sources of K1 and K2 columns with different row pitches (K1 % 32 == 0, K2 % 4 == 0);
    no under IDIFF_NO_2SRC_PITCH and IDIFF_NO_PIPE.  Launches nothing."""
    return bool(lib().idiff_gemm_2src_ld_ok(K1, K2))


def conv2d_nhwc(x, wt, out, B, H, W, Cin, Cout, KH, KW, stride, pad, epilogue=None, pad_hi=None):
    ep = _ep_ref(epilogue, "conv2d_nhwc")
    _check(lib().idiff_conv2d_nhwc_f32(x.data_ptr(), wt.data_ptr(), out.data_ptr(), B, H, W, Cin, Cout, KH, KW, stride,
                                       pad, pad if pad_hi is None else pad_hi, ep, _stream()), "idiff_conv2d_nhwc_f32")
    return out


def _addr(t):
    return t if isinstance(t, int) else t.data_ptr()


def gemm_route(a, bt, out, M, N, K, lda, ldb, ldc, epilogue=None, batch=1, stride_a=0, stride_b=0, stride_c=0, pairs=False):
    """"<family> <tile> <arithmetic> <epilogue form>" of the launch ``gemm`` (``pairs``: ``gemm_pairs``) would make for these arguments
    (idiff_gemm_route), None if it refuses them.  a / bt / out: tensors or raw addresses (only null and 16-byte alignment matter);
    nothing is launched."""
    name = lib().idiff_gemm_route(_addr(a), lda, stride_a, _addr(bt), ldb, stride_b, _addr(out), ldc, stride_c, M, N, K, batch,
                                  _ep_ref(epilogue, "gemm_route"), int(bool(pairs)))
    return None if name is None else name.decode()


def conv2d_route(x, wt, out, B, H, W, Cin, Cout, KH, KW, stride, pad, epilogue=None, pad_hi=None):
    """The same for ``conv2d_nhwc`` (idiff_conv2d_route)."""
    name = lib().idiff_conv2d_route(_addr(x), _addr(wt), _addr(out), B, H, W, Cin, Cout, KH, KW, stride, pad, pad if pad_hi is None else pad_hi,
                                    _ep_ref(epilogue, "conv2d_route"))
    return None if name is None else name.decode()


# ---- Winograd convolutions.  Four kernel forms, named by the stem of their entry points (idiff_<stem>_weight_floats,
# idiff_<stem>_pack_f32, idiff_conv2d_<stem>_f32): winograd = F(2x2, 3x3) on the fp32 matrix cores, winograd43 / winograd43h = F(4x4, 3x3) on fp32 / on fp16 pairs, wino1d = F(4, 3) along the rows on fp16 pairs.
def _wino_pack(stem, name, wt, Cin, Cout):
    """wt [Cout, 3, 3, Cin] (the direct kernel's panel) -> the transformed filter bank of idiff_conv2d_<stem>_f32."""
    _dev(wt, "wt")
    if tuple(wt.shape) != (Cout, 3, 3, Cin):
        raise RuntimeError(f"{name}: expected {Cout}x3x3x{Cin} weights, got {tuple(wt.shape)}")
    entry = f"idiff_{stem}_pack_f32"
    u = torch.empty(getattr(lib(), f"idiff_{stem}_weight_floats")(Cin, Cout), device=wt.device, dtype=torch.float32)
    _check(getattr(lib(), entry)(wt.data_ptr(), u.data_ptr(), Cin, Cout, _stream()), entry)
    return u


def _wino_conv(stem, packed_by, x, u, out, B, H, W, Cin, Cout, epilogue):
    """One launch of idiff_conv2d_<stem>_f32.  The forms' banks differ in size, so a bank of another form is refused here
    (never reinterpreted) with the ``packed_by`` call that makes the right one."""
    want = getattr(lib(), f"idiff_{stem}_weight_floats")(Cin, Cout)
    if u.numel() != want:
        raise RuntimeError(f"conv2d_{stem}: a filter bank of {u.numel()} floats ({want} expected): pack it with {packed_by}")
    gn = getattr(epilogue, "groupnorm", None)
    nl = getattr(epilogue, "normload", None)
    ru = getattr(epilogue, "residual_up2", None)
    if ru is not None and stem == "wino1d":
        if gn is not None or nl is not None:
            raise RuntimeError("conv2d_wino1d: the upsampled residual (with_residual_up2) cannot be combined with a fused GroupNorm "
                               "(with_groupnorm) or one in the loader (with_normload)")
        if ru.lo.numel() != B * (H // 2) * (W // 2) * Cout:
            raise RuntimeError(f"conv2d_wino1d: a low-resolution residual of {ru.lo.numel()} floats for [B, (H/2)(W/2), Cout] = "
                               f"[{B}, {(H // 2) * (W // 2)}, {Cout}]")
        _check(lib().idiff_conv2d_wino1d_resup_f32(x.data_ptr(), u.data_ptr(), out.data_ptr(), B, H, W, Cin, Cout, ctypes.byref(epilogue),
                                                   ru.lo.data_ptr(), (ctypes.c_float * 16)(*ru.taps), _stream()), "idiff_conv2d_wino1d_resup_f32")
        return out
    if nl is not None and stem == "wino1d":
        if gn is not None:
            raise RuntimeError("conv2d_wino1d: a GroupNorm in the loader (with_normload) and one in the tail (with_groupnorm) in one launch")
        if nl.coef.numel() != B * Cin * 2:
            raise RuntimeError(f"conv2d_wino1d: {nl.coef.numel()} loader coefficients for [B, Cin, 2] = [{B}, {Cin}, 2]")
        if nl.x2 is not None:
            _check(lib().idiff_conv2d_wino1d_normload_2src_f32(x.data_ptr(), nl.C1, nl.x2.data_ptr(), Cin - nl.C1, u.data_ptr(), out.data_ptr(),
                                                               B, H, W, Cout, ctypes.byref(epilogue), nl.coef.data_ptr(), nl.act, _stream()),
                   "idiff_conv2d_wino1d_normload_2src_f32")
        else:
            _check(lib().idiff_conv2d_wino1d_normload_f32(x.data_ptr(), u.data_ptr(), out.data_ptr(), B, H, W, Cin, Cout, ctypes.byref(epilogue),
                                                          nl.coef.data_ptr(), nl.act, _stream()), "idiff_conv2d_wino1d_normload_f32")
        return out
    if gn is not None and stem == "wino1d":
        groups, gamma, beta, eps, act = gn
        if gamma.numel() != Cout or beta.numel() != Cout:
            raise RuntimeError(f"conv2d_wino1d: fused GroupNorm with {gamma.numel()} / {beta.numel()} gamma / beta entries for {Cout} channels")
        _check(lib().idiff_conv2d_wino1d_gn_f32(x.data_ptr(), u.data_ptr(), out.data_ptr(), B, H, W, Cin, Cout, ctypes.byref(epilogue), groups,
                                                gamma.data_ptr(), beta.data_ptr(), eps, act, _stream()), "idiff_conv2d_wino1d_gn_f32")
        return out
    ep = _ep_ref(epilogue, f"conv2d_{stem}")
    entry = f"idiff_conv2d_{stem}_f32"
    _check(getattr(lib(), entry)(x.data_ptr(), u.data_ptr(), out.data_ptr(), B, H, W, Cin, Cout, ep, _stream()), entry)
    return out


def conv2d_winograd_ok(B, H, W, Cin, Cout):
    return bool(lib().idiff_conv2d_winograd_ok(B, H, W, Cin, Cout))


def conv2d_winograd_colstats_split(B, H, W, Cin, Cout):
    return lib().idiff_conv2d_winograd_colstats_split(B, H, W, Cin, Cout)


def winograd_pack(wt, Cin, Cout):
    """The filter bank of idiff_conv2d_winograd_f32."""
    return _wino_pack("winograd", "winograd_pack", wt, Cin, Cout)


def conv2d_winograd(x, u, out, B, H, W, Cin, Cout, epilogue=None):
    """The bank must be the one ``winograd_pack`` made."""
    return _wino_conv("winograd", "winograd_pack", x, u, out, B, H, W, Cin, Cout, epilogue)


def conv2d_winograd43_ok(B, H, W, Cin, Cout):
    """True when the F(4x4, 3x3) kernel serves this geometry (asked per call: IDIFF_NO_WINO43 / IDIFF_NO_WINOGRAD switch it off)."""
    return bool(lib().idiff_conv2d_winograd43_ok(B, H, W, Cin, Cout))


def conv2d_winograd43h_ok(B, H, W, Cin, Cout):
    """True when the fp16-pair F(4x4, 3x3) kernel serves this geometry (IDIFF_NO_WINO43H and the fp32 form's switches turn it off)."""
    return bool(lib().idiff_conv2d_winograd43h_ok(B, H, W, Cin, Cout))


def conv2d_winograd43_colstats_split(B, H, W, Cin, Cout):
    return lib().idiff_conv2d_winograd43_colstats_split(B, H, W, Cin, Cout)


def winograd43_pack(wt, Cin, Cout, pairs=False):
    """The filter bank of idiff_conv2d_winograd43_f32 (36 * Cin * Cout floats), or with pairs=True that of idiff_conv2d_winograd43h_f32
    (scaled fp16 pairs, 36 * Cin * Cout + 4 floats)."""
    return _wino_pack("winograd43h" if pairs else "winograd43", "winograd43_pack", wt, Cin, Cout)


def conv2d_winograd43(x, u, out, B, H, W, Cin, Cout, epilogue=None, pairs=False):
    """pairs: `u` is a bank of fp16 pairs (winograd43_pack(..., pairs=True)) and the contraction runs on the fp16 matrix cores."""
    if pairs:
        return _wino_conv("winograd43h", "winograd43_pack(..., pairs=True)", x, u, out, B, H, W, Cin, Cout, epilogue)
    return _wino_conv("winograd43", "winograd43_pack", x, u, out, B, H, W, Cin, Cout, epilogue)


def conv2d_wino1d_ok(B, H, W, Cin, Cout):
    """True when the row-wise F(4, 3) kernel on fp16 pairs (csrc/wino1d.hip) serves this geometry (W in {4, 8, 16, 32, 64}; off under
    IDIFF_NO_WINOGRAD / IDIFF_NO_WINO43H / IDIFF_NO_WINO1D)."""
    return bool(lib().idiff_conv2d_wino1d_ok(B, H, W, Cin, Cout))


def conv2d_wino1d_colstats_split(B, H, W, Cin, Cout):
    return lib().idiff_conv2d_wino1d_colstats_split(B, H, W, Cin, Cout)


def conv2d_wino1d_gn_ok(B, H, W, Cin, Cout, groups):
    """True when conv2d_wino1d also applies the GroupNorm (``groups`` groups) + activation behind it (with_groupnorm): maps of at most 256
    pixels in rows of at most 16, group widths that divide 64; off under IDIFF_NO_FUSED_GN and wherever conv2d_wino1d_ok is."""
    return bool(lib().idiff_conv2d_wino1d_gn_ok(B, H, W, Cin, Cout, groups))


def conv2d_wino1d_resup_ok(B, H, W, Cin, Cout):
    """True where conv2d_wino1d adds a residual given at half the resolution, upsampled x2 in its tail (with_residual_up2): rows of 8, 16 or
    32 pixels, even H; off under IDIFF_NO_FUSED_RES_UP and wherever conv2d_wino1d_ok is."""
    return bool(lib().idiff_conv2d_wino1d_resup_ok(B, H, W, Cin, Cout))


def conv2d_wino1d_normload_ok(B, H, W, Cin, Cout):
    """True where conv2d_wino1d applies the GroupNorm (+ SiLU) in front of it in its loader (with_normload) and that was measured faster than
    the pass: rows of 32 pixels; off under IDIFF_NO_FUSED_GN_LOAD, IDIFF_NO_PAIRS and wherever conv2d_wino1d_ok is."""
    return bool(lib().idiff_conv2d_wino1d_normload_ok(B, H, W, Cin, Cout))


def conv2d_wino1d_normload_2src_ok(B, H, W, C1, C2, Cout):
    """The same for cat[x1, x2] read from its two sources (with_normload's x2, C1): whole K steps (16 channels) from each; off under
    IDIFF_NO_FUSED_GN_LOAD_2SRC (not under IDIFF_NO_FUSED_GN_LOAD), IDIFF_NO_PAIRS and wherever conv2d_wino1d_ok is."""
    return bool(lib().idiff_conv2d_wino1d_normload_2src_ok(B, H, W, C1, C2, Cout))


def groupnorm_coef(ws1, ns1, C1, ws2, ns2, C2, B, HW, G, eps, gamma, beta, coef):
    """coef [B, C1 + C2, 2] = (rstd gamma, beta - mean rstd gamma) from the producers' column sums (one launch, no pass over the activations)."""
    _dev(coef, "coef"); _dev(gamma, "gamma"); _dev(beta, "beta")
    if coef.numel() != B * (C1 + (C2 if ws2 is not None else 0)) * 2:
        raise RuntimeError(f"groupnorm_coef: coef holds {coef.numel()} floats, [B, C, 2] = {B * (C1 + C2) * 2} expected")
    _check(lib().idiff_groupnorm_coef_f32(ws1.data_ptr(), ns1, C1, _ptr(ws2), ns2, C2, B, HW, G, eps, gamma.data_ptr(), beta.data_ptr(),
                                          coef.data_ptr(), _stream()), "idiff_groupnorm_coef_f32")
    return coef


def groupnorm_reader_coef(ws, ns, C, B, HW, G, eps, gamma, beta, coef):
    """groupnorm_coef of one source for the readers that are not the convolution loader (upfirdn2d_gn): the same C entry, a name of its
    own so that the launches of either kind can be told apart."""
    _dev(coef, "coef"); _dev(gamma, "gamma"); _dev(beta, "beta")
    if coef.numel() != B * C * 2:
        raise RuntimeError(f"groupnorm_reader_coef: coef holds {coef.numel()} floats, [B, C, 2] = {B * C * 2} expected")
    _check(lib().idiff_groupnorm_coef_f32(ws.data_ptr(), ns, C, 0, 0, 0, B, HW, G, eps, gamma.data_ptr(), beta.data_ptr(),
                                          coef.data_ptr(), _stream()), "idiff_groupnorm_coef_f32")
    return coef


def wino1d_pack(wt, Cin, Cout):
    """The filter bank of idiff_conv2d_wino1d_f32 (scaled fp16 pairs of (G g[ky])[i], 18 * Cin * Cout + 4 floats)."""
    return _wino_pack("wino1d", "wino1d_pack", wt, Cin, Cout)


def conv2d_wino1d(x, u, out, B, H, W, Cin, Cout, epilogue=None):
    """``epilogue`` may carry a GroupNorm request (with_groupnorm): the launch then stores act(GroupNorm(conv + bias + rowbias)); or one for
    the loader (with_normload; with its x2, C1 ``x`` is the first source, ``Cin`` the total and the second travels in the request)."""
    return _wino_conv("wino1d", "wino1d_pack", x, u, out, B, H, W, Cin, Cout, epilogue)


# ------------------------------------------------------------------------------------------- norm / pointwise
def gemm_colstats_split(M, N, K, lda, ldb, rows_per_sample):
    return lib().idiff_gemm_colstats_split(M, N, K, lda, ldb, rows_per_sample)


def conv2d_colstats_split(B, H, W, Cin, Cout, KH, KW, stride, pad, pad_hi=None):
    return lib().idiff_conv2d_colstats_split(B, H, W, Cin, Cout, KH, KW, stride, pad, pad if pad_hi is None else pad_hi)


def groupnorm_finalize(ws1, nsplit1, C1, ws2, nsplit2, C2, B, HW, G, eps, stats):
    _check(lib().idiff_groupnorm_finalize_f32(ws1.data_ptr(), nsplit1, C1, _ptr(ws2), nsplit2, C2, B, HW, G, eps,
                                              stats.data_ptr(), _stream()), "idiff_groupnorm_finalize_f32")


def groupnorm_nsplit(B, HW, C):
    return lib().idiff_groupnorm_nsplit(B, HW, C)


def groupnorm_stats(x, C, x2, C2, B, HW, G, eps, workspace, stats):
    _check(lib().idiff_groupnorm_stats_f32(x.data_ptr(), C, _ptr(x2), C2, B, HW, G, eps, workspace.data_ptr(),
                                           stats.data_ptr(), _stream()), "idiff_groupnorm_stats_f32")


def groupnorm_apply(x, C, x2, C2, B, HW, G, stats, gamma, beta, act, y, mod=None):
    _check(lib().idiff_groupnorm_apply_f32(x.data_ptr(), C, _ptr(x2), C2, B, HW, G, stats.data_ptr(), gamma.data_ptr(),
                                           beta.data_ptr(), _ptr(mod), mod.stride(0) if mod is not None else 0,
                                           ACT[act], y.data_ptr(), _stream()),
           "idiff_groupnorm_apply_f32")


def groupnorm_apply_colstats(x, C, x2, C2, B, HW, G, ws1, ns1, ws2, ns2, eps, gamma, beta, act, y, mod=None):
    """GroupNorm apply whose statistics come from the producers' epilogue column sums (finalize + apply in one launch)."""
    _check(lib().idiff_groupnorm_apply_colstats_f32(x.data_ptr(), C, _ptr(x2), C2, B, HW, G, ws1.data_ptr(), ns1, _ptr(ws2), ns2,
                                                    eps, gamma.data_ptr(), beta.data_ptr(), _ptr(mod),
                                                    mod.stride(0) if mod is not None else 0, ACT[act], y.data_ptr(), _stream()),
           "idiff_groupnorm_apply_colstats_f32")


def _route(name):
    return None if name is None else name.decode()


def _addr0(t):
    """Address of a tensor, a raw address, or 0 for None: the route queries look at null and 16-byte alignment only."""
    return 0 if t is None else _addr(t)


def groupnorm_apply_route(x, C, x2, C2, B, HW, G, stats, gamma, beta, y):
    """"rows" or "flat": the kernel ``groupnorm_apply`` would launch for these arguments (idiff_groupnorm_apply_route), None if it
    refuses them.  Tensors or raw addresses; nothing is launched."""
    return _route(lib().idiff_groupnorm_apply_route(_addr0(x), C, _addr0(x2), C2, B, HW, G, _addr0(stats), _addr0(gamma), _addr0(beta),
                                                    _addr0(y)))


def groupnorm_apply_colstats_route(x, C, x2, C2, B, HW, G, ws1, ns1, ws2, ns2, gamma, beta, y):
    """The same for ``groupnorm_apply_colstats`` (idiff_groupnorm_apply_colstats_route): "rows", or None."""
    return _route(lib().idiff_groupnorm_apply_colstats_route(_addr0(x), C, _addr0(x2), C2, B, HW, G, _addr0(ws1), ns1, _addr0(ws2), ns2,
                                                             _addr0(gamma), _addr0(beta), _addr0(y)))


def softmax_rows(x, y, rows, cols, scale):
    _check(lib().idiff_softmax_rows_f32(x.data_ptr(), y.data_ptr(), rows, cols, scale, _stream()),
           "idiff_softmax_rows_f32")


def softmax_rows_route(x, y, rows, cols, scale):
    """"vec<1>" / "vec<2>" / "vec<4>" / "regs" / "stream" ("none" for rows == 0): the kernel, and for the general kernel the branch,
    that ``softmax_rows`` would run (idiff_softmax_rows_route); None if it refuses the arguments.  Nothing is launched."""
    return _route(lib().idiff_softmax_rows_route(_addr0(x), _addr0(y), rows, cols, scale))


def attention256_ok(B, tokens, C):
    """True when the one-launch attention serves this shape (256 tokens, 128 / 256 channels; off under IDIFF_NO_FUSED_ATTN / IDIFF_NO_PAIRS)."""
    return bool(lib().idiff_attention256_ok(B, tokens, C))


def pairs_scale_from_rows(w, bias=None, extra=1.0):
    """Device tensor {s, 1 / s}: the power of two that brings the output of ``w @ n + bias`` -- n a GroupNorm's output, unit variance per
    element by construction -- to a root mean square near one: rms^2 = mean_i |w_i|^2 (+ mean b^2).  Computed on the device, once per
    weight (no host synchronisation).  ``extra``: a known factor of the input's scale (GroupNorm gamma's rms)."""
    ms = (w.double() ** 2).sum(dim=1).mean() * float(extra) ** 2
    if bias is not None:
        ms = ms + (bias.double() ** 2).mean()
    e = torch.round(-0.5 * torch.log2(ms.clamp_min(1e-300))).clamp(-24, 24)
    s = torch.exp2(e)
    return torch.stack([s, 1.0 / s]).to(torch.float32).contiguous()


def attention256(qk, vt, out, B, C, s_qk, s_v, scale, bias_v=None):
    """out [B * 256, C] = softmax(q k^T * scale) v (+ bias_v) per sample; qk [B * 256, 2 C] (q | k), vt [B, C, 256]."""
    _dev(qk, "qk"); _dev(vt, "vt"); _dev(out, "out"); _dev(s_qk, "s_qk"); _dev(s_v, "s_v")
    if qk.shape != (B * 256, 2 * C) or vt.shape != (B, C, 256) or out.numel() != B * 256 * C:
        raise RuntimeError(f"attention256: shapes qk {tuple(qk.shape)}, vt {tuple(vt.shape)}, out {tuple(out.shape)} for B = {B}, C = {C}")
    _check(lib().idiff_attention256_f32(qk.data_ptr(), qk.stride(0), vt.data_ptr(), _ptr(bias_v), s_qk.data_ptr(), s_v.data_ptr(),
                                        out.data_ptr(), B, 256, C, float(scale), _stream()), "idiff_attention256_f32")
    return out


def attention_heads_ok(B, tokens, heads, D):
    """True when the streaming one-launch attention serves this shape (heads of 32 / 64 / 128 channels, tokens a multiple of 64 up to
    4096; off under IDIFF_NO_FUSED_ATTN / IDIFF_NO_PAIRS / IDIFF_NO_SPLIT)."""
    return bool(lib().idiff_attention_heads_ok(B, tokens, heads, D))


def attention_heads(qk, vt, out, B, tokens, heads, D, s_qk, s_v, scale, bias_v=None):
    """out [B * tokens, C] = per head softmax(q_h k_h^T * scale) v_h (+ bias_v), C = heads * D, head h in columns [h D, (h + 1) D) of
    q, k (qk [B * tokens, 2 C]: q | k) and out, rows [h D, (h + 1) D) of vt [B, C, tokens]."""
    _dev(qk, "qk"); _dev(vt, "vt"); _dev(out, "out"); _dev(s_qk, "s_qk"); _dev(s_v, "s_v")
    C = heads * D
    if bias_v is not None:
        _dev(bias_v, "bias_v")
    if (qk.shape != (B * tokens, 2 * C) or vt.shape != (B, C, tokens) or out.numel() != B * tokens * C
            or (bias_v is not None and bias_v.numel() != C) or s_qk.numel() < 2 or s_v.numel() < 2):
        raise RuntimeError(f"attention_heads: shapes qk {tuple(qk.shape)}, vt {tuple(vt.shape)}, out {tuple(out.shape)} for B = {B}, "
                           f"{tokens} tokens, {heads} heads of {D}")
    _check(lib().idiff_attention_heads_f32(qk.data_ptr(), qk.stride(0), vt.data_ptr(), _ptr(bias_v), s_qk.data_ptr(), s_v.data_ptr(),
                                           out.data_ptr(), B, tokens, heads, D, float(scale), _stream()), "idiff_attention_heads_f32")
    return out


def attention256_route(qk, ld_qk, vt, bias_v, s_qk, s_v, out, B, tokens, C):
    """"attention256<128>" / "attention256<256>" ("none" for B == 0): the instantiation ``idiff_attention256_f32`` would launch for these
    arguments (idiff_attention256_route), None if it refuses them.  Tensors or raw addresses; nothing is launched."""
    return _route(lib().idiff_attention256_route(_addr0(qk), ld_qk, _addr0(vt), _addr0(bias_v), _addr0(s_qk), _addr0(s_v), _addr0(out),
                                                 B, tokens, C))


def attention_heads_route(qk, ld_qk, vt, bias_v, s_qk, s_v, out, B, tokens, heads, D):
    """"heads<D,NW>" ("none" for B == 0): the same for ``idiff_attention_heads_f32`` (idiff_attention_heads_route)."""
    return _route(lib().idiff_attention_heads_route(_addr0(qk), ld_qk, _addr0(vt), _addr0(bias_v), _addr0(s_qk), _addr0(s_v), _addr0(out),
                                                    B, tokens, heads, D))


def affine_act(a, y, n, alpha=1.0, beta=0.0, act=None, rowscale=None, inner=0):
    _check(lib().idiff_affine_act_f32(a.data_ptr(), y.data_ptr(), n, alpha, beta, ACT[act], _ptr(rowscale), inner,
                                      _stream()), "idiff_affine_act_f32")


def affine_act_route(a, y, n, rowscale=None, inner=0):
    """"vec4" or "scalar" ("none" for n == 0): the kernel ``affine_act`` would launch (idiff_affine_act_route), None if it refuses."""
    return _route(lib().idiff_affine_act_route(_addr0(a), _addr0(y), n, _addr0(rowscale), inner))


def add_scale(a, b, y, n, scale):
    _check(lib().idiff_add_scale_f32(a.data_ptr(), b.data_ptr(), y.data_ptr(), n, scale, _stream()),
           "idiff_add_scale_f32")


def add_scale_route(a, b, y, n):
    """The same for ``add_scale`` (idiff_add_scale_route)."""
    return _route(lib().idiff_add_scale_route(_addr0(a), _addr0(b), _addr0(y), n))


def fourier_embed(t, W, out, B, half):
    _check(lib().idiff_fourier_embed_f32(t.data_ptr(), W.data_ptr(), out.data_ptr(), B, half, _stream()),
           "idiff_fourier_embed_f32")


def positional_embed(t, out, B, dim, max_positions=10000.0, mode=0):
    _check(lib().idiff_positional_embed_f32(t.data_ptr(), out.data_ptr(), B, dim, max_positions, mode, _stream()),
           "idiff_positional_embed_f32")


def concat_cols(a, Ca, b, Cb, out, rows):
    _check(lib().idiff_concat_cols_f32(a.data_ptr(), Ca, b.data_ptr(), Cb, out.data_ptr(), rows, _stream()),
           "idiff_concat_cols_f32")


def concat_cols_route(a, Ca, b, Cb, out, rows):
    """The same for ``concat_cols`` (idiff_concat_cols_route; "none" for rows == 0)."""
    return _route(lib().idiff_concat_cols_route(_addr0(a), Ca, _addr0(b), Cb, _addr0(out), rows))


def nchw_to_nhwc(x, y, B, C, HW, Cpad, alpha=1.0, beta=0.0):
    _check(lib().idiff_nchw_to_nhwc_f32(x.data_ptr(), y.data_ptr(), B, C, HW, Cpad, alpha, beta, _stream()),
           "idiff_nchw_to_nhwc_f32")


def nhwc_to_nchw(x, y, B, C, HW, Cpad, rowscale=None):
    _check(lib().idiff_nhwc_to_nchw_f32(x.data_ptr(), y.data_ptr(), B, C, HW, Cpad, _ptr(rowscale), _stream()),
           "idiff_nhwc_to_nchw_f32")


def perturb(x, z, std, mean_coeff, out, rows, D):
    _check(lib().idiff_perturb_f32(x.data_ptr(), z.data_ptr(), std.data_ptr(), _ptr(mean_coeff), out.data_ptr(), rows, D,
                                   _stream()), "idiff_perturb_f32")


def perturb_randn(x, std, mean_coeff, out, rows, D, row0, seed, z_out=None):
    _check(lib().idiff_perturb_randn_f32(x.data_ptr(), std.data_ptr(), _ptr(mean_coeff), out.data_ptr(), rows, D, row0,
                                         int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(z_out), _stream()), "idiff_perturb_randn_f32")


def resample2x_nhwc(x, y, B, H, W, C, up):
    _check(lib().idiff_resample2x_nhwc_f32(x.data_ptr(), y.data_ptr(), B, H, W, C, int(up), _stream()),
           "idiff_resample2x_nhwc_f32")


# ------------------------------------------------------------------------------------------- spectrum
def spectrum_workspace_bytes(P, M, D):
    return lib().idiff_spectrum_workspace_bytes(P, M, D)


def spectrum(S, workspace=None, return_eig=False, full=False):
    """Singular values (descending, fp32, min(M, D) of them as torch.linalg.svd gives) of the column-centred matrices
    S [P, M, D] or [M, D].  ``full=True`` keeps all D values of the Gram route (the drivers gather fixed-width rows and cut
    each point's list to its own min(M, D) on the host).  ``return_eig=True`` adds the Gram eigenvalues behind them (fp64,
    ASCENDING, the same count as the singular values: ``sv[i] == sqrt(max(eig[-1 - i], 0))``)."""
    _dev(S, "scores")
    squeeze = S.ndim == 2
    if squeeze:
        S = S.unsqueeze(0)
    if S.ndim != 3:
        raise RuntimeError("scores must be [M, D] or [P, M, D]")
    P, M, D = S.shape
    need = spectrum_workspace_bytes(P, M, D)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty((need + 7) // 8, dtype=torch.float64, device=S.device)
    sv = torch.empty(P, D, dtype=torch.float32, device=S.device)
    eig = torch.empty(P, D, dtype=torch.float64, device=S.device) if return_eig else None
    _check(lib().idiff_spectrum_f32(S.data_ptr(), P, M, D, workspace.data_ptr(),
                                    workspace.numel() * workspace.element_size(), sv.data_ptr(), _ptr(eig), _stream()),
           "idiff_spectrum_f32")
    if M < D and not full:
        sv = sv[:, :M].contiguous()           # the Gram route yields D values, the last D - M of them zeros up to rounding
        if eig is not None:
            eig = eig[:, D - M:].contiguous()  # ascending: the SAME M values as sv (sv[i]^2 = eig[M - 1 - i])
    if squeeze:
        sv = sv[0]
        eig = eig[0] if eig is not None else None
    return (sv, eig) if return_eig else sv


def symtridiag_plan(D):
    """0 LDS-resident, 1 two-stage + systolic chase, 2 two-stage + wavefront chase, 3 one-stage (include/idiff_hip.h)."""
    return lib().idiff_symtridiag_plan(int(D))


# The eigensolver never returns a silently wrong spectrum: a band-reduction residual above tolerance or a stalled systolic
# chase (its workgroups wait on each other; a device that cannot keep them all resident stalls it) poisons the outputs
# with NaN.  These are the slower forms that do not share the failure: tried in turn, in the same process.
_FALLBACKS = (("IDIFF_CHASE_WAVEFRONT", "bulge chasing one launch per wavefront"),
              ("IDIFF_TRIDIAG_ONESTAGE", "one-stage Householder sweep"))


def solve_with_fallbacks(solve, any_rank=None, log=None):
    """``solve()`` under each fallback form in turn, on the current stream, until one comes back without NaN; raises when none
    does.  Synchronises (the rare path).  ``any_rank``: with a process group, a callable that reduces the failure flag (a bool
    tensor -> a Python bool, true if it is set on any rank), so that every rank runs the same forms and returns the same result.
    ``log`` takes the one-line account of the form that served (default ``warnings.warn``)."""
    import warnings
    for name, what in _FALLBACKS:
        with thread_option(name, 1):                       # this thread's launches only
            out = solve()
        failed = torch.isnan(out).any()
        if not (any_rank(failed) if any_rank is not None else bool(failed)):
            msg = f"id-diff_amd: the two-stage eigensolver reported a failure; spectrum re-solved with {what} ({name})"
            (log or warnings.warn)(msg)
            return out
    raise RuntimeError("the eigensolver reported a failure (NaN) in all of its three forms: two-stage with the systolic chase, with "
                       "the wavefront chase, and the one-stage sweep")


def resolve_failed_spectrum(S, full=False, log=None):
    """``spectrum(S)`` came back with NaN: solve the same matrices again with the fallback forms of the eigensolver, on
    the current stream.  Synchronises (the rare path).  Raises if S itself is non-finite or every form fails."""
    if not bool(torch.isfinite(S).all()):
        raise RuntimeError("the score matrix holds non-finite values (NaN / inf score vectors): no spectrum exists")
    return solve_with_fallbacks(lambda: spectrum(S, full=full), log=log)


# ---- the stages of the spectrum, for the row-sharded single-point pipeline (dim_reduction.row_sharded_spectrum)
def column_sums(S):
    """fp64 column sums [D] of S [M, D] (two-stage, deterministic: idiff_colmean_f64 times M)."""
    _dev(S, "scores")
    M, D = S.shape
    if M == 0:
        return torch.zeros(D, dtype=torch.float64, device=S.device)
    mean = torch.empty(D, dtype=torch.float64, device=S.device)
    scratch = torch.empty(32 * D, dtype=torch.float64, device=S.device)
    _check(lib().idiff_colmean_f64(S.data_ptr(), 1, M, D, mean.data_ptr(), scratch.data_ptr(), _stream()), "idiff_colmean_f64")
    return mean * M


def centered_gram(S, mean):
    """fp64 Gram [D, D] of the rows of S [M, D] after subtracting ``mean`` [D] (fp64): sum_i (s_i - mean)(s_i - mean)^T."""
    _dev(S, "scores"); _dev(mean, "mean", dtype=torch.float64)
    M, D = S.shape
    if M == 0:
        return torch.zeros(D, D, dtype=torch.float64, device=S.device)
    G = torch.empty(D, D, dtype=torch.float64, device=S.device)
    _check(lib().idiff_centered_gram_f64(S.data_ptr(), mean.data_ptr(), 1, M, D, G.data_ptr(), _stream()), "idiff_centered_gram_f64")
    return G


def centered_gram_rows(S, mean, G, row0, row1):
    """Upper-triangle rows [row0, row1) of the centred Gram into the (pre-zeroed) [D, D] fp64 matrix G."""
    _dev(S, "scores"); _dev(mean, "mean", dtype=torch.float64); _dev(G, "G", dtype=torch.float64)
    M, D = S.shape
    if M == 0:
        return G
    _check(lib().idiff_centered_gram_rows_f64(S.data_ptr(), mean.data_ptr(), M, D, row0, row1, G.data_ptr(), _stream()),
           "idiff_centered_gram_rows_f64")
    return G


def symmetrize_upper(G):
    _dev(G, "G", dtype=torch.float64)
    _check(lib().idiff_symmetrize_upper_f64(G.data_ptr(), G.shape[0], _stream()), "idiff_symmetrize_upper_f64")
    return G


def sym_band(G, dense=True):
    """Stage 1 of the two-stage eigensolver alone (G is overwritten).  ``dense=True``: the dense symmetric band matrix
    [D, D] (half-width 32) similar to G, for the parity tests; ``dense=False``: the compact band [D, ld] with
    band[j, k] = B[j + k, j], for timing."""
    _dev(G, "G", dtype=torch.float64)
    D = G.shape[0]
    scratch = torch.empty(lib().idiff_symtridiag_scratch_doubles(D), dtype=torch.float64, device=G.device)   # stage 1 writes the band AND its bulge room
    _check(lib().idiff_symband_f64(G.data_ptr(), D, scratch.data_ptr(), _stream()), "idiff_symband_f64")
    ld = lib().idiff_symband_ld()
    band = scratch[:D * ld].view(D, ld)                       # band[j, k] = B[j + k, j]
    if not dense:
        return band
    B = torch.zeros(D, D, dtype=torch.float64, device=G.device)
    j = torch.arange(D, device=G.device)
    for k in range(ld):
        n = D - k
        if n <= 0:
            break
        B[j[:n] + k, j[:n]] = band[:n, k]
        B[j[:n], j[:n] + k] = band[:n, k]
    return B


def sym_eigvals(G):
    """Eigenvalues (ascending, fp64) of a symmetric fp64 matrix [D, D]; G is overwritten (Householder + Sturm bisection)."""
    _dev(G, "G", dtype=torch.float64)
    D = G.shape[0]
    diag = torch.empty(D, dtype=torch.float64, device=G.device)
    offd = torch.empty(D, dtype=torch.float64, device=G.device)
    scratch = torch.empty(max(1, lib().idiff_symtridiag_scratch_doubles(D)), dtype=torch.float64, device=G.device)
    eig = torch.empty(D, dtype=torch.float64, device=G.device)
    _check(lib().idiff_symtridiag_f64(G.data_ptr(), 1, D, diag.data_ptr(), offd.data_ptr(), scratch.data_ptr(), _stream()),
           "idiff_symtridiag_f64")
    _check(lib().idiff_tridiag_eigvals_f64(diag.data_ptr(), offd.data_ptr(), 1, D, eig.data_ptr(), _stream()), "idiff_tridiag_eigvals_f64")
    return eig


TANGENT_MAX = 128      # widest basis idiff_sym_lowvecs_f64 serves


def sym_lowvecs(G, k):
    """``(T, ritz, resid)`` of a symmetric positive semi-definite fp64 matrix G [D, D]: T [D, k] fp64 with orthonormal columns
    spanning the invariant subspace of the k smallest eigenvalues, ritz [k] fp64 ascending (column i of T belongs to ritz[i]),
    resid a 0-d fp64 tensor |G T - T diag(ritz)|_F.  1 <= k <= 128, k < D.  G is only read; trouble (G not positive
    semi-definite to rounding, a NaN in G) comes back as NaN in all three.  No host sync."""
    _dev(G, "G", dtype=torch.float64)
    if G.ndim != 2 or G.shape[0] != G.shape[1]:
        raise RuntimeError(f"sym_lowvecs: G must be [D, D], got {tuple(G.shape)}")
    D, k = G.shape[0], int(k)
    scratch = torch.empty(max(1, lib().idiff_sym_lowvecs_scratch_doubles(D, k)), dtype=torch.float64, device=G.device)
    ok = 1 <= k < D
    T = torch.empty((D, k) if ok else (1,), dtype=torch.float64, device=G.device)
    ritz = torch.empty(k if ok else 1, dtype=torch.float64, device=G.device)
    resid = torch.empty((), dtype=torch.float64, device=G.device)
    _check(lib().idiff_sym_lowvecs_f64(G.data_ptr(), D, k, T.data_ptr(), ritz.data_ptr(), resid.data_ptr(), scratch.data_ptr(), _stream()),
           "idiff_sym_lowvecs_f64")
    return T, ritz, resid



# ------------------------------------------------------------------------------------------- largest eigenpairs
TOPVECS_MAX = 64                  # most eigenpairs idiff_sym_topvecs_f64 returns
TOPVECS_BLOCK_MAX = 128           # widest block it iterates on
TOPVECS_OVERSAMPLING = 16         # fewest columns beyond k (max(16, k) are taken): the filter's upper end is lambda_(p + 1), not lambda_(k + 1)
TOPVECS_AMPLIFICATION = 1e6       # bound of C_m(lambda_1) / C_m(lambda_k) per sweep: column k keeps 10 of its 16 digits
TOPVECS_BLOCK_AMPLIFICATION = 1e10   # the same for the last column of the block (it need only stay a direction)
TOPVECS_DEGREE_MAX = 32
TOPVECS_TARGET = 1e13             # total damping of lambda_(p+1) against lambda_k the sweeps must reach
TOPVECS_PRODUCTS_MAX = 1000       # matrix products (degree * sweeps) a plan may ask for


def _log_cheb(m, x):
    """log T_m(x) for x >= 1, without forming T_m (which overflows a double beyond m acosh(x) = 710)."""
    import math
    a = m * math.acosh(x) if x > 1.0 else 0.0
    return a + math.log1p(math.exp(-2.0 * a)) - math.log(2.0)


def topvecs_plan(eigvals, k):
    """The fixed schedule of ``sym_topvecs`` from ALL eigenvalues of the matrix (any order; host numpy): a dict with the block
    width ``p`` = min(k + max(16, k), 128, N - 1) (a wide block keeps lambda_(p+1) well below lambda_k where the spectrum decays
    slowly), the filter interval ``lo`` = lambda_min, ``hi`` = lambda_(p+1), ``top`` = lambda_1 (for
    p = N - 1, where the two ends coincide, lo = hi - (top - hi)), the
    Chebyshev ``degree`` per sweep, the number of ``sweeps``, ``products`` = degree * sweeps and ``amplification`` =
    C_m(lambda_1) / C_m(lambda_k), the factor by which one sweep lifts column 1 over column k.  The degree is, among those (up to 32)
    that keep that factor below 1e6 (and the same factor for the block's last column below 1e10), the one with the fewest products: a filter that lifts lambda_1
    by 1e40 over lambda_3 leaves nothing of column 3 in fp64.  The sweeps are as many as damp lambda_(p+1) by 1e13 against
    lambda_k, plus one.  Pure host arithmetic.  Raises ``ValueError`` when lambda_k is not positive (above 1e-12 of lambda_1, the
    rule of ``isomap.n_positive``) or when the schedule would need more than 1000 matrix products (a flat spectrum from lambda_k
    to lambda_(p+1))."""
    import math
    import numpy as np
    lam = np.sort(np.asarray(eigvals, dtype=np.float64).reshape(-1))[::-1]
    N, k = lam.size, int(k)
    if not 1 <= k <= TOPVECS_MAX or k >= N:
        raise ValueError(f"topvecs_plan: k = {k} outside 1..min({TOPVECS_MAX}, N - 1 = {N - 1})")
    if not np.isfinite(lam).all():
        raise ValueError("topvecs_plan: the eigenvalues hold NaN or inf")
    if not (lam[0] > 0 and lam[k - 1] > 1e-12 * lam[0]):
        raise ValueError(f"topvecs_plan: lambda_{k} = {float(lam[k - 1])!r} is not positive (lambda_1 = {float(lam[0])!r}): the matrix has "
                         f"{int(np.count_nonzero(lam > 1e-12 * lam[0])) if lam[0] > 0 else 0} positive eigenvalues")
    p = min(k + max(TOPVECS_OVERSAMPLING, k), TOPVECS_BLOCK_MAX, N - 1)
    lo, hi, top = float(lam[-1]), float(lam[p]), float(lam[0])
    if p == N - 1:                                   # lambda_(p+1) is lambda_min itself: an interval as wide below it as lambda_1 is above
        lo = hi - (top - hi)
    flat = (f"topvecs_plan: lambda_{k} = {float(lam[k - 1])!r} and lambda_{p + 1} = {hi!r} (lambda_1 = {top!r}, lambda_min = {lo!r}) are too "
            f"close: separating them needs more than {TOPVECS_PRODUCTS_MAX} matrix products")
    c, e = 0.5 * (hi + lo), 0.5 * (hi - lo)
    if not e > 0:
        raise ValueError(flat)
    x1, xk, xp = (top - c) / e, (float(lam[k - 1]) - c) / e, (float(lam[p - 1]) - c) / e
    log_amp, log_block = math.log(TOPVECS_AMPLIFICATION), math.log(TOPVECS_BLOCK_AMPLIFICATION)
    allowed = 1                                      # degrees 1 .. allowed keep both amplifications within their bounds
    while (allowed < TOPVECS_DEGREE_MAX and _log_cheb(allowed + 1, x1) - _log_cheb(allowed + 1, xk) <= log_amp
           and _log_cheb(allowed + 1, x1) - _log_cheb(allowed + 1, xp) <= log_block):
        allowed += 1
    if not _log_cheb(allowed, xk) > 1e-12:
        raise ValueError(flat)
    sweeps_of = lambda m: max(2, int(math.ceil(math.log(TOPVECS_TARGET) / _log_cheb(m, xk))) + 1)
    degree = min(range(1, allowed + 1), key=lambda m: (m * sweeps_of(m), m))        # the fewest products, the lower degree among equals
    sweeps, log_gain = sweeps_of(degree), _log_cheb(degree, xk)
    if degree * sweeps > TOPVECS_PRODUCTS_MAX:
        raise ValueError(flat)
    return {"p": p, "lo": lo, "hi": hi, "top": top, "degree": degree, "sweeps": sweeps, "products": degree * sweeps,
            "amplification": math.exp(min(_log_cheb(degree, x1) - log_gain, 700.0))}


def sym_topvecs(K, k, eigvals, plan=None):
    """``(V, ritz, resid)`` of a symmetric fp64 matrix K [N, N] that may be indefinite: V [N, k] fp64 with orthonormal columns, the
    eigenvectors of the k LARGEST eigenvalues, ritz [k] fp64 descending, resid a 0-d fp64 tensor |K V - V diag(ritz)|_F.
    ``eigvals``: all N eigenvalues as a host array (``sym_eigvals(K.clone()).cpu()``), from which ``topvecs_plan`` fixes the
    schedule (``plan``: that plan, when the caller has made it already); 1 <= k <= 64, k < N.  K is only read; a NaN in K or a failed factorisation comes back as NaN in all three.
    No host sync."""
    N = _square_f64(K, "K")
    k = int(k)
    if len(eigvals) != N:
        raise ValueError(f"sym_topvecs: {len(eigvals)} eigenvalues for a {N} x {N} matrix")
    if plan is None:
        plan = topvecs_plan(eigvals, k)
    p = plan["p"]
    scratch = torch.empty(max(1, lib().idiff_sym_topvecs_scratch_doubles(N, k, p)), dtype=torch.float64, device=K.device)
    V = torch.empty(N, k, dtype=torch.float64, device=K.device)
    ritz = torch.empty(k, dtype=torch.float64, device=K.device)
    resid = torch.empty((), dtype=torch.float64, device=K.device)
    _check(lib().idiff_sym_topvecs_f64(K.data_ptr(), N, k, p, plan["lo"], plan["hi"], plan["top"], plan["degree"], plan["sweeps"],
                                       V.data_ptr(), ritz.data_ptr(), resid.data_ptr(), scratch.data_ptr(), _stream()),
           "idiff_sym_topvecs_f64")
    return V, ritz, resid


def tangent_basis(S, k):
    """The estimated tangent space at a point from its score matrix S [M, D] (CUDA fp32): the k right singular vectors of the
    column-centred S with the SMALLEST singular values, through the fp64 Gram matrix the spectrum is computed from
    (idiff_colmean_f64 -> idiff_centered_gram_f64 -> sym_lowvecs).  Returns what ``sym_lowvecs`` returns; ritz[i] is the
    square of the singular value that column i of T belongs to."""
    _dev(S, "scores")
    if S.ndim != 2 or S.shape[0] < 1:
        raise RuntimeError(f"tangent_basis: scores must be [M >= 1, D], got {tuple(S.shape)}")
    M, D = S.shape
    mean = torch.empty(D, dtype=torch.float64, device=S.device)
    scratch = torch.empty(32 * D, dtype=torch.float64, device=S.device)
    _check(lib().idiff_colmean_f64(S.data_ptr(), 1, M, D, mean.data_ptr(), scratch.data_ptr(), _stream()), "idiff_colmean_f64")
    return sym_lowvecs(centered_gram(S, mean), k)


# ------------------------------------------------------------------------------------------- k nearest neighbours
def knn(X, k, workspace=None):
    """Exact k nearest OTHER rows of every row of X [N, D] (CUDA fp32, contiguous): ``(dist, idx, n_exact_rows)`` with
    dist [N, k] fp64 (Euclidean, ascending; equal distances by lower index), idx [N, k] int64 and n_exact_rows a 0-d int32
    device tensor (rows the kernel settled by fp64 brute force).  No host sync."""
    _dev(X, "X")
    if X.ndim != 2:
        raise RuntimeError(f"knn: X must be [N, D], got {tuple(X.shape)}")
    N, D = X.shape
    k = int(k)
    need = lib().idiff_knn_workspace_bytes(N, D, k)
    if need > 0 and (workspace is None or workspace.numel() * workspace.element_size() < need):
        workspace = torch.empty((need + 7) // 8, dtype=torch.float64, device=X.device)
    dist = torch.empty(N, k, dtype=torch.float64, device=X.device) if N > 0 and k > 0 else torch.empty(0, device=X.device)
    idx = torch.empty(N, k, dtype=torch.int64, device=X.device) if N > 0 and k > 0 else torch.empty(0, device=X.device)
    n_exact = torch.zeros((), dtype=torch.int32, device=X.device)
    _check(lib().idiff_knn_f32(X.data_ptr(), N, D, k, _ptr(workspace), 0 if workspace is None else workspace.numel() * 8,
                               dist.data_ptr(), idx.data_ptr(), n_exact.data_ptr(), _stream()), "idiff_knn_f32")
    return dist, idx, n_exact


# ------------------------------------------------------------------------------------------- local PCA
def local_pca(X, centre, idx, n_vectors=0):
    """Spectrum and leading eigenvectors of the sample covariance of every neighbourhood {centre[q]} + idx[q, :] of X [N, D]
    (CUDA fp32, contiguous; centre [Q] and idx [Q, k] int64, 2 <= k <= 64): ``(eig, basis)`` with eig [Q, min(k, D)] fp64
    descending and basis [Q, n_vectors, D] fp64 (unit rows, largest component positive, NaN where the eigenvalue is zero to
    rounding), or None for n_vectors = 0 (idiff_local_pca_f64, one launch).  The kernel checks every index against [0, N)
    before it reads a row.  One host sync: the per-query status, read back to raise ``RuntimeError`` naming how many queries
    did not converge, held an index out of range or met a NaN or Inf in their rows."""
    _dev(X, "X"); _dev(centre, "centre", dtype=torch.int64); _dev(idx, "idx", dtype=torch.int64)
    if X.ndim != 2 or centre.ndim != 1 or idx.ndim != 2 or idx.shape[0] != centre.shape[0]:
        raise RuntimeError(f"local_pca: X must be [N, D], centre [Q] and idx [Q, k], got {tuple(X.shape)}, {tuple(centre.shape)} "
                           f"and {tuple(idx.shape)}")
    (N, D), (Q, k), nv = X.shape, idx.shape, int(n_vectors)
    r = min(k, D)
    eig = torch.empty(Q, r, dtype=torch.float64, device=X.device)
    basis = torch.empty(Q, nv, D, dtype=torch.float64, device=X.device) if nv > 0 else None
    status = torch.empty(Q, dtype=torch.int32, device=X.device)
    if Q == 0:                        # nothing to launch (and no pointers to pass); the sizes are still the library's to refuse
        if not lib().idiff_local_pca_ok(N, D, k, nv):
            raise RuntimeError(f"local_pca: N = {N}, D = {D}, k = {k}, n_vectors = {nv} not served (idiff_local_pca_ok)")
        return eig, basis
    _check(lib().idiff_local_pca_f64(X.data_ptr(), N, D, centre.data_ptr(), idx.data_ptr(), Q, k, nv, eig.data_ptr(), _ptr(basis),
                                     status.data_ptr(), _stream()), "idiff_local_pca_f64")
    st = status.cpu()
    stalled, outside, nonfinite = int((st == 1).sum()), int((st == 2).sum()), int((st == 3).sum())
    if stalled or outside or nonfinite:
        raise RuntimeError(f"local_pca: {stalled} of {Q} queries reached the Jacobi sweep cap without converging, "
                           f"{outside} hold an index outside [0, {N}), {nonfinite} have a neighbourhood that is not finite (NaN or Inf in X)")
    return eig, basis


# ------------------------------------------------------------------------------------------- simplex skewness
def simplex_skewness(X, centre, idx, scales):
    """Expected Simplex Skewness (d = 1) of every neighbourhood {centre[q]} + idx[q, :scales[s]] of X [N, D] (CUDA fp32,
    contiguous; centre [Q] and idx [Q, k] int64 in ascending distance, 2 <= k <= 64; scales: 1 to 16 ints, strictly ascending,
    2 <= scales[s] <= k): ess [Q, S, 3] fp64 = the weighted mean of |sin|, the weighted mean of |cos| and the weight sum over all
    pairs of the rows centred on their mean (idiff_simplex_skewness_f64, one launch).  The kernel checks every index against
    [0, N) before it reads a row.  One host sync: the per-query status, read back to raise ``RuntimeError`` naming how many
    queries held an index out of range or met a NaN or Inf in their rows.  A scale whose rows are identical (status 4) does not
    raise: its two means are NaN and its weight sum 0."""
    _dev(X, "X"); _dev(centre, "centre", dtype=torch.int64); _dev(idx, "idx", dtype=torch.int64)
    if X.ndim != 2 or centre.ndim != 1 or idx.ndim != 2 or idx.shape[0] != centre.shape[0]:
        raise RuntimeError(f"simplex_skewness: X must be [N, D], centre [Q] and idx [Q, k], got {tuple(X.shape)}, "
                           f"{tuple(centre.shape)} and {tuple(idx.shape)}")
    (N, D), (Q, k) = X.shape, idx.shape
    scales = [int(s) for s in scales]
    S = len(scales)
    host_scales = (c_i * max(S, 1))(*scales)
    ess = torch.empty(Q, S, 3, dtype=torch.float64, device=X.device)
    status = torch.empty(Q, dtype=torch.int32, device=X.device)
    if Q == 0:                        # nothing to launch (and no pointers to pass); the sizes are still the library's to refuse
        if not lib().idiff_simplex_skewness_ok(N, D, k, S):
            raise RuntimeError(f"simplex_skewness: N = {N}, D = {D}, k = {k}, {S} scales not served (idiff_simplex_skewness_ok)")
        return ess
    _check(lib().idiff_simplex_skewness_f64(X.data_ptr(), N, D, centre.data_ptr(), idx.data_ptr(), Q, k,
                                            ctypes.cast(host_scales, c_p), S, ess.data_ptr(), status.data_ptr(), _stream()),
           "idiff_simplex_skewness_f64")
    st = status.cpu()
    outside, nonfinite = int((st == 2).sum()), int((st == 3).sum())
    if outside or nonfinite:
        raise RuntimeError(f"simplex_skewness: {outside} of {Q} queries hold an index outside [0, {N}), "
                           f"{nonfinite} have a neighbourhood that is not finite (NaN or Inf in X)")
    return ess


# ------------------------------------------------------------------------------------------- geodesic distances (Isomap)
def __getattr__(name):
    """``_lib.APSP_TILE``: the tile of the blocked Floyd-Warshall, asked of the library (idiff_apsp_tile; the edge cases of the
    tests sit around it).  ``_lib.LOCAL_PCA_CHUNK``: the columns of X one step of local_pca gathers (idiff_local_pca_chunk)."""
    if name == "APSP_TILE":
        return lib().idiff_apsp_tile()
    if name == "LOCAL_PCA_CHUNK":
        return lib().idiff_local_pca_chunk()
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _square_f64(M, name):
    _dev(M, name, dtype=torch.float64)
    if M.ndim != 2 or M.shape[0] != M.shape[1] or M.shape[0] < 1:
        raise RuntimeError(f"{name} must be [N, N] with N >= 1, got {tuple(M.shape)}")
    return M.shape[0]


def knn_graph(dist, idx):
    """Dense neighbourhood graph G [N, N] fp64 of a ``knn`` result (dist [N, k] fp64, idx [N, k] int64): 0 on the diagonal,
    the distance where either point is among the other's neighbours (the smaller where both are), +inf elsewhere -- the graph
    ``scipy.sparse.csgraph.shortest_path(directed=False)`` reads from sklearn's ``kneighbors_graph``.  No host sync."""
    _dev(dist, "dist", dtype=torch.float64); _dev(idx, "idx", dtype=torch.int64)
    if dist.ndim != 2 or dist.shape != idx.shape:
        raise RuntimeError(f"knn_graph: dist and idx must both be [N, k], got {tuple(dist.shape)} and {tuple(idx.shape)}")
    N, k = dist.shape
    G = torch.empty(max(N, 1), max(N, 1), dtype=torch.float64, device=dist.device)
    _check(lib().idiff_knn_graph_f64(_ptr(dist), _ptr(idx), N, k, G.data_ptr(), _stream()), "idiff_knn_graph_f64")
    return G


def geodesic_distances(G):
    """All-pairs shortest paths of the dense graph G [N, N] fp64 (non-negative weights, 0 diagonal, +inf = no edge), IN PLACE
    (blocked Floyd-Warshall, idiff_apsp_f64); returns G.  Unreachable pairs stay +inf.  No host sync."""
    N = _square_f64(G, "G")
    _check(lib().idiff_apsp_f64(G.data_ptr(), N, _stream()), "idiff_apsp_f64")
    return G


def double_center(D, return_means=False):
    """``(K, fro2)`` of a symmetric distance matrix D [N, N] fp64 (only read): K = -1/2 J (D o D) J fp64 [N, N] and the 0-d
    fp64 device tensor ||K||_F^2.  ``return_means=True`` adds ``(colmean [N], grand 0-d)``, the column means and the grand mean
    of -1/2 D o D (what ``isomap_project`` centres a new point's row with).  No host sync."""
    N = _square_f64(D, "D")
    K = torch.empty_like(D)
    fro2 = torch.empty((), dtype=torch.float64, device=D.device)
    scratch = torch.empty(max(1, lib().idiff_double_center_scratch_doubles(N)), dtype=torch.float64, device=D.device)
    _check(lib().idiff_double_center_f64(D.data_ptr(), N, K.data_ptr(), fro2.data_ptr(), scratch.data_ptr(), _stream()),
           "idiff_double_center_f64")
    if return_means:
        return K, fro2, (-0.5 * scratch[:N], -0.5 * scratch[2 * N])
    return K, fro2


# ------------------------------------------------------------------------------------------- a disconnected graph, joined
# bridge endpoints / N up to which repair_geodesics updates the matrix (above: a second full solve).  NOT MEASURED yet: by operation
# count the update is 10 % cheaper up to 0.54 (scripts/isomap_connect_bench.py measures it, profiles/isomap_connect_bench.txt)
UPDATE_MAX_ENDPOINT_FRACTION = 0.5


def component_labels(D):
    """``(labels, count)`` of a shortest-path matrix D [N, N] fp64 (only read): labels [N] int32, 0 .. C - 1 in the order of each
    component's smallest vertex, and the 0-d int32 device tensor C.  Two vertices share a component exactly when their distance is
    finite.  No host sync."""
    N = _square_f64(D, "D")
    labels = torch.empty(N, dtype=torch.int32, device=D.device)
    count = torch.empty((), dtype=torch.int32, device=D.device)
    scratch = torch.empty(N, dtype=torch.int32, device=D.device)
    _check(lib().idiff_component_labels_f64(D.data_ptr(), N, labels.data_ptr(), count.data_ptr(), scratch.data_ptr(), _stream()),
           "idiff_component_labels_f64")
    return labels, count


def component_bridges(X, labels, C):
    """The edges scikit-learn joins C components with: ``(i, j, w)``, int64 [B], int64 [B], fp64 [B] device tensors, B = C (C - 1) / 2.
    For every component i and every j < i (position i (i - 1) / 2 + j) the point i[.] of component i and the point j[.] of
    component j at the smallest Euclidean distance w[.] (fp64 from the fp32 rows of X [N, D]); exact ties by the smallest i[.], then
    the smallest j[.].  labels [N] int32 as ``component_labels`` writes them.  2 <= C <= 1024.  No host sync."""
    _dev(X, "X"); _dev(labels, "labels", dtype=torch.int32)
    if X.ndim != 2 or labels.shape != (X.shape[0],):
        raise RuntimeError(f"component_bridges: X must be [N, D] and labels [N], got {tuple(X.shape)} and {tuple(labels.shape)}")
    (N, D), C = X.shape, int(C)
    B = max(C * (C - 1) // 2, 1)
    ws = torch.empty(max(1, lib().idiff_component_bridges_workspace_bytes(C) // 8), dtype=torch.int64, device=X.device)
    bi = torch.empty(B, dtype=torch.int64, device=X.device)
    bj = torch.empty(B, dtype=torch.int64, device=X.device)
    bw = torch.empty(B, dtype=torch.float64, device=X.device)
    _check(lib().idiff_component_bridges_f64(X.data_ptr(), N, D, labels.data_ptr(), C, ws.data_ptr(), ws.numel() * 8, bi.data_ptr(),
                                             bj.data_ptr(), bw.data_ptr(), _stream()), "idiff_component_bridges_f64")
    return bi, bj, bw


def minplus(A, B, C):
    """C = min(C, A (x) B) in place, the (min, +) product of A [m, p] and B [p, n] into C [m, n] (fp64; each may be a view with
    unit column stride; C may not overlap A or B); returns C.  No host sync."""
    for t, name in ((A, "A"), (B, "B"), (C, "C")):
        _dev(t, name, dtype=torch.float64, contiguous=False)
        if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1 or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
            raise RuntimeError(f"minplus: {name} must be a non-empty matrix with unit column stride, got shape {tuple(t.shape)}, strides {t.stride()}")
    (m, p), n = A.shape, B.shape[1]
    if B.shape[0] != p or C.shape != (m, n):
        raise RuntimeError(f"minplus: shapes {tuple(A.shape)} (x) {tuple(B.shape)} -> {tuple(C.shape)}")
    ld = lambda t: max(t.stride(0), t.shape[1]) if t.shape[0] > 1 else t.shape[1]
    _check(lib().idiff_minplus_f64(A.data_ptr(), ld(A), B.data_ptr(), ld(B), C.data_ptr(), ld(C), m, n, p, _stream()), "idiff_minplus_f64")
    return C


def symmetrize_min(G):
    """G = min(G, G^T) in place (G [N, N] fp64); returns G.  No host sync."""
    N = _square_f64(G, "G")
    _check(lib().idiff_symmetrize_min_f64(G.data_ptr(), N, _stream()), "idiff_symmetrize_min_f64")
    return G


def _min_edges(G, bi, bj, bw):
    """The undirected edges (bi, bj, bw) min-ed into the square matrix G (B <= C (C - 1) / 2 single entries; the pairs are distinct)."""
    G[bi, bj] = torch.minimum(G[bi, bj], bw)
    G[bj, bi] = torch.minimum(G[bj, bi], bw)
    return G


def repair_geodesics(D0, bi, bj, bw, route=None, knn=None):
    """All-pairs shortest paths of the graph behind D0 plus the undirected edges (bi, bj, bw) (device tensors as
    ``component_bridges`` returns them): D0 [N, N] fp64 holds the shortest paths of that graph, +inf between its components.
    Returns the repaired matrix (D0 itself, updated in place, on the update route), bit-symmetric with a zero diagonal.

    route="update": with P the p distinct endpoints of the edges, M = D0[P, P] with the edges min-ed in is closed by
    ``geodesic_distances``; then T = D0[:, P] (x) M and D = min(D0, T (x) D0[P, :]) by ``minplus`` (a shortest path that uses a new
    edge is a leg inside a component to its first endpoint, a path among endpoints, and a leg from its last endpoint), and
    ``symmetrize_min``, because the two triangles of the product associate their sums differently.  2 N^2 p + 2 N p^2 + 2 p^3
    operations.  route="full": the edges go into the neighbourhood graph of ``knn`` = (dist, idx) and ``geodesic_distances`` runs
    again, 2 N^3 operations.  route=None: "update" while p <= UPDATE_MAX_ENDPOINT_FRACTION * N or without ``knn``.  One host sync
    (the endpoints are sorted on the host)."""
    if route not in (None, "update", "full"):
        raise ValueError(f"repair_geodesics: route = {route!r}, expected 'update', 'full' or None")
    N = _square_f64(D0, "D0")
    _dev(bi, "bi", dtype=torch.int64); _dev(bj, "bj", dtype=torch.int64); _dev(bw, "bw", dtype=torch.float64)
    if bi.ndim != 1 or bi.shape != bj.shape or bi.shape != bw.shape:
        raise RuntimeError(f"repair_geodesics: bi, bj, bw must be [B], got {tuple(bi.shape)}, {tuple(bj.shape)}, {tuple(bw.shape)}")
    if bi.numel() == 0:
        return D0
    ends = torch.cat([bi, bj])
    if int(ends.min()) < 0 or int(ends.max()) >= N:
        raise RuntimeError(f"repair_geodesics: an edge endpoint outside 0..{N - 1}")
    P = torch.unique(ends)                                       # sorted
    p = P.numel()
    if route is None:
        route = "update" if knn is None or p <= UPDATE_MAX_ENDPOINT_FRACTION * N else "full"
    if route == "full":
        if knn is None:
            raise ValueError("repair_geodesics: route='full' needs knn=(dist, idx), the neighbours the graph is built from")
        return geodesic_distances(_min_edges(knn_graph(*knn), bi, bj, bw))
    pos = torch.searchsorted(P, ends)
    M = _min_edges(D0[P][:, P].contiguous(), pos[:bi.numel()], pos[bi.numel():], bw)
    geodesic_distances(M)
    cols, rows = D0[:, P].contiguous(), D0[P].contiguous()       # [N, p], [p, N]: copies, D0 is written below
    T = minplus(cols, M, cols.clone())
    return symmetrize_min(minplus(T, rows, D0))


def knn_cross(Xq, X, k, workspace=None):
    """Exact k nearest rows of X [N, D] for every row of Xq [M, D] (both CUDA fp32, contiguous): ``(dist, idx)`` with dist [M, k]
    fp64 (Euclidean, from fp64 sums of squared differences of the fp32 coordinates; ascending, equal distances by lower index)
    and idx [M, k] int64.  No row is excluded: a query that is a row of X finds it at distance 0.  k <= 64, k <= N.  No host sync."""
    _dev(Xq, "Xq"); _dev(X, "X")
    if Xq.ndim != 2 or X.ndim != 2 or Xq.shape[1] != X.shape[1]:
        raise RuntimeError(f"knn_cross: Xq and X must be [M, D] and [N, D], got {tuple(Xq.shape)} and {tuple(X.shape)}")
    if Xq.device != X.device:
        raise RuntimeError(f"knn_cross: Xq on {Xq.device}, X on {X.device}")
    (M, D), N, k = Xq.shape, X.shape[0], int(k)
    need = lib().idiff_knn_cross_workspace_bytes(M, N)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(1, need // 8), dtype=torch.float64, device=X.device)
    ok = M > 0 and k > 0
    dist = torch.empty((M, k) if ok else (1,), dtype=torch.float64, device=X.device)
    idx = torch.empty((M, k) if ok else (1,), dtype=torch.int64, device=X.device)
    _check(lib().idiff_knn_cross_f64(Xq.data_ptr(), M, X.data_ptr(), N, D, k, workspace.data_ptr(), workspace.numel() * 8,
                                     dist.data_ptr(), idx.data_ptr(), _stream()), "idiff_knn_cross_f64")
    return dist, idx


def isomap_project(dist, idx, D, A, colmean, grand):
    """Isomap coordinates Z [M, c] fp64 of M new points from their neighbours among the fitted points (dist [M, k] fp64, idx [M, k]
    int64, as ``knn_cross`` returns them), the fitted geodesic matrix D [N, N], A [N, c] = eigenvectors / sqrt(eigenvalue), and
    ``colmean`` [N], ``grand`` (0-d device tensor), the means of -1/2 D o D (``double_center(D, return_means=True)``): what
    scikit-learn's ``Isomap.transform`` computes, in one pass that never writes the [M, N] geodesic matrix.  An index outside
    0..N-1 is ignored.  k <= 64, c <= 64.  No host sync."""
    N = _square_f64(D, "D")
    for t, name in ((dist, "dist"), (A, "A"), (colmean, "colmean"), (grand, "grand")):
        _dev(t, name, dtype=torch.float64)
    _dev(idx, "idx", dtype=torch.int64)
    if dist.ndim != 2 or dist.shape != idx.shape:
        raise RuntimeError(f"isomap_project: dist and idx must both be [M, k], got {tuple(dist.shape)} and {tuple(idx.shape)}")
    if A.ndim != 2 or A.shape[0] != N or colmean.shape != (N,) or grand.numel() != 1:
        raise RuntimeError(f"isomap_project: A must be [{N}, c], colmean [{N}] and grand a scalar, got {tuple(A.shape)}, "
                           f"{tuple(colmean.shape)}, {tuple(grand.shape)}")
    (M, k), c = dist.shape, A.shape[1]
    Z = torch.empty(max(M, 1), max(c, 1), dtype=torch.float64, device=D.device)
    scratch = torch.empty(max(1, lib().idiff_isomap_project_scratch_doubles(c)), dtype=torch.float64, device=D.device)
    _check(lib().idiff_isomap_project_f64(dist.data_ptr(), idx.data_ptr(), M, k, D.data_ptr(), N, A.data_ptr(), c, colmean.data_ptr(),
                                          grand.data_ptr(), Z.data_ptr(), scratch.data_ptr(), _stream()), "idiff_isomap_project_f64")
    return Z


# ------------------------------------------------------------------------------------------- image manifolds
def _host_table(table, cols, name):
    """A host table of integers [K, cols] as contiguous int32 numpy (device tensors are refused: the table is checked here, on the host)."""
    import numpy as np
    if isinstance(table, torch.Tensor):
        if table.device.type != "cpu":
            raise RuntimeError(f"{name}: the table is checked on the host before upload; pass a host array, got a tensor on {table.device}")
        table = table.numpy()
    arr = np.asarray(table)
    if arr.ndim != 2 or arr.shape[1] != cols or arr.shape[0] < 1 or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"{name}: expected an integer table [K >= 1, {cols}], got {arr.dtype} {tuple(arr.shape)}")
    return np.ascontiguousarray(arr.astype(np.int64))


def _render(entry, values, table, S, out):
    N, K = values.shape
    S = int(S)
    if table.shape[0] != K:
        raise ValueError(f"{entry}: {table.shape[0]} table rows for {K} columns of per-image values")
    if out is None:
        if N * S * S >= 2 ** 31:
            raise RuntimeError(f"{entry}: N * S * S = {N * S * S} is not below 2^31; render in slabs")
        out = torch.empty(N, S, S, device=values.device, dtype=torch.float32)
    _dev(out, "out")
    if out.numel() != N * S * S or out.device != values.device:
        raise RuntimeError(f"{entry}: out holds {out.numel()} values on {out.device} for {N} images of {S} x {S} on {values.device}")
    tab = torch.from_numpy(table.astype("int32")).to(values.device)
    _check(getattr(lib(), entry)(values.data_ptr(), tab.data_ptr(), out.data_ptr(), N, K, S, _stream()), entry)
    return out


def render_squares(coef, rects, S, out=None):
    """out [N, S, S] fp32 with out[n, p] = sum_k coef[n, k] [p in square k], a sequential fp32 chain in ascending k (bit-equal to the
    reference's FixedSquaresManifold).  coef [N, K] CUDA fp32; rects [K, 3] HOST integers (row0, col0, side), checked against the
    image here, before upload: a square that leaves it is a ValueError and nothing is launched."""
    _dev(coef, "coef")
    if coef.ndim != 2:
        raise RuntimeError(f"render_squares: coef must be [N, K], got {tuple(coef.shape)}")
    r = _host_table(rects, 3, "render_squares")
    bad = (r[:, 2] < 1) | (r[:, 0] < 0) | (r[:, 1] < 0) | (r[:, 0] + r[:, 2] > int(S)) | (r[:, 1] + r[:, 2] > int(S))
    if bad.any():
        k = int(bad.nonzero()[0][0])
        raise ValueError(f"render_squares: square {k} (row0, col0, side) = {tuple(int(v) for v in r[k])} leaves the {S} x {S} image")
    return _render("idiff_render_squares_f32", coef, r, S, out)


def render_gaussians(std, centres, S, out=None):
    """out [N, S, S] fp32: sum_k of Gaussian blobs of standard deviation std[n, k] around centres[k], each image scaled to [0, 1]
    (the reference's FixedGaussiansManifold; fp64 accumulation, see idiff_render_gaussians_f32).  std [N, K] CUDA fp64; centres
    [K, 2] HOST integers (row, column), checked against the image here, before upload."""
    _dev(std, "std", dtype=torch.float64)
    if std.ndim != 2:
        raise RuntimeError(f"render_gaussians: std must be [N, K], got {tuple(std.shape)}")
    c = _host_table(centres, 2, "render_gaussians")
    bad = ((c < 0) | (c >= int(S))).any(axis=1)
    if bad.any():
        k = int(bad.nonzero()[0][0])
        raise ValueError(f"render_gaussians: centre {k} = {tuple(int(v) for v in c[k])} is outside the {S} x {S} image")
    return _render("idiff_render_gaussians_f32", std, c, S, out)


# ------------------------------------------------------------------------------------------- union of k-spheres
def ksphere_union_ok(n, J, P):
    """True where ksphere_union_score serves frames of P columns in all, J components, in R^n (idiff_ksphere_union_ok: host only)."""
    return bool(lib().idiff_ksphere_union_ok(int(n), int(J), int(P)))


def ksphere_union_score(x, qcat, comp, sigma, mult=None, out=None, refused=None):
    """out [B, n] = mult[b] (-x_b + sum_j w_j (R_j A_j / r_j) Q_j Q_j^T x_b): the exact score of the noised union of spheres times
    mult sigma^2, one launch (idiff_ksphere_union_score_f32).  x [B, n] fp32, qcat [n, P] fp64, sigma [B] and mult [B] (or None) fp32 on
    the device; comp: HOST rows (first column, columns, radius, log weight), one per component.  Returns (out, refused): refused is
    a device int32 [1] the launch ADDS its count of refused rows to (made and zeroed here when not given); those rows are NaN.
    A shape the kernel does not serve is a RuntimeError before any launch."""
    import numpy as np
    _dev(x, "x"); _dev(qcat, "qcat", dtype=torch.float64); _dev(sigma, "sigma")
    if x.ndim != 2 or qcat.ndim != 2 or qcat.shape[0] != x.shape[1] or sigma.numel() != x.shape[0]:
        raise RuntimeError(f"ksphere_union_score: x {tuple(x.shape)}, qcat {tuple(qcat.shape)}, sigma {tuple(sigma.shape)}")
    B, n = x.shape
    P = qcat.shape[1]
    tab = np.ascontiguousarray(np.asarray(comp, dtype=np.float64))
    if tab.ndim != 2 or tab.shape[1] != 4 or tab.shape[0] < 1:
        raise ValueError(f"ksphere_union_score: expected a host table [J, 4], got {tuple(tab.shape)}")
    J = tab.shape[0]
    if not ksphere_union_ok(n, J, P):
        raise RuntimeError(f"ksphere_union_score: n = {n}, J = {J}, P = {P} is not served (idiff_ksphere_union_ok): at most 8 components "
                           "of at most 128 columns each, and the frames must fit the LDS")
    if mult is not None:
        _dev(mult, "mult")
        if mult.numel() != B:
            raise RuntimeError(f"ksphere_union_score: mult holds {mult.numel()} values for {B} rows")
    if out is None:
        out = torch.empty_like(x)
    _dev(out, "out")
    if out.shape != x.shape:
        raise RuntimeError(f"ksphere_union_score: out {tuple(out.shape)} for x {tuple(x.shape)}")
    if refused is None:
        refused = torch.zeros(1, device=x.device, dtype=torch.int32)
    _dev(refused, "refused", dtype=torch.int32)
    _check(lib().idiff_ksphere_union_score_f32(x.data_ptr(), qcat.data_ptr(), tab.ctypes.data, sigma.data_ptr(), _ptr(mult), out.data_ptr(),
                                               refused.data_ptr(), B, n, J, P, _stream()), "idiff_ksphere_union_score_f32")
    return out, refused


# ------------------------------------------------------------------------------------------- empirical score of a point cloud
def empirical_score_ok(N, D):
    """True where empirical_score serves a cloud of N points in R^D (idiff_empirical_score_ok: host only; D <= 192)."""
    return bool(lib().idiff_empirical_score_ok(int(N), int(D)))


def empirical_pack(X):
    """The cloud X [N, D] (CUDA fp32) as the kernel reads it: ``{"Y", "h", "c", "N", "D"}`` with c [D] the fp64 column mean,
    Y [N, D4] = X - c in fp64, rows padded with zeros to D4 = 4 ceil(D / 4), and h [N] = |y_i|^2 / 2.  Plain torch fp64 ops on the
    device, once per cloud; no host sync."""
    _dev(X, "X")
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise RuntimeError(f"empirical_pack: X must be [N >= 1, D >= 1], got {tuple(X.shape)}")
    N, D = X.shape
    Xd = X.double()
    c = Xd.mean(dim=0).contiguous()
    Y = torch.zeros(N, (D + 3) // 4 * 4, dtype=torch.float64, device=X.device)
    Y[:, :D] = Xd - c
    h = (0.5 * (Y * Y).sum(dim=1)).contiguous()
    return {"Y": Y, "h": h, "c": c, "N": N, "D": D}


def empirical_score(x, pack, sigma, mult=None, out=None, ess=None):
    """out [B, D] = mult[b] (sum_i w_bi x_i - x_b), w_b = softmax_i(-|x_b - x_i|^2 / (2 sigma_b^2)) over the packed cloud: the score
    of the cloud's empirical distribution at noise level sigma_b times mult sigma^2, one launch (idiff_empirical_score_f32), fp64
    throughout, no [B, N] buffer.  x [B, D], sigma [B] and mult [B] (or None) fp32 on the device; ``pack`` from ``empirical_pack``.
    Returns (out, ess): ess [B] fp32 = 1 / sum_i w_bi^2 (made here when not given).  A row whose x or sigma is not finite, or whose
    sigma <= 0, is NaN in both.  A shape the kernel does not serve is a RuntimeError before any launch.  No host sync."""
    _dev(x, "x"); _dev(sigma, "sigma")
    Y, h, c = _dev(pack["Y"], "pack Y", dtype=torch.float64), _dev(pack["h"], "pack h", dtype=torch.float64), \
        _dev(pack["c"], "pack c", dtype=torch.float64)
    N, D = int(pack["N"]), int(pack["D"])
    if x.ndim != 2 or x.shape[1] != D or sigma.numel() != x.shape[0] or tuple(Y.shape) != (N, (D + 3) // 4 * 4) or h.numel() != N \
            or c.numel() != D:
        raise RuntimeError(f"empirical_score: x {tuple(x.shape)}, sigma {tuple(sigma.shape)}, a cloud of {N} points in R^{D} packed as "
                           f"Y {tuple(Y.shape)}, h {tuple(h.shape)}, c {tuple(c.shape)}")
    B = x.shape[0]
    if not empirical_score_ok(N, D):
        raise RuntimeError(f"empirical_score: N = {N}, D = {D} is not served (idiff_empirical_score_ok): the kernel keeps a row's fp64 "
                           "output in registers, D <= 192")
    if mult is not None:
        _dev(mult, "mult")
        if mult.numel() != B:
            raise RuntimeError(f"empirical_score: mult holds {mult.numel()} values for {B} rows")
    if out is None:
        out = torch.empty_like(x)
    _dev(out, "out")
    if out.shape != x.shape:
        raise RuntimeError(f"empirical_score: out {tuple(out.shape)} for x {tuple(x.shape)}")
    if ess is None:
        ess = torch.empty(B, device=x.device, dtype=torch.float32)
    _dev(ess, "ess")
    if ess.numel() != B:
        raise RuntimeError(f"empirical_score: ess holds {ess.numel()} values for {B} rows")
    if B == 0:
        return out, ess
    _check(lib().idiff_empirical_score_f32(x.data_ptr(), Y.data_ptr(), h.data_ptr(), c.data_ptr(), sigma.data_ptr(), _ptr(mult),
                                           out.data_ptr(), ess.data_ptr(), B, N, D, _stream()), "idiff_empirical_score_f32")
    return out, ess


# ------------------------------------------------------------------------------------------- Jacobian of the empirical score
JACOBIAN_D_MAX = 192          # idiff_empirical_jacobian_ok: the upper blocks of one query's C live in a workgroup's registers
EIGVALS_BATCH_MAX = 65535     # matrices idiff_tridiag_eigvals_f64 takes per call


def empirical_jacobian_ok(N, D):
    """True where empirical_jacobian serves a cloud of N points in R^D (idiff_empirical_jacobian_ok: host only; D <= 192)."""
    return bool(lib().idiff_empirical_jacobian_ok(int(N), int(D)))


def empirical_jacobian(x, X, sigma, C=None, mean=None, ess=None):
    """``(C [B, D, D] fp64, mean [B, D] fp64, ess [B] fp32)`` for the queries (x_b, sigma_b) against the RAW cloud X [N, D] (CUDA
    fp32, not the pack): with d_i = x_i - x_b and w_b = softmax_i(-|d_i|^2 / (2 sigma_b^2)), mean = sum_i w_i d_i (the score times
    sigma^2), C = sum_i w_i (d_i - mean)(d_i - mean)^T / sigma_b^2 = I + sigma_b^2 times the Jacobian of the score (symmetric to the
    bit) and ess = 1 / sum_i w_i^2.  One launch (idiff_empirical_jacobian_f64), fp64 throughout, no workspace.  x [B, D] and sigma [B]
    fp32 on the device; the outputs are made here when not given.  A query whose x or sigma is not finite, or whose sigma <= 0, is
    NaN in all three.  A shape the kernel does not serve is a RuntimeError before any launch.  No host sync."""
    _dev(x, "x"); _dev(X, "X"); _dev(sigma, "sigma")
    if X.ndim != 2 or x.ndim != 2 or x.shape[1] != X.shape[1] or sigma.numel() != x.shape[0]:
        raise RuntimeError(f"empirical_jacobian: x {tuple(x.shape)}, sigma {tuple(sigma.shape)}, X {tuple(X.shape)}")
    (B, D), N = x.shape, X.shape[0]
    if not empirical_jacobian_ok(N, D):
        raise RuntimeError(f"empirical_jacobian: N = {N}, D = {D} is not served (idiff_empirical_jacobian_ok): a workgroup keeps the "
                           f"upper triangle of a query's fp64 C in registers, 1 <= D <= {JACOBIAN_D_MAX}, 1 <= N")
    if C is None:
        C = torch.empty(B, D, D, device=x.device, dtype=torch.float64)
    if mean is None:
        mean = torch.empty(B, D, device=x.device, dtype=torch.float64)
    if ess is None:
        ess = torch.empty(B, device=x.device, dtype=torch.float32)
    _dev(C, "C", dtype=torch.float64); _dev(mean, "mean", dtype=torch.float64); _dev(ess, "ess")
    if tuple(C.shape) != (B, D, D) or tuple(mean.shape) != (B, D) or ess.numel() != B:
        raise RuntimeError(f"empirical_jacobian: C {tuple(C.shape)}, mean {tuple(mean.shape)}, ess {tuple(ess.shape)} for x {tuple(x.shape)}")
    if B == 0:
        return C, mean, ess
    _check(lib().idiff_empirical_jacobian_f64(x.data_ptr(), X.data_ptr(), sigma.data_ptr(), C.data_ptr(), mean.data_ptr(), ess.data_ptr(),
                                              B, N, D, _stream()), "idiff_empirical_jacobian_f64")
    return C, mean, ess


# ------------------------------------------------------------------------------------------- FLIPD of the empirical distribution
FLIPD_S_MAX = 32              # idiff_empirical_flipd_ok: bandwidths a call


def empirical_flipd_ok(N, D, S=1):
    """True where empirical_flipd serves a cloud of N points in R^D at S bandwidths (idiff_empirical_flipd_ok: host only; any
    D <= 65536, S <= 32)."""
    return bool(lib().idiff_empirical_flipd_ok(int(N), int(D), int(S)))


def empirical_flipd_splits(P, N, D):
    """The ranges the cloud is cut into for P queries when the caller names none (idiff_empirical_flipd_splits: host only)."""
    return int(lib().idiff_empirical_flipd_splits(int(P), int(N), int(D)))


def empirical_flipd(x, pack, sigmas, exclude=None, flipd=None, ess=None, splits=None, workspace=None):
    """``(flipd [P, S] fp64, ess [P, S] fp32)``: flipd[p, j] = sum_i w_i r_i^2 / sigma_j^2 with r_i^2 = |x_i - x_p|^2 and
    w = softmax_i(-r_i^2 / (2 sigma_j^2)) over the packed cloud, ess = 1 / sum_i w_i^2 -- FLIPD, D + sigma^2 (tr grad s + |s|^2), of the
    cloud's empirical distribution at every bandwidth from one pass over the distances (idiff_empirical_flipd_f64: two launches, fp64
    throughout, any D).  x [P, D] and sigmas [S <= 32] fp32 on the device; ``pack`` from ``empirical_pack``.  ``exclude`` [P]: for each
    query the cloud row left out of its softmax (-1: none), given ON THE HOST (a sequence, numpy array or CPU tensor of integers) so
    that a value outside [-1, N) is refused here without reading the device back.  ``splits``: the ranges N is cut into across
    workgroups (default ``empirical_flipd_splits``); equal splits give equal bits.  A query row that is not finite is NaN in its row, a
    sigma that is not positive and finite in its column, a query with no admissible point everywhere.  A shape the kernel does not
    serve is a RuntimeError before any launch.  No host sync."""
    _dev(x, "x"); _dev(sigmas, "sigmas")
    Y, h, c = _dev(pack["Y"], "pack Y", dtype=torch.float64), _dev(pack["h"], "pack h", dtype=torch.float64), \
        _dev(pack["c"], "pack c", dtype=torch.float64)
    N, D = int(pack["N"]), int(pack["D"])
    if x.ndim != 2 or x.shape[1] != D or sigmas.ndim != 1 or tuple(Y.shape) != (N, (D + 3) // 4 * 4) or h.numel() != N \
            or c.numel() != D:
        raise RuntimeError(f"empirical_flipd: x {tuple(x.shape)}, sigmas {tuple(sigmas.shape)}, a cloud of {N} points in R^{D} packed "
                           f"as Y {tuple(Y.shape)}, h {tuple(h.shape)}, c {tuple(c.shape)}")
    P, S = x.shape[0], sigmas.numel()
    if not empirical_flipd_ok(N, D, S):
        raise RuntimeError(f"empirical_flipd: N = {N}, D = {D}, S = {S} is not served (idiff_empirical_flipd_ok): 1 <= D <= 65536, "
                           f"1 <= S <= {FLIPD_S_MAX} bandwidths a call, 1 <= N")
    if exclude is not None:
        if isinstance(exclude, torch.Tensor) and exclude.is_cuda:
            raise RuntimeError("empirical_flipd: exclude is checked on the host: pass a sequence, numpy array or CPU tensor")
        ex = torch.as_tensor(exclude, dtype=torch.int64).reshape(-1)
        if ex.numel() != P:
            raise RuntimeError(f"empirical_flipd: exclude holds {ex.numel()} values for {P} queries")
        if P and (int(ex.min()) < -1 or int(ex.max()) >= N):
            raise RuntimeError(f"empirical_flipd: exclude out of range: values {int(ex.min())} .. {int(ex.max())} for a cloud of {N} "
                               "points (-1 excludes nothing)")
        exclude = ex.to(torch.int32).to(x.device, non_blocking=True)
    if splits is None:
        splits = empirical_flipd_splits(P, N, D)
    splits = int(splits)
    if not 1 <= splits <= 65535:
        raise RuntimeError(f"empirical_flipd: splits = {splits}, must be 1 .. 65535")
    if flipd is None:
        flipd = torch.empty(P, S, device=x.device, dtype=torch.float64)
    if ess is None:
        ess = torch.empty(P, S, device=x.device, dtype=torch.float32)
    _dev(flipd, "flipd", dtype=torch.float64); _dev(ess, "ess")
    if tuple(flipd.shape) != (P, S) or tuple(ess.shape) != (P, S):
        raise RuntimeError(f"empirical_flipd: flipd {tuple(flipd.shape)}, ess {tuple(ess.shape)} for {P} queries and {S} bandwidths")
    need = int(lib().idiff_empirical_flipd_workspace_doubles(P, S, splits))
    if workspace is None:
        workspace = torch.empty(max(need, 1), device=x.device, dtype=torch.float64)
    _dev(workspace, "workspace", dtype=torch.float64)
    if workspace.numel() < need:
        raise RuntimeError(f"empirical_flipd: workspace of {workspace.numel()} doubles, P = {P}, S = {S}, splits = {splits} need {need}")
    if P == 0:
        return flipd, ess
    _check(lib().idiff_empirical_flipd_f64(x.data_ptr(), Y.data_ptr(), h.data_ptr(), c.data_ptr(), sigmas.data_ptr(), _ptr(exclude),
                                           flipd.data_ptr(), ess.data_ptr(), workspace.data_ptr(), workspace.numel(), P, N, D, S, splits,
                                           _stream()), "idiff_empirical_flipd_f64")
    return flipd, ess


# ------------------------------------------------------------------------------------------- Stein divergence from sampled score rows
STEIN_P_MAX = 65535           # points idiff_stein_rows_f64 takes per call


def stein_rows_ok(M, D):
    """True where stein_rows serves M rows of width D a point (idiff_stein_rows_ok: host only; 1 <= M < 2^31, 1 <= D <= 2^30)."""
    return bool(lib().idiff_stein_rows_ok(int(M), int(D)))


def column_means(S):
    """fp64 column means [P, D] of the contiguous S [P, M, D] (idiff_colmean_f64: two-stage, fixed order; the means the spectrum
    centres with)."""
    _dev(S, "scores")
    if S.ndim != 3 or S.shape[0] > 65535 or S.shape[1] < 1 or S.shape[2] < 1:
        raise RuntimeError(f"column_means: scores must be [P <= 65535, M >= 1, D >= 1], got {tuple(S.shape)}")
    P, M, D = S.shape
    mean = torch.empty(P, D, dtype=torch.float64, device=S.device)
    if P:
        scratch = torch.empty(P * 32 * D, dtype=torch.float64, device=S.device)
        _check(lib().idiff_colmean_f64(S.data_ptr(), P, M, D, mean.data_ptr(), scratch.data_ptr(), _stream()), "idiff_colmean_f64")
    return mean


def _rows3(t, name, P, M, D):
    """(row pitch, point stride) in elements of the fp32 [P, M, D] (or [M, D]: one point) device tensor ``t`` whose rows are dense."""
    _dev(t, name, contiguous=False)
    if t.ndim == 2:
        t = t.unsqueeze(0)
    if tuple(t.shape) != (P, M, D) or (D > 1 and t.stride(2) != 1) or (M > 1 and t.stride(1) < D) or \
            (P > 1 and t.stride(0) < (M - 1) * t.stride(1) + D):
        raise RuntimeError(f"stein_rows: {name} must be [{P}, {M}, {D}] with dense rows that do not overlap, got shape {tuple(t.shape)} "
                           f"strides {tuple(t.stride())}")
    return (t.stride(1) if M > 1 else D), (t.stride(0) if P > 1 else M * D)


def stein_rows(S, mean, seeds=None, Z=None, row0=0, rows_out=None, sums_out=None):
    """``(rows [P, M, 2], sums [P, 5])`` fp64 of the score rows S [P, M, D] (or [M, D]: one point) fp32, rows dense and possibly
    pitched: per row a' = z . (s - mean) and q = |z|^2, per point the sums of a', a'^2, q, q^2, a' q (idiff_stein_rows_f64: one pass over S,
    fp64 throughout, fixed order, no atomics).  ``mean`` [P, D] fp64, the column means (``column_means``).  Noise: ``Z``, shaped as S,
    or (D % 4 == 0) ``seeds``, one integer a point: row i is row ``row0 + i`` of the in-kernel Philox stream ``perturb_randn`` drew
    from that seed -- the same bits, never materialised.  A point with a non-finite value in S, Z or its mean has NaN there and in
    its sums, and no other point has.  A shape the kernel does not serve is a RuntimeError before any launch.  No host sync beyond
    the copy of the seeds."""
    if S.ndim not in (2, 3):
        raise RuntimeError(f"stein_rows: scores must be [M, D] or [P, M, D], got {tuple(S.shape)}")
    P, M, D = (1,) + tuple(S.shape) if S.ndim == 2 else tuple(S.shape)
    if not stein_rows_ok(M, D) or P > STEIN_P_MAX:
        raise RuntimeError(f"stein_rows: P = {P}, M = {M}, D = {D} is not served (idiff_stein_rows_ok; at most {STEIN_P_MAX} points a call)")
    lds, stride_s = _rows3(S, "scores", P, M, D)
    _dev(mean, "mean", dtype=torch.float64)
    if mean.numel() != P * D:
        raise RuntimeError(f"stein_rows: mean holds {mean.numel()} values for {P} points of width {D}")
    ldz = stride_z = 0
    if Z is not None:
        ldz, stride_z = _rows3(Z, "Z", P, M, D)
    elif seeds is None:
        raise RuntimeError("stein_rows: pass Z or seeds")
    elif D % 4:
        raise RuntimeError(f"stein_rows: D = {D} is no multiple of 4: the in-kernel Philox stream draws 4-column groups, pass Z")
    else:
        seeds = [int(s) & 0xFFFFFFFFFFFFFFFF for s in ([seeds] if isinstance(seeds, int) else seeds)]
        if len(seeds) != P:
            raise RuntimeError(f"stein_rows: {len(seeds)} seeds for {P} points")
        # (uint64 bit patterns through int64: torch has no unsigned 64-bit arithmetic, the kernel reads the bits)
        seeds = torch.tensor([s - (1 << 64) if s >> 63 else s for s in seeds], dtype=torch.int64).to(S.device)
    if int(row0) < 0:
        raise RuntimeError(f"stein_rows: row0 = {row0}")
    if rows_out is None:
        rows_out = torch.empty(P, M, 2, device=S.device, dtype=torch.float64)
    if sums_out is None:
        sums_out = torch.empty(P, 5, device=S.device, dtype=torch.float64)
    _dev(rows_out, "rows_out", dtype=torch.float64); _dev(sums_out, "sums_out", dtype=torch.float64)
    if rows_out.numel() != P * M * 2 or sums_out.numel() != P * 5:
        raise RuntimeError(f"stein_rows: rows_out {tuple(rows_out.shape)}, sums_out {tuple(sums_out.shape)} for {P} points of {M} rows")
    if P == 0:
        return rows_out, sums_out
    _check(lib().idiff_stein_rows_f64(S.data_ptr(), lds, stride_s, mean.data_ptr(), _ptr(Z), ldz, stride_z,
                                      0 if Z is not None else seeds.data_ptr(), int(row0), rows_out.data_ptr(), sums_out.data_ptr(),
                                      P, M, D, _stream()), "idiff_stein_rows_f64")
    return rows_out, sums_out


def sym_eigvals_batched(G):
    """Eigenvalues [P, D] (ascending, fp64) of P symmetric fp64 matrices G [P, D, D]; G is overwritten.  ``sym_eigvals`` with the P
    argument of idiff_symtridiag_f64 / idiff_tridiag_eigvals_f64: for D <= 128 one workgroup per matrix in one launch, above that
    the C side takes the matrices in turn over one scratch.  At most 65535 matrices a call, so more go in chunks.  No host sync."""
    _dev(G, "G", dtype=torch.float64)
    if G.ndim != 3 or G.shape[1] != G.shape[2] or G.shape[1] < 1:
        raise RuntimeError(f"sym_eigvals_batched: G must be [P, D >= 1, D], got {tuple(G.shape)}")
    P, D = G.shape[0], G.shape[1]
    eig = torch.empty(P, D, dtype=torch.float64, device=G.device)
    if P == 0:
        return eig
    chunk = min(P, EIGVALS_BATCH_MAX)
    diag = torch.empty(chunk, D, dtype=torch.float64, device=G.device)
    offd = torch.empty(chunk, D, dtype=torch.float64, device=G.device)
    scratch = torch.empty(max(1, lib().idiff_symtridiag_scratch_doubles(D)), dtype=torch.float64, device=G.device)
    for lo in range(0, P, chunk):
        n = min(chunk, P - lo)
        _check(lib().idiff_symtridiag_f64(G[lo:lo + n].data_ptr(), n, D, diag.data_ptr(), offd.data_ptr(), scratch.data_ptr(), _stream()),
               "idiff_symtridiag_f64")
        _check(lib().idiff_tridiag_eigvals_f64(diag.data_ptr(), offd.data_ptr(), n, D, eig[lo:lo + n].data_ptr(), _stream()),
               "idiff_tridiag_eigvals_f64")
    return eig


# ------------------------------------------------------------------------------------------- training the fcn score network
REDUCE_WS_DOUBLES = 1024      # IDIFF_REDUCE_WS_DOUBLES: workspace of the two fixed-order reductions


def _ld(t, name):
    if t.ndim != 2 or t.stride(1) != 1:
        raise RuntimeError(f"{name}: expected a 2-D tensor with contiguous rows, got shape {tuple(t.shape)} strides {t.stride()}")
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), (t.shape[1] + 3) // 4 * 4)


def gemm_nn(a, bm, out=None, elu_out=None, M=None, N=None, K=None, lda=None, ldb=None, ldc=None, ldp=None):
    """out[M, N] = (a[M, K] @ bm[K, N]) * g(elu_out): the data gradient of a Linear layer through the ELU below it, with ``bm`` the
    weight [out, in] as it lies and ``elu_out`` [M, N] (optional) that ELU's OUTPUT, g(a) = 1 if a > 0 else a + 1.  2-D tensors with
    contiguous rows (a row stride is the leading dimension), or explicit geometry.  Exact fp32 on the matrix cores, bit-reproducible."""
    _dev(a, "a", contiguous=False); _dev(bm, "bm", contiguous=False)
    if M is None:
        (M, K), N = a.shape, bm.shape[1]
        if bm.shape[0] != K:
            raise RuntimeError(f"gemm_nn: inner dimensions differ: {tuple(a.shape)} x {tuple(bm.shape)}")
        lda, ldb = _ld(a, "a"), _ld(bm, "bm")
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    _dev(out, "out", contiguous=False)
    if ldc is None:
        ldc = _ld(out, "out")
    if elu_out is not None:
        _dev(elu_out, "elu_out", contiguous=False)
        if ldp is None:
            ldp = _ld(elu_out, "elu_out")
    _check(lib().idiff_gemm_nn_f32(a.data_ptr(), lda, bm.data_ptr(), ldb, out.data_ptr(), ldc, _ptr(elu_out), ldp or 0, M, N, K,
                                   _stream()), "idiff_gemm_nn_f32")
    return out


def gemm_tn(at, bm, out=None, colsum=None, M=None, N=None, K=None, lda=None, ldb=None, ldc=None):
    """out[M, N] = at[K, M].T @ bm[K, N] (the weight gradient: K is the batch) and, with ``colsum`` [M], colsum[m] = sum_k at[k, m] in
    the order k = 0, 1, ... (the bias gradient).  Geometry as gemm_nn.  Exact fp32 on the matrix cores, bit-reproducible."""
    _dev(at, "at", contiguous=False); _dev(bm, "bm", contiguous=False)
    if M is None:
        (K, M), N = at.shape, bm.shape[1]
        if bm.shape[0] != K:
            raise RuntimeError(f"gemm_tn: inner dimensions differ: {tuple(at.shape)}^T x {tuple(bm.shape)}")
        lda, ldb = _ld(at, "at"), _ld(bm, "bm")
    if out is None:
        out = torch.empty(M, N, device=at.device, dtype=torch.float32)
    _dev(out, "out", contiguous=False)
    if ldc is None:
        ldc = _ld(out, "out")
    if colsum is not None:
        _dev(colsum, "colsum")
        if colsum.numel() != M:
            raise RuntimeError(f"gemm_tn: colsum has {colsum.numel()} entries for M = {M}")
    _check(lib().idiff_gemm_tn_f32(at.data_ptr(), lda, bm.data_ptr(), ldb, out.data_ptr(), ldc, _ptr(colsum), M, N, K, _stream()),
           "idiff_gemm_tn_f32")
    return out


def reduce_workspace(device):
    return torch.empty(REDUCE_WS_DOUBLES, device=device, dtype=torch.float64)


def dsm_loss_grad(out, z, weight=None, reduce_mean=True, grad=None, loss=None, want_grad=True, workspace=None):
    """``(loss, G)``: the denoising score matching loss mean_b weight[b] reduce_d (z - out)^2 (reduce = mean, or half the sum) as a
    device float summed in fp64 in a fixed order, and G = dloss/dout (None with ``want_grad=False``: the evaluation loss).  A given ``grad`` may be wider than D columns (its row stride
    is the pitch; the columns beyond D are left alone)."""
    _dev(out, "out"); _dev(z, "z")
    if out.ndim != 2 or out.shape != z.shape:
        raise RuntimeError(f"dsm_loss_grad: out {tuple(out.shape)}, z {tuple(z.shape)}")
    B, D = out.shape
    if weight is not None:
        _dev(weight, "weight")
        if weight.numel() != B:
            raise RuntimeError(f"dsm_loss_grad: weight has {weight.numel()} entries for {B} rows")
    if want_grad and grad is None:
        grad = torch.empty_like(out)
    ldg = 0
    if grad is not None:
        _dev(grad, "grad", contiguous=False)
        if grad.ndim != 2 or grad.shape[0] != B or grad.shape[1] < D or grad.stride(1) != 1:
            raise RuntimeError(f"dsm_loss_grad: grad {tuple(grad.shape)} for out {tuple(out.shape)}")
        ldg = grad.stride(0) if B > 1 else max(grad.stride(0), D)
    if loss is None:
        loss = torch.empty((), device=out.device, dtype=torch.float32)
    if workspace is None:
        workspace = reduce_workspace(out.device)
    _dev(loss, "loss"); _dev(workspace, "workspace", dtype=torch.float64)
    _check(lib().idiff_dsm_loss_grad_f32(out.data_ptr(), z.data_ptr(), _ptr(weight), _ptr(grad), ldg, loss.data_ptr(), workspace.data_ptr(),
                                         B, D, int(bool(reduce_mean)), _stream()), "idiff_dsm_loss_grad_f32")
    return loss, grad


def grad_sumsq(x, out=None, workspace=None):
    """Device double: sum of squares of the flat fp32 tensor ``x`` in fp64, fixed order."""
    _dev(x, "x")
    if out is None:
        out = torch.empty((), device=x.device, dtype=torch.float64)
    if workspace is None:
        workspace = reduce_workspace(x.device)
    _dev(out, "out", dtype=torch.float64); _dev(workspace, "workspace", dtype=torch.float64)
    _check(lib().idiff_grad_sumsq_f32(x.data_ptr(), x.numel(), workspace.data_ptr(), out.data_ptr(), _stream()), "idiff_grad_sumsq_f32")
    return out


def adam_step(theta, grad, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, sumsq=None, max_norm=0.0):
    """One torch.optim.Adam step over the flat buffers, in place in theta, m, v; ``step`` >= 1 numbers this step.  With ``sumsq`` (the
    device double of grad_sumsq) the gradient is first scaled by min(1, max_norm / (sqrt(sumsq) + 1e-6)) as clip_grad_norm_ does."""
    for t, name in ((theta, "theta"), (grad, "grad"), (m, "m"), (v, "v")):
        _dev(t, name)
        if t.numel() != theta.numel():
            raise RuntimeError(f"adam_step: {name} has {t.numel()} entries, theta {theta.numel()}")
    if sumsq is not None:
        _dev(sumsq, "sumsq", dtype=torch.float64)
    _check(lib().idiff_adam_step_f32(theta.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), theta.numel(), _ptr(sumsq),
                                     float(max_norm), float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                     int(step), _stream()), "idiff_adam_step_f32")


def fcn_train_input(x, z, std, mean_coeff, label, h):
    """h[b] = [mean_coeff[b] x[b] + std[b] z[b], label[b], 0 ...]: the padded input rows [B, kpad] of the fcn for a training batch."""
    _dev(x, "x"); _dev(z, "z"); _dev(std, "std"); _dev(label, "label"); _dev(h, "h")
    if mean_coeff is not None:
        _dev(mean_coeff, "mean_coeff")
    B, D = x.shape
    if z.shape != x.shape or h.ndim != 2 or h.shape[0] != B or std.numel() != B or label.numel() != B or \
            (mean_coeff is not None and mean_coeff.numel() != B):
        raise RuntimeError(f"fcn_train_input: x {tuple(x.shape)}, z {tuple(z.shape)}, std {tuple(std.shape)}, h {tuple(h.shape)}")
    _check(lib().idiff_fcn_train_input_f32(x.data_ptr(), z.data_ptr(), std.data_ptr(), _ptr(mean_coeff), label.data_ptr(), h.data_ptr(),
                                           B, D, h.shape[1], _stream()), "idiff_fcn_train_input_f32")
    return h


# ------------------------------------------------------------------------------------------- Jacobian of the fcn score network
def jvp_layer_ok(R, N, K):
    """True where jvp_layer serves R tangent rows a point, N outputs and K inputs (idiff_jvp_layer_ok: host only)."""
    return bool(lib().idiff_jvp_layer_ok(int(R), int(N), int(K)))


def _points3(t, name):
    """(P, rows, cols, ld, point stride) of a [P, rows, cols] (or [rows, cols]: one point) fp32 tensor with contiguous rows."""
    _dev(t, name, contiguous=False)
    if t.ndim == 2:
        t = t.unsqueeze(0)
    if t.ndim != 3 or t.stride(2) != 1:
        raise RuntimeError(f"{name}: expected [P, rows, cols] with contiguous rows, got shape {tuple(t.shape)} strides {t.stride()}")
    P, rows, cols = t.shape
    ld = t.stride(1) if rows > 1 else max(t.stride(1), (cols + 3) // 4 * 4)
    return P, rows, cols, ld, (t.stride(0) if P > 1 else max(t.stride(0), rows * ld))


def jvp_seed(w1, act, D=None, out=None, P=None, N=None, ldw=None, ld_act=None, ldt=None, stride_t=None):
    """out[p][i, n] = w1[n, i] * g(act[p, n]) for i < D: the tangent rows of the D input directions behind the first Linear + ELU, with
    ``w1`` [N, > D] that Linear's weight as it lies (its columns from D on, the time column and the pads, are never read), ``act`` [P, N]
    the ELU OUTPUT of the P points and g(a) = 1 if a > 0 else a + 1.  Tensors with contiguous rows (``out`` [P, D, N]; a row stride is the
    leading dimension), or explicit geometry.  One fp32 multiply per element: bit-equal to fl(w1 * fl(a + 1))."""
    _dev(w1, "w1", contiguous=False); _dev(act, "act", contiguous=False)
    if P is None:
        if D is None or act.ndim != 2 or w1.ndim != 2 or w1.shape[0] != act.shape[1] or w1.shape[1] < D:
            raise RuntimeError(f"jvp_seed: w1 {tuple(w1.shape)}, act {tuple(act.shape)}, D = {D}")
        (P, N), ldw, ld_act = act.shape, _ld(w1, "w1"), _ld(act, "act")
    if out is None:
        out = torch.empty(P, D, N, device=act.device, dtype=torch.float32)
    _dev(out, "out", contiguous=False)
    if ldt is None:
        Po, Do, No, ldt, stride_t = _points3(out, "out")
        if (Po, Do, No) != (P, D, N):
            raise RuntimeError(f"jvp_seed: out {tuple(out.shape)} for P = {P}, D = {D}, N = {N}")
    _check(lib().idiff_jvp_seed_f32(w1.data_ptr(), ldw, act.data_ptr(), ld_act, out.data_ptr(), ldt, stride_t, P, D, N, _stream()),
           "idiff_jvp_seed_f32")
    return out


def jvp_layer(a, w, act=None, out=None, P=None, R=None, N=None, K=None, lda=None, stride_a=None, ldw=None, ld_act=None, ldc=None,
              stride_c=None):
    """out[p] = (a[p] @ w.T) * g(act[p]) with g broadcast over the rows of point p: one layer of the forward-mode Jacobian.  ``a``
    [P, R, K] the tangent rows, ``w`` [N, K] an nn.Linear weight as it lies, ``act`` [P, N] the layer's ELU OUTPUT (None: no factor, the
    output layer), g(a) = 1 if a > 0 else a + 1.  Tensors with contiguous rows (row and point strides are taken from them), or explicit
    geometry.  Exact fp32 on the matrix cores, bit-reproducible; a point's bits do not depend on the other points."""
    _dev(a, "a", contiguous=False); _dev(w, "w", contiguous=False)
    if P is None:
        P, R, K, lda, stride_a = _points3(a, "a")
        if w.ndim != 2 or w.shape[1] != K:
            raise RuntimeError(f"jvp_layer: inner dimensions differ: {tuple(a.shape)} x {tuple(w.shape)}^T")
        N, ldw = w.shape[0], _ld(w, "w")
    if act is not None:
        _dev(act, "act", contiguous=False)
        if ld_act is None:
            if act.ndim != 2 or tuple(act.shape) != (P, N):
                raise RuntimeError(f"jvp_layer: act {tuple(act.shape)} for P = {P}, N = {N}")
            ld_act = _ld(act, "act")
    if out is None:
        out = torch.empty(P, R, N, device=a.device, dtype=torch.float32)
    _dev(out, "out", contiguous=False)
    if ldc is None:
        Po, Ro, No, ldc, stride_c = _points3(out, "out")
        if (Po, Ro, No) != (P, R, N):
            raise RuntimeError(f"jvp_layer: out {tuple(out.shape)} for P = {P}, R = {R}, N = {N}")
    _check(lib().idiff_jvp_layer_f32(a.data_ptr(), lda, stride_a, w.data_ptr(), ldw, _ptr(act), ld_act or 0, out.data_ptr(), ldc, stride_c,
                                     P, R, N, K, _stream()), "idiff_jvp_layer_f32")
    return out


def _pitch(t, name, B, D):
    """Row pitch of a [B, >= D] fp32 tensor with contiguous rows (a view of wider rows keeps their pitch)."""
    _dev(t, name, contiguous=False)
    if t.ndim != 2 or t.shape[0] != B or t.shape[1] < D or t.stride(1) != 1:
        raise RuntimeError(f"{name}: expected [{B}, >= {D}] with contiguous rows, got shape {tuple(t.shape)} strides {t.stride()}")
    return t.stride(0) if B > 1 else max(t.stride(0), t.shape[1])


def sampler_step(x, s, a, b, c, z=None, out=None, mean_out=None, D=None, seed=0, row0=0, noise_norm=None, lang_scale=0.0,
                 score_scale=1.0, label_col=-1, label_value=0.0):
    """``(out, mean_out)``: mean_out = a x + b score_scale s and out = mean_out + c z over the first ``D`` columns (default: all of x) of
    2-D tensors with contiguous rows, in fp64 from the fp32 inputs, each output rounded once.  ``z`` None: the noise is drawn in the
    kernel from the stream (seed, row0); ``out`` None: in place in x.  ``noise_norm`` (device double of sampler_noise_norm) selects the
    Langevin form a = 1, b = lang_scale nn^2 score_scale, c = sqrt(2 lang_scale nn^2).  ``label_col`` >= D: ``label_value`` is written
    into that column of every row of out."""
    if x.ndim != 2:
        raise RuntimeError(f"sampler_step: x must be [B, D], got {tuple(x.shape)}")
    B = x.shape[0]
    D = x.shape[1] if D is None else int(D)
    if out is None:
        out = x
    ldx, lds, ldo = _pitch(x, "x", B, D), _pitch(s, "s", B, D), _pitch(out, "out", B, D)
    ldz = _pitch(z, "z", B, D) if z is not None else 0
    ldm = _pitch(mean_out, "mean_out", B, D) if mean_out is not None else 0
    if noise_norm is not None:
        _dev(noise_norm, "noise_norm", dtype=torch.float64)
    _check(lib().idiff_sampler_step_f32(x.data_ptr(), ldx, s.data_ptr(), lds, _ptr(z), ldz, out.data_ptr(), ldo, _ptr(mean_out), ldm, B, D,
                                        float(a), float(b), float(c), _ptr(noise_norm), float(lang_scale), float(score_scale),
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, int(row0), int(label_col), float(label_value), _stream()),
           "idiff_sampler_step_f32")
    return out, mean_out


def sampler_noise_norm(z=None, B=None, D=None, seed=0, row0=0, out=None, workspace=None, device=None):
    """Device double: mean_r |z_r| of the explicit noise ``z`` [B, >= D], or (z None) of the stream (seed, row0) that sampler_step draws
    for B rows of D columns; fp64, fixed order."""
    if z is not None:
        B = z.shape[0] if B is None else int(B)
        D = z.shape[1] if D is None else int(D)
        ldz, device = _pitch(z, "z", B, D), z.device
    else:
        if B is None or D is None or device is None:
            raise RuntimeError("sampler_noise_norm: without z pass B, D and device")
        ldz = 0
    if out is None:
        out = torch.empty((), device=device, dtype=torch.float64)
    if workspace is None:
        workspace = reduce_workspace(device)
    _dev(out, "out", dtype=torch.float64); _dev(workspace, "workspace", dtype=torch.float64)
    _check(lib().idiff_sampler_noise_norm_f32(_ptr(z), ldz, int(B), int(D), int(seed) & 0xFFFFFFFFFFFFFFFF, int(row0), workspace.data_ptr(),
                                              out.data_ptr(), _stream()), "idiff_sampler_noise_norm_f32")
    return out


# ------------------------------------------------------------------------------------------- probability-flow ODE (csrc/ode.hip)
def _pitch64(t, name, B, W):
    """Row pitch of a [B, >= W] fp64 tensor with contiguous rows."""
    _dev(t, name, dtype=torch.float64, contiguous=False)
    if t.ndim != 2 or t.shape[0] != B or t.shape[1] < W or t.stride(1) != 1:
        raise RuntimeError(f"{name}: expected [{B}, >= {W}] with contiguous rows, got shape {tuple(t.shape)} strides {t.stride()}")
    return t.stride(0) if B > 1 else max(t.stride(0), t.shape[1])


def _stages(K, B, W):
    """(row pitch, stage stride) of the stage derivatives K [7, B, >= W] fp64."""
    _dev(K, "K", dtype=torch.float64, contiguous=False)
    if K.ndim != 3 or K.shape[0] != 7 or K.shape[1] != B or K.shape[2] < W or K.stride(2) != 1:
        raise RuntimeError(f"K: expected [7, {B}, >= {W}] with contiguous rows, got shape {tuple(K.shape)} strides {K.stride()}")
    ldk = K.stride(1) if B > 1 else max(K.stride(1), K.shape[2])
    return ldk, max(K.stride(0), B * ldk)


def rk_stage(y, K, coef, x32, D, label_value, y_out=None):
    """v = y + sum_j coef[j] K[j] over the first W = y.shape[1] columns (``coef``: up to six host floats); ``y_out`` (optional, may be
    y) receives v, ``x32`` [B, > D] fp32 receives fl32(v[:, :D]) and ``label_value`` in column D (its later columns are not written)."""
    B, W = y.shape
    aug = W - int(D)
    coef = [float(c) for c in coef]
    ldk, strideK = _stages(K, B, W)
    ldy = _pitch64(y, "y", B, W)
    ldyo = _pitch64(y_out, "y_out", B, W) if y_out is not None else 0
    ldx = _pitch(x32, "x32", B, D + 1)
    if len(coef) > 6:
        raise RuntimeError(f"rk_stage: {len(coef)} coefficients (at most 6)")
    if B == 0:                                    # an empty tensor has no address to hand over
        return y_out
    arr = (c_d * 6)(*(coef + [0.0] * (6 - len(coef))))
    _check(lib().idiff_rk_stage_f64(y.data_ptr(), ldy, K.data_ptr(), ldk, strideK, arr, len(coef), _ptr(y_out), ldyo, x32.data_ptr(), ldx,
                                    B, int(D), aug, float(label_value), _stream()), "idiff_rk_stage_f64")
    return y_out


def rk_error(K, coef, y, y_new, atol, rtol, out=None, workspace=None):
    """Device double: sum over all elements of ((sum_j coef[j] K[j]) / (atol + rtol max(|y|, |y_new|)))^2, ``coef`` seven host floats;
    fp64, fixed order."""
    B, W = y.shape
    coef = [float(c) for c in coef]
    if len(coef) != 7:
        raise RuntimeError(f"rk_error: {len(coef)} coefficients (needs 7)")
    ldk, strideK = _stages(K, B, W)
    ldy, ldyn = _pitch64(y, "y", B, W), _pitch64(y_new, "y_new", B, W)
    if out is None:
        out = torch.zeros((), device=y.device, dtype=torch.float64)
    if workspace is None:
        workspace = reduce_workspace(y.device)
    _dev(out, "out", dtype=torch.float64); _dev(workspace, "workspace", dtype=torch.float64)
    if B == 0:
        return out
    _check(lib().idiff_rk_error_f64(K.data_ptr(), ldk, strideK, (c_d * 7)(*coef), y.data_ptr(), ldy, y_new.data_ptr(), ldyn, B, W,
                                    float(atol), float(rtol), workspace.data_ptr(), out.data_ptr(), _stream()), "idiff_rk_error_f64")
    return out


def flow_rhs(x32, v, a, b, Ks, D, aug, eps=None, u=None, q=None):
    """Ks[:, :D] = a x32 + b v; with ``aug`` Ks[:, D] = a D + b q, q the device doubles ``q`` [B] or the row sums of eps * u."""
    B = Ks.shape[0]
    D, aug = int(D), int(aug)
    ldk = _pitch64(Ks, "Ks", B, D + aug)
    ldx, ldv = _pitch(x32, "x32", B, D), _pitch(v, "v", B, D)
    lde = _pitch(eps, "eps", B, D) if eps is not None else 0
    ldu = _pitch(u, "u", B, D) if u is not None else 0
    if q is not None:
        _dev(q, "q", dtype=torch.float64)
        if q.numel() != B:
            raise RuntimeError(f"flow_rhs: q has {q.numel()} entries for {B} rows")
    if B == 0:
        return Ks
    _check(lib().idiff_flow_rhs_f64(x32.data_ptr(), ldx, v.data_ptr(), ldv, float(a), float(b), Ks.data_ptr(), ldk, B, D, aug, _ptr(eps), lde,
                                    _ptr(u), ldu, _ptr(q), _stream()), "idiff_flow_rhs_f64")
    return Ks


def jvp_trace(T, w_out, out=None, P=None, D=None, N=None, ldt=None, stride_t=None, ldw=None):
    """out[p] = sum_{i, n} T[p][i, n] w_out[i, n] (device doubles [P]): the trace of the network Jacobian from the tangent rows ``T``
    [P, D, N] in front of the output layer ``w_out`` [D, >= N]; tensors with contiguous rows, or explicit geometry."""
    _dev(T, "T", contiguous=False); _dev(w_out, "w_out", contiguous=False)
    if P is None:
        P, D, N, ldt, stride_t = _points3(T, "T")
        if w_out.ndim != 2 or w_out.shape[0] != D or w_out.shape[1] < N:
            raise RuntimeError(f"jvp_trace: w_out {tuple(w_out.shape)} for T {tuple(T.shape)}")
        ldw = _ld(w_out, "w_out")
    if out is None:
        out = torch.empty(P, device=T.device, dtype=torch.float64)
    _dev(out, "out", dtype=torch.float64)
    if out.numel() != P:
        raise RuntimeError(f"jvp_trace: out has {out.numel()} entries for P = {P}")
    if P == 0:
        return out
    _check(lib().idiff_jvp_trace_f64(T.data_ptr(), ldt, stride_t, w_out.data_ptr(), ldw, out.data_ptr(), P, D, N, _stream()),
           "idiff_jvp_trace_f64")
    return out
