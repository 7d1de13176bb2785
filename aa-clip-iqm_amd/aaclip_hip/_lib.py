"""ctypes binding of libaaclip_hip.so (C ABI: include/aaclip.h).

The product path has no fallback: if the shared library is missing or a call
fails, a RuntimeError is raised.  Build it with `__graft_entry__.build()` or
`make -C aa-clip-iqm_amd/csrc`.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AACLIP_LIB") or os.path.join(_HERE, "libaaclip_hip.so")   # AACLIP_LIB: experiment builds
ABI_VERSION = 10   # include/aaclip.h AACLIP_ABI_VERSION this binding was written against

F32, F16, BF16, F16X2 = 0, 1, 2, 3   # F16X2: split fp16 (hi + lo pairs), include/aaclip.h
EXACT16_QKV, EXACT16_OUT, EXACT16_FC, EXACT16_PROJ, EXACT16_ADAPTER = 1, 2, 4, 8, 16
ACT_NONE, ACT_LEAKY, ACT_RELU = 0, 1, 2
ACT_GELU = 3   # aaclip_act_backward only
EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_ACT_F32 = 0, 1, 2, 3
SUPPORT_FP32, SUPPORT_FP16 = 0, 1   # include/aaclip.h AACLIP_SUPPORT_*
SEG_LOSS_FOCAL, SEG_LOSS_DICE0, SEG_LOSS_DICE1, SEG_LOSS_ALL = 1, 2, 4, 7

_vp, _i, _l, _f, _sz, _d = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_size_t, C.c_double


class BlockWeights(C.Structure):
    """struct aaclip_block_weights (include/aaclip.h).  struct_bytes is filled in on construction; the library
    refuses a struct whose size field does not match its own sizeof."""
    _fields_ = [("struct_bytes", _sz)] + [(n, _vp) for n in (
        "ln1_w", "ln1_b", "qkv_w", "qkv_b", "out_w", "out_b", "ln2_w", "ln2_b",
        "fc_w", "fc_b", "proj_w", "proj_b", "adapter_w", "fc_w_fold", "fc_fold_s", "fc_fold_b",
        "qkv_w_fold", "qkv_fold_s", "qkv_fold_b")] + [("exact16", C.c_uint)]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_bytes = C.sizeof(BlockWeights)


class GemmFusedArgs(C.Structure):
    """struct aaclip_gemm_fused_args (include/aaclip.h): the fields of a product that only the block path sets.
    struct_bytes is filled in on construction; the library refuses any other size."""
    _fields_ = [("struct_bytes", _sz), ("resid", _vp), ("out16", _vp), ("stats_out", _vp), ("row_ab", _vp),
                ("col_s", _vp), ("w_exact16", _i), ("out_qk8", _i), ("out_no_hi8", _i)]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_bytes = C.sizeof(GemmFusedArgs)


OPTIM_MAX_GROUPS = 8     # include/aaclip.h AACLIP_OPTIM_MAX_GROUPS
OPTIM_CHUNK, OPTIM_TABLE_TENSORS, OPTIM_TABLE_BLOCKS = 16384, 24, 640   # csrc/optim_pack.h


class OptimTensor(C.Structure):
    """struct aaclip_optim_tensor (include/aaclip.h)"""
    _fields_ = [("p", _vp), ("g", _vp), ("m", _vp), ("v", _vp), ("n", _l), ("group", _i)]


class OptimTensors(C.Structure):
    """struct aaclip_optim_tensors (include/aaclip.h): a host array of OptimTensor.  struct_bytes is filled in on
    construction; the library refuses any other size."""
    _fields_ = [("struct_bytes", _sz), ("items", C.POINTER(OptimTensor)), ("count", _l)]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_bytes = C.sizeof(OptimTensors)


class OptimGroup(C.Structure):
    """struct aaclip_optim_group (include/aaclip.h)"""
    _fields_ = [("lr", _d), ("beta1", _d), ("beta2", _d), ("eps", _d), ("weight_decay", _d), ("decoupled", _i),
                ("step", _l)]


class TilePlan(C.Structure):
    """struct aaclip_tile_plan (include/aaclip.h): the geometry of a tiled frame and the stream of the call.
    struct_bytes is filled in on construction; the library refuses any other size."""
    _fields_ = [("struct_bytes", _sz), ("images", _i), ("channels", _i), ("tile", _i), ("grid", _i), ("overlap", _i),
                ("stream", _vp)]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_bytes = C.sizeof(TilePlan)


class OverlayPlan(C.Structure):
    """struct aaclip_overlay_plan (include/aaclip.h): the sizes, panels, colours and normalisation of an overlay call and
    its stream.  struct_bytes is filled in on construction; the library refuses any other size."""
    _fields_ = [("struct_bytes", _sz), ("images", _i), ("height", _i), ("width", _i), ("panels", C.c_uint), ("alpha256", _i),
                ("thickness", _i), ("pred_colour", C.c_uint8 * 3), ("truth_colour", C.c_uint8 * 3), ("mean", _f * 3),
                ("std", _f * 3), ("stream", _vp)]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_bytes = C.sizeof(OverlayPlan)


OVERLAY_FRAME, OVERLAY_HEAT, OVERLAY_TRUTH = 1, 2, 4


class PngPlan(C.Structure):
    """struct aaclip_png_plan (include/aaclip.h): the sizes of a PNG encoding call and its stream.  struct_bytes is
    filled in on construction; the library refuses any other size."""
    _fields_ = [("struct_bytes", _sz), ("images", _i), ("height", _i), ("width", _i), ("channels", _i), ("stream", _vp)]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_bytes = C.sizeof(PngPlan)


class BootstrapPlan(C.Structure):
    """struct aaclip_bootstrap_plan (include/aaclip.h): the sizes of a bootstrap call and its stream.  struct_bytes is
    filled in on construction; the library refuses any other size."""
    _fields_ = [("struct_bytes", _sz), ("n", _l), ("images", _l), ("replicates", _l), ("stream", _vp)]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_bytes = C.sizeof(BootstrapPlan)


# name -> (restype, argtypes); every symbol include/aaclip.h declares
SIGNATURES = {
    "aaclip_version": (_i, []),
    "aaclip_last_error": (C.c_char_p, []),
    "aaclip_workspace_bytes": (_sz, [_i, _l, _i, _i, _i]),
    "aaclip_patch_embed": (_i, [_vp] * 7 + [_i] * 6 + [_vp, _sz, _vp]),
    "aaclip_block": (_i, [_vp, C.POINTER(BlockWeights), _f] + [_i] * 7 + [_vp, _sz, _vp]),
    "aaclip_blocks": (_i, [_vp, C.POINTER(BlockWeights), _i, _f] + [_i] * 7 + [_vp, _sz, _vp]),
    "aaclip_blocks_to": (_i, [_vp, _vp, C.POINTER(BlockWeights), _i, _f] + [_i] * 7 + [_vp, _sz, _vp]),
    "aaclip_blocks_taps": (_i, [_vp, C.POINTER(_vp), C.POINTER(BlockWeights), _i, _f] + [_i] * 7 + [_vp, _sz, _vp]),
    "aaclip_tap_head": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp] + [_i] * 5 + [_vp, _sz, _vp]),
    "aaclip_tap_head_keep_rows": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp] + [_i] * 5 + [_vp, _sz, _vp]),
    "aaclip_det_head": (_i, [_vp, _vp, _vp, _vp, _i, _vp] + [_i] * 5 + [_vp, _sz, _vp]),
    "aaclip_anomaly_map": (_i, [C.POINTER(_vp), _i, _vp, _l, _vp, _i, _i, _i, _i, _i, _f, _vp, _sz, _vp]),
    "aaclip_similarity_map_train": (_i, [_vp, _vp, _l, _vp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "aaclip_similarity_map_train_backward_workspace_bytes": (_sz, [_i, _i, _i]),
    "aaclip_similarity_map_train_backward": (_i, [_vp, _vp, _l, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "aaclip_iqm_map_train": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "aaclip_iqm_map_train_backward_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "aaclip_iqm_map_train_backward": (_i, [_vp] * 6 + [_i] * 4 + [_vp, _sz, _vp]),
    "aaclip_seg_loss_workspace_bytes": (_sz, [_i]),
    "aaclip_seg_loss": (_i, [_vp, _l, _l, _vp, _i, _vp, _vp, _i, _l, _vp, _sz, _vp]),
    "aaclip_seg_loss_backward": (_i, [_vp, _l, _l, _vp, _i, _vp, _vp, _vp, _i, _l, _vp]),
    "aaclip_text_backward_workspace_bytes": (_sz, [_l, _i, _i]),
    "aaclip_gemm_wgrad": (_i, [_vp, _l, _vp, _l, _vp, _l, _i, _i, _vp, _sz, _vp]),
    "aaclip_attention_backward": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "aaclip_attention_backward_long_workspace_bytes": (_sz, [_i, _i, _i]),
    "aaclip_attention_backward_long": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _sz, _vp]),
    "aaclip_layernorm_backward": (_i, [_vp, _vp, _vp, _vp, _vp, _l, _i, _f, _vp]),
    "aaclip_adapter_mix_backward": (_i, [_vp, _vp, _vp, _vp, _vp, _l, _i, _f, _vp]),
    "aaclip_block_backward": (_i, [_vp, C.POINTER(BlockWeights), C.POINTER(BlockWeights), _f] + [_i] * 6
                              + [_vp, _vp, _vp, _vp, _sz, _vp]),
    "aaclip_block_backward_long_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "aaclip_block_backward_long": (_i, [_vp, C.POINTER(BlockWeights), C.POINTER(BlockWeights), _f] + [_i] * 6
                                   + [_vp, _vp, _vp, _vp, _sz, _vp]),
    "aaclip_split3_rows": (_i, [_vp, _vp, _l, _i, _vp]),
    "aaclip_attention_backward_long_bf16x3_workspace_bytes": (_sz, [_i, _i, _i]),
    "aaclip_attention_backward_long_bf16x3": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _sz, _vp]),
    "aaclip_block_backward_long_bf16x3_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "aaclip_block_backward_long_bf16x3": (_i, [_vp] + [C.POINTER(BlockWeights)] * 3 + [_f] + [_i] * 6
                                          + [_vp, _vp, _vp, _vp, _sz, _vp]),
    "aaclip_row_head_backward": (_i, [_vp] * 6 + [_i, _vp, _vp, _vp] + [_i] * 5 + [_vp, _sz, _vp]),
    "aaclip_tap_head_backward_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "aaclip_tap_head_backward": (_i, [_vp] * 5 + [_i] + [_vp] * 7 + [_i] * 4 + [_vp, _sz, _vp]),
    "aaclip_text_embed": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "aaclip_resample_ksize": (_i, [_i, _i]),
    "aaclip_resample_table": (_i, [_i, _i, _vp, _vp]),
    "aaclip_preprocess": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "aaclip_color_jitter_workspace_bytes": (_sz, [_i, _i, _i]),
    "aaclip_color_jitter": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "aaclip_nearest_table": (_i, [_i, _i, _vp]),
    "aaclip_mask_preprocess": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "aaclip_augment_geometric": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "aaclip_metrics_range_workspace_bytes": (_sz, [_l, _l]),
    "aaclip_metrics_range": (_i, [_vp, _vp, _l, _l, _vp, _vp, _vp, _sz, _vp]),
    "aaclip_metrics_normalise": (_i, [_vp, _vp, _l, _vp, _vp]),
    "aaclip_metrics_sort_workspace_bytes": (_sz, [_l]),
    "aaclip_metrics_sort_group_items": (_l, []),
    "aaclip_metrics_sort": (_i, [_vp, _vp, _l, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "aaclip_metrics_curve_workspace_bytes": (_sz, [_l]),
    "aaclip_metrics_curve": (_i, [_vp, _vp, _l, _i, _vp, _vp, _sz, _vp]),
    "aaclip_metrics_f1max_workspace_bytes": (_sz, [_l]),
    "aaclip_metrics_f1max": (_i, [_vp, _vp, _l, _i, _vp, _vp, _sz, _vp]),
    "aaclip_metrics_threshold_workspace_bytes": (_sz, [_l, _l]),
    "aaclip_metrics_threshold": (_i, [_vp, _vp, _l, _l, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "aaclip_metrics_regions_workspace_bytes": (_sz, [_l, _l, _l]),
    "aaclip_metrics_regions": (_i, [_vp, _l, _l, _l, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "aaclip_region_table_workspace_bytes": (_sz, [_l, _l, _l]),
    "aaclip_region_table": (_i, [_vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _l, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "aaclip_metrics_sort_pairs_workspace_bytes": (_sz, [_l]),
    "aaclip_metrics_sort_pairs": (_i, [_vp, _vp, _l, _vp, _vp, _vp, _sz, _vp]),
    "aaclip_metrics_pro_curve_workspace_bytes": (_sz, [_l]),
    "aaclip_metrics_pro_curve": (_i, [_vp, _vp, _l, _vp, _d, _vp, _vp, _sz, _vp]),
    "aaclip_optim_grad_norm_workspace_bytes": (_sz, [C.POINTER(OptimTensors)]),
    "aaclip_optim_grad_norm": (_i, [C.POINTER(OptimTensors), _f, _vp, _vp, _sz, _vp]),
    "aaclip_optim_adam_step": (_i, [C.POINTER(OptimTensors), C.POINTER(OptimGroup), _i, _vp, _vp]),
    "aaclip_support_nearest_workspace_bytes": (_sz, [_l, _l, _i, _i]),
    "aaclip_support_nearest": (_i, [_vp, _l, _vp, _l, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "aaclip_support_bank_rows": (_i, [_vp, _l, _i, _i, _vp, _vp]),
    "aaclip_support_map": (_i, [C.POINTER(_vp), _i, _vp, _f, _vp, _i, _i, _i, _i, _f, _vp, _sz, _vp]),
    "aaclip_coreset_rows": (_i, [_vp, _l, _i, _vp, _vp, _vp]),
    "aaclip_coreset_unit_rows": (_i, [_vp, _l, _i, _vp, _vp]),
    "aaclip_coreset_select_workspace_bytes": (_sz, [_l, _i, _l]),
    "aaclip_coreset_select": (_i, [_vp, _vp, _l, _i, _l, _l, _vp, _vp, _vp, _vp, _sz, _vp]),
    "aaclip_tile_canvas": (_i, [_i, _i, _i]),
    "aaclip_tile_gather": (_i, [C.POINTER(TilePlan), _vp, _vp]),
    "aaclip_tile_stitch": (_i, [C.POINTER(TilePlan), _vp, _vp]),
    "aaclip_overlay_render": (_i, [C.POINTER(OverlayPlan)] + [_vp] * 7),
    "aaclip_png_workspace_bytes": (_sz, [C.POINTER(PngPlan)]),
    "aaclip_png_capacity_bytes": (_sz, [C.POINTER(PngPlan)]),
    "aaclip_png_encode": (_i, [C.POINTER(PngPlan), _vp, _vp, _sz, _vp, _sz, _vp]),
    "aaclip_bootstrap_max_images": (_l, []),
    "aaclip_bootstrap_workspace_bytes": (_sz, [_l, _l, _l]),
    "aaclip_bootstrap_curves": (_i, [C.POINTER(BootstrapPlan), _vp, _vp, _vp, _vp, _vp, _sz]),
    "aaclip_row_head": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp] + [_i] * 6 + [_vp, _sz, _vp]),
    "aaclip_layernorm": (_i, [_vp, _vp, _vp, _vp, _i, _l, _i, _f, _vp]),
    "aaclip_gemm": (_i, [_i, _i, _vp, _l, _vp, _vp, _vp, _l, _i, _i, _i, _i, _i, _f, _vp]),
    "aaclip_attention": (_i, [_i, _vp, _vp, _i, _i, _i, _i, _vp]),
    "aaclip_attention_log2q": (_i, [_i, _vp, _vp, _i, _i, _i, _i, _vp]),
    "aaclip_adapter_mix": (_i, [_vp, _vp, _l, _i, _f, _vp]),
    "aaclip_gemm_fused": (_i, [_i, _i, _vp, _l, _vp, _vp, _vp, _l, _i, _i, _i, _i, _i, _f, C.POINTER(GemmFusedArgs), _vp]),
    "aaclip_ln_stats_finalize": (_i, [_vp, _vp, _l, _i, _f, _vp]),
    "aaclip_adapter_mix_fold": (_i, [_i, _vp, _vp, _l, _i, _f, _vp, _vp, _vp]),
    "aaclip_attention_split": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "aaclip_layernorm_split": (_i, [_vp, _vp, _vp, _vp, _l, _i, _f, _i, _vp]),
    "aaclip_split_rows": (_i, [_vp, _vp, _l, _i, _i, _vp]),
    "aaclip_small_attention": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp]),
    "aaclip_cross_rows_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "aaclip_cross_rows": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "aaclip_cross_rows_backward_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "aaclip_cross_rows_backward": (_i, [_i] + [_vp] * 5 + [_i] * 6 + [_vp, _sz, _vp]),
    "aaclip_cross_rows_levels_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "aaclip_cross_rows_levels": (_i, [_i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _l, _vp, _sz, _vp]),
    "aaclip_cross_rows_levels_backward_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "aaclip_cross_rows_levels_backward": (_i, [_i, _vp, _vp, _i, _vp, _vp, _vp] + [_i] * 7 + [_l, _vp, _sz, _vp]),
    "aaclip_head_expand": (_i, [_i, _vp, _vp, _l, _i, _i, _f, _vp]),
    "aaclip_head_diag": (_i, [_vp, _vp, _l, _i, _i, _vp]),
    "aaclip_residual_layernorm": (_i, [_vp, _vp, _vp, _vp, _vp, _l, _i, _f, _vp]),
    "aaclip_combine3": (_i, [_vp, _vp, _vp, _f, _f, _f, _vp, _l, _vp]),
    "aaclip_linear_smallk": (_i, [_i, _vp, _vp, _vp, _vp, _l, _i, _i, _vp]),
    "aaclip_small_attention_backward": (_i, [_vp] * 7 + [_i] * 5 + [_f, _vp]),
    "aaclip_layernorm_param_grad_workspace_bytes": (_sz, [_l, _i]),
    "aaclip_layernorm_param_grad": (_i, [_vp, _vp, _vp, _vp, _l, _i, _f, _vp, _sz, _vp]),
    "aaclip_bias_grad_workspace_bytes": (_sz, [_l, _i]),
    "aaclip_bias_grad": (_i, [_vp, _l, _vp, _l, _i, _vp, _sz, _vp]),
    "aaclip_act_backward": (_i, [_i, _vp, _vp, _vp, _l, _vp]),
    "aaclip_linear_smallk_backward_workspace_bytes": (_sz, [_l, _i, _i]),
    "aaclip_linear_smallk_backward": (_i, [_vp, _vp, _vp, _vp, _l, _i, _i, _vp, _sz, _vp]),
    "aaclip_drop_cls_rows": (_i, [_i, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "aaclip_iqm_map": (_i, [C.POINTER(_vp), _i, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _vp, _sz, _vp]),
    "aaclip_set_gemm_variant": (_i, [_i]),
    "aaclip_set_tail_overlap": (_i, [_i]),
    "aaclip_set_plan_cus": (_i, [_i]),
    "aaclip_tail_overlap_count": (_l, []),
    "aaclip_profile_begin": (_i, [C.c_uint, _i]),
    "aaclip_profile_end": (_i, [C.POINTER(C.c_float), C.POINTER(C.c_int), _i]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load the library once; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the AA-CLIP HIP extension has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C aa-clip-iqm_amd/csrc`). "
                "There is no PyTorch fallback for this path.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        got = lib.aaclip_version()
        if got != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} reports ABI version {got}, this binding needs {ABI_VERSION}: rebuild it "
                               "(make -C aa-clip-iqm_amd/csrc)")
        _lib = lib
    return _lib


def kernel_source_revision(files=("gemm256t.hip", "gemm.hip", "common.h", "mma16.h", "kernels.h")) -> str:
    """sha256 (first 16 hex digits) over the sources of the large-batch GEMM kernels, in the order given.  Offline
    counter measurements committed under profiles/ record it, and bench.py only reports a measurement taken on the
    sources it is running (a stale file yields traffic: null)."""
    import hashlib
    h = hashlib.sha256()
    src = os.path.join(os.path.dirname(_HERE), "csrc")
    for name in files:
        with open(os.path.join(src, name), "rb") as f:
            h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().aaclip_last_error()
        raise RuntimeError(f"aaclip {what} failed (rc={rc}): {msg.decode() if msg else ''}")
