"""ctypes binding of libtad_mi355x.so (the C ABI declared in include/tad_mi355x.h).

The product path has no CPU or PyTorch fallback: if the shared library is missing
or a symbol cannot be resolved, loading raises and every op fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TAD_LIB") or os.path.join(_HERE, "libtad_mi355x.so")  # TAD_LIB: an experiment build (simple_tad_amd/build.py)

_vp, _i, _i64, _f, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t

# name -> (restype, argtypes); mirrors include/tad_mi355x.h one-to-one
SIGNATURES = {
    "tad_abi_version": (_i, []),
    "tad_last_error_string": (C.c_char_p, []),
    "tad_cast_f32_bf16": (_i, [_vp, _vp, _i64, _vp]),
    "tad_transpose_cast_f32_bf16": (_i, [_vp, _vp, _i, _i, _vp]),
    "tad_patch_embed_ldk": (_i, [_i, _i, _i]),
    "tad_im2col_tubelets": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "tad_im2col_tubelets_16": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "tad_patch_embed_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "tad_patch_embed_fwd_implicit": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "tad_im2col_tubelets_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, C.POINTER(_f), C.POINTER(_f), _i, _i, _vp]),
    "tad_im2col_frame_windows": (_i, [_vp, _i64, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_f), C.POINTER(_f), _i, _vp]),
    "tad_patch_embed_gemm": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, _vp]),
    "tad_patch_embed_bwd_workspace_bytes": (_sz, [_i64, _i, _i]),
    "tad_patch_embed_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _i64, _i, _i, _vp]),
    "tad_layernorm_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i64, _i, _f, _vp]),
    "tad_layernorm_bwd_workspace_bytes": (_sz, [_i64, _i]),
    "tad_layernorm_bwd": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _sz, _i64, _i, _vp]),
    "tad_linear_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _sz, _i64, _i, _i, _vp]),
    "tad_linear_workspace_bytes": (_sz, [_i64, _i, _i]),
    "tad_linear_tuning": (_i, [C.c_char_p, _i]),
    "tad_linear_tuning_get": (_i, [C.c_char_p, C.POINTER(_i)]),
    "tad_linear_plan": (_i, [_i64, _i, _i, _i, _i, _i, _i, _i, _i, _i, _sz, C.POINTER(C.c_int32), _i]),
    "tad_linear_bwd_weight_plan": (_i, [_i64, _i, _i, _i, _sz, C.POINTER(C.c_int32), _i]),
    "tad_linear_fwd_qkv": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _f, _i64, _i, _i, _vp]),
    "tad_linear_bwd_weight_qkv": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _sz, _i64, _i, _i, _vp]),
    "tad_linear_bwd_weight_pair": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _sz, _i64, _i, _vp]),
    "tad_linear_debug_stamps": (_i, [_vp]),
    "tad_linear_kernel_launches": (C.c_longlong, []),
    "tad_linear_bwd_input": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _sz, _i64, _i, _i, _vp]),
    "tad_linear_bwd_weight_workspace_bytes": (_sz, [_i64, _i, _i]),
    "tad_linear_bwd_weight": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _sz, _i64, _i, _i, _vp]),
    "tad_attn_fwd": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _f, C.c_uint32, _vp]),
    "tad_attn_tuning": (_i, [C.c_char_p, _i]),
    "tad_attn_tuning_get": (_i, [C.c_char_p, C.POINTER(_i)]),
    "tad_attn_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, _f, _i, _i, C.POINTER(C.c_int32), _i]),
    "tad_attn_bwd_scratch_bytes": (_sz, [_i, _i, _i]),
    "tad_attn_debug_stamps": (_i, [_vp]),
    "tad_attn_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _f, C.c_uint32, _vp]),
    "tad_attn_colsum": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp]),
    "tad_meanpool_fwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "tad_meanpool_bwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "tad_colsum_segments": (_i, [_vp, _i, _vp, _vp, _sz, _i, _i, _i, _vp]),
    "tad_pooled_linear": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "tad_gelu_grad_bcast":(_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "tad_colsum_workspace_bytes": (_sz, [_i64, _i]),
    "tad_colsum_bf16": (_i, [_vp, _vp, _i, _vp, _sz, _i64, _i, _vp]),
    "tad_colsum_window_f32": (_i, [_vp, _vp, _i, _vp, _sz, _i, _i, _i, _i, _i, _vp]),
    "tad_scale_cast_bf16": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _vp]),
    "tad_rowscale_transpose_cast": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "tad_layerscale_grads": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "tad_branch_dropout_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _f, C.c_uint32, _i64, _i, _vp]),
    "tad_branch_dropout_cast": (_i, [_vp, _vp, _vp, _i, _f, C.c_uint32, _i64, _i, _vp]),
    "tad_sumsq_workspace_bytes": (_sz, []),
    "tad_sumsq_f32": (_i, [_vp, _i64, _vp, _vp, _sz, _vp]),
    "tad_grad_norm_coef": (_i, [_vp, _i64, _f, _f, _vp, _vp, _sz, _vp]),
    "tad_grad_segnorm_workspace_bytes": (_sz, [_i]),
    "tad_grad_segnorm_plan_check": (_i, [_vp, _i, _vp, _i, _i64, _i]),
    "tad_grad_segnorm": (_i, [_vp, _i64, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "tad_transpose_bf16_batched": (_i, [_vp, _vp, _vp, _i, _vp]),
    "tad_adamw_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, C.POINTER(_f), C.POINTER(_f), _i, C.POINTER(C.c_int32), _f, _f, _f, _vp, _vp,
                       _vp]),
    "tad_ema_update": (_i, [_vp, _i, _vp, _i, _f, _f, _vp]),
    "tad_mixup_plan_check": (_i, [_vp, _i, _i, _i, _i]),
    "tad_mixup_clips": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "tad_mixup_target": (_i, [_vp, _vp, _vp, _i, _i, _f, _f, _vp]),
    "tad_soft_target_ce": (_i, [_vp, _vp, _vp, _f, _vp, _vp, _i, _i, _vp]),
    "tad_frame_loss": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f, _vp, _vp, _i, _i, _vp]),
    "tad_erase_plan_check": (_i, [_vp, _i, _i, _i, _i, _i]),
    "tad_erase_clips": (_i, [_vp, _vp, _i, C.c_uint32, _i, _i, _i, _i, _i, _vp]),
    "tad_randaug_plan_check": (_i, [_vp, _i64, _i, _i, _i]),
    "tad_randaug_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "tad_randaug_apply": (_i, [_vp, _vp, _vp, _i, C.c_uint32, _vp, _sz, _i, _i, _i, _i, _vp]),
    "tad_frames_to_clip": (_i, [_vp, _vp, C.POINTER(_f), C.POINTER(_f), _i, _i, _i, _i, _vp]),
    "tad_multiscale_crop_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "tad_multiscale_crop_plan_check": (_i, [_vp, _i64, _i, _i, _i, _i, _i, _i, _i]),
    "tad_multiscale_crop": (_i, [_vp, _vp, _i, C.POINTER(_f), C.POINTER(_f), _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "tad_frame_resize_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "tad_frame_resize_plan_check": (_i, [_vp, _i64, _i, _i, _i, _i, _i, _i]),
    "tad_frame_resize": (_i, [_vp, _vp, _i, C.POINTER(_f), C.POINTER(_f), _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "tad_spatial_sample_workspace_bytes": (_sz, [_i, _i]),
    "tad_spatial_sample_plan_check": (_i, [_vp, _i64, _i, _i, _i, _i, _i]),
    "tad_spatial_sample": (_i, [_vp, _i, _vp, C.POINTER(_f), C.POINTER(_f), _vp, _sz, _i, _i, _i, _i, _i, _vp]),
    "tad_gather_rows_f32": (_i, [_vp, _vp, _vp, _i64, _i, _vp]),
    "tad_scatter_rows_f32": (_i, [_vp, _vp, _vp, _i64, _i, _vp]),
    "tad_mae_assemble": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "tad_mae_target": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_f), C.POINTER(_f), _i, _vp]),
    "tad_mse_loss_blocks": (_i, [_i64]),
    "tad_mse_loss": (_i, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "tad_threshold_histogram": (_i, [_vp, _vp, _vp, _i, _i64, _vp, _vp]),
    "tad_group_threshold_histogram": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i64, _vp, _vp]),
    "tad_group_rank_stats": (_i, [_vp, _vp, _vp, _i, _i64, _vp, _vp, _vp]),
    "tad_split_bf16x3": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp]),
    "tad_im2col_tubelets_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "tad_attn_fwd_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _f, C.c_uint32, _vp]),
    "tad_attn_bwd_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, C.c_uint32, _vp]),
    "tad_gelu_f32": (_i, [_vp, _vp, _i64, _vp]),
    "tad_gelu_bwd_f32": (_i, [_vp, _vp, _vp, _i64, _vp]),
    "tad_colsum_f32": (_i, [_vp, _vp, _i64, _i, _vp]),
    "tad_device_info": (_i, [C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.c_char_p, _i]),
    "tad_rccl_unique_id": (_i, [_vp]),
    "tad_rccl_init": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "tad_rccl_world_size": (_i, [_vp, C.POINTER(_i)]),
    "tad_rccl_allreduce": (_i, [_vp, _vp, _sz, _i, _i, _vp]),
    "tad_rccl_broadcast": (_i, [_vp, _vp, _sz, _i, _i, _vp]),
    "tad_rccl_destroy": (_i, [_vp]),
}

TAD_F32, TAD_BF16, TAD_F16 = 0, 1, 2

# IEEE-half twins (include/tad_mi355x.h, "IEEE half operand twins"): same signature as the bf16 entry point they mirror
F16_TWINS = {
    "tad_cast_f32_bf16": "tad_cast_f32_f16", "tad_transpose_cast_f32_bf16": "tad_transpose_cast_f32_f16",
    "tad_scale_cast_bf16": "tad_scale_cast_f16", "tad_colsum_bf16": "tad_colsum_f16", "tad_split_bf16x3": "tad_split_f16x3",
    "tad_im2col_tubelets": "tad_im2col_tubelets_f16", "tad_im2col_tubelets_u8": "tad_im2col_tubelets_u8_f16",
    "tad_patch_embed_fwd": "tad_patch_embed_fwd_f16", "tad_patch_embed_gemm": "tad_patch_embed_gemm_f16",
    "tad_patch_embed_fwd_implicit": "tad_patch_embed_fwd_implicit_f16",
    "tad_patch_embed_bwd": "tad_patch_embed_bwd_f16", "tad_layernorm_fwd": "tad_layernorm_fwd_f16",
    "tad_layernorm_bwd": "tad_layernorm_bwd_f16", "tad_linear_fwd": "tad_linear_fwd_f16", "tad_linear_fwd_qkv": "tad_linear_fwd_qkv_f16",
    "tad_linear_bwd_input": "tad_linear_bwd_input_f16", "tad_linear_bwd_weight": "tad_linear_bwd_weight_f16",
    "tad_linear_bwd_weight_qkv": "tad_linear_bwd_weight_qkv_f16", "tad_linear_bwd_weight_pair": "tad_linear_bwd_weight_pair_f16",
    "tad_attn_fwd": "tad_attn_fwd_f16", "tad_attn_bwd": "tad_attn_bwd_f16",
    "tad_meanpool_bwd": "tad_meanpool_bwd_f16", "tad_adamw_step": "tad_adamw_step_f16",
}
# the twins of the fused Block variants' kernels (csrc/layerscale.hip), a table of their own beside the 23 of the plain block
VARIANT_F16_TWINS = {
    "tad_rowscale_transpose_cast": "tad_rowscale_transpose_cast_f16", "tad_branch_dropout_cast": "tad_branch_dropout_cast_f16",
}
for _bf, _h in (*F16_TWINS.items(), *VARIANT_F16_TWINS.items()):
    SIGNATURES[_h] = SIGNATURES[_bf]
EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESIDUAL = 0, 1, 2
ABI_VERSION = 5

# The extension ABI (include/tad_mi355x_ext.h): entry points added beside the frozen core ABI, in the same library, with a version of
# their own.  name -> (restype, argtypes); the 16-bit format is an argument (TAD_BF16 / TAD_F16), so there are no twins.
EXT_SIGNATURES = {
    "tadx_abi_version": (_i, []),
    "tadx_rmsnorm_fwd": (_i, [_vp, _vp, _vp, _i, _vp, _i64, _i, _f, _vp]),
    "tadx_rmsnorm_bwd_workspace_bytes": (_sz, [_i64, _i]),
    "tadx_rmsnorm_bwd": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _sz, _i64, _i, _vp]),
    "tadx_qk_rmsnorm_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _f, _i64, _i, _f, _vp]),
    "tadx_qk_rmsnorm_bwd_workspace_bytes": (_sz, [_i64, _i]),
    "tadx_qk_rmsnorm_bwd": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _i, _vp, _sz, _i64, _i, _vp]),
}
EXT_ABI_VERSION = 1

# The pre-training ABI (include/tad_mi355x_pretrain.h): the third surface of the library, tadp_*, with a version of its own.  The
# extension ABI above is held at its seven entry points, so what MAE pre-training of the InternVideo2 family adds lives here.  f32 only.
PRETRAIN_SIGNATURES = {
    "tadp_abi_version": (_i, []),
    "tadp_visible_tokens_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "tadp_visible_tokens_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
}
PRETRAIN_ABI_VERSION = 1

# The serving ABI (include/tad_mi355x_serve.h): the fourth surface, tads_*, in a library of its own -- libtad_mi355x_serve.so, loaded beside
# the first one (the three surfaces above are held where they are).  It keeps its own error text (tads_last_error_string; check_serve).
SERVE_LIB_PATH = os.path.join(_HERE, "libtad_mi355x_serve.so")
SERVE_SIGNATURES = {
    "tads_abi_version": (_i, []),
    "tads_last_error_string": (C.c_char_p, []),
    "tads_class_token_entry_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "tads_class_token_entry_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "tads_residual_rmsnorm_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _f, _vp]),
}
SERVE_ABI_VERSION = 1

# The reconstruction ABI (include/tad_mi355x_recon.h): the fifth surface, tadr_*, in a library of its own -- libtad_mi355x_recon.so, loaded
# beside the other two (every older surface is held where it is).  It keeps its own error text (tadr_last_error_string; check_recon).
RECON_LIB_PATH = os.path.join(_HERE, "libtad_mi355x_recon.so")
RECON_SIGNATURES = {
    "tadr_abi_version": (_i, []),
    "tadr_last_error_string": (C.c_char_p, []),
    "tadr_mae_reconstruct": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_f), C.POINTER(_f), _i, _f, _vp]),
}
RECON_ABI_VERSION = 1

# The stream-bank ABI (include/tad_mi355x_bank.h): the sixth surface, tadb_*, in a library of its own -- libtad_mi355x_bank.so, loaded
# beside the other three.  It keeps its own error text (tadb_last_error_string; check_bank).
BANK_LIB_PATH = os.path.join(_HERE, "libtad_mi355x_bank.so")
BANK_SIGNATURES = {
    "tadb_abi_version": (_i, []),
    "tadb_last_error_string": (C.c_char_p, []),
    "tadb_ingest_plan_check": (_i, [_vp, _i64, _i, _i, _i, _i64, _i64, _i, _i]),
    "tadb_ingest_frames": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _vp]),
}
BANK_ABI_VERSION = 1
BANK_ROW_WORDS, BANK_MAX_FRAMES, BANK_MAX_SETS, BANK_MAX_EXTENT, BANK_SWAP_RB = 8, 4096, 64, 32768, 1

# The YUV-ingest ABI (include/tad_mi355x_yuv.h): the seventh surface, tady_*, in a library of its own -- libtad_mi355x_yuv.so, loaded
# beside the other four.  It keeps its own error text (tady_last_error_string; check_yuv).
YUV_LIB_PATH = os.path.join(_HERE, "libtad_mi355x_yuv.so")
YUV_SIGNATURES = {
    "tady_abi_version": (_i, []),
    "tady_last_error_string": (C.c_char_p, []),
    "tady_ingest_plan_check": (_i, [_vp, _i64, _i, _i, _i, _i, _i64, _i64, _i, _i]),
    "tady_ingest_yuv": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _i, _vp]),
}
YUV_ABI_VERSION = 1
YUV_ROW_WORDS, YUV_CSET_WORDS, YUV_MAX_FRAMES, YUV_MAX_SETS, YUV_MAX_CSETS, YUV_MAX_EXTENT, YUV_BGR = 16, 8, 4096, 64, 16, 32768, 1
LINEAR_PLAN_FIELDS = ("r0", "rows", "kernel", "persistent", "direct", "grid", "block", "group_m", "sk_splits", "sk_mode", "epilogue")
ATTN_PLAN_FIELDS = ("kernel", "hd", "out16", "qs", "drop", "dma_mode", "skip", "has_lo", "grid", "block")
ATTN_FWD, ATTN_FWD_Q64, ATTN_BWD_DQ, ATTN_BWD_DKV = range(4)  # the "kernel" field
LINEAR_BWD_WEIGHT_PLAN_FIELDS = ("N", "tile_k", "tiles", "tiles_k", "splits", "rows_per_split", "kernel", "grid", "block", "pair", "ws_lo", "ws_hi")
ADAMW_CHUNK = 4096
ADAMW_MAX_GROUPS = 128
EMA_CHUNK = 8192
MIXUP_PLAN_WORDS = 12
MIX_KEEP, MIX_BLEND, MIX_PASTE = 0, 1, 2
FRAME_LOSS_KINDS = {"focal": 0, "focal2": 1, "exponential": 2, "2bce": 3, "smoothap": 4}
ERASE_BOX_WORDS = 8
ERASE_CONST, ERASE_RAND, ERASE_PIXEL = 0, 1, 2
RANDAUG_ROW_WORDS = 20
RANDAUG_MAX_LAYERS = 32
(RA_COPY, RA_INVERT, RA_POSTERIZE, RA_SOLARIZE, RA_SOLARIZE_ADD, RA_AUTOCONTRAST, RA_EQUALIZE, RA_BRIGHTNESS, RA_COLOR, RA_CONTRAST,
 RA_SHARPNESS, RA_AFFINE) = range(12)
RA_STATS_OPS = (RA_AUTOCONTRAST, RA_EQUALIZE, RA_CONTRAST)
MSC_ROW_WORDS, MSC_SET_HEAD, MSC_MAX_KSIZE, MSC_MAX_SETS = 8, 4, 17, 64
SS_ROW_WORDS = 12
FR_ROW_WORDS, FR_SET_HEAD, FR_MAX_SETS, FR_MAX_ABS_SUM = 8, 4, 64, 2818
FR_NONE, FR_CONST, FR_REFLECT, FR_REPLICATE = range(4)
SEGNORM_WORK_MAX = 16384  # TAD_SEGNORM_WORK_MAX: the longest work item of tad_grad_segnorm, in floats
SEGNORM_DEPTH = 17  # the longest chain of f32 additions behind one element's square (csrc/grad_segnorm.hip, "depth")
POOL_SPLIT = 8
GROUP_MAX, GROUP_RANK_TILE = 64, 4096  # tad_group_*: the most groups of one call; TAD_GROUP_RANK_TILE, the samples per scan tile

_lib = None


class TadError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load (once) and return the shared library; raise if it is absent or incomplete."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TadError(
            f"{LIB_PATH} not found: the HIP extension has not been built. Run `python -m simple_tad_amd.build` "
            "(or __graft_entry__.build()). There is no CPU fallback for the MI355X path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in (*SIGNATURES.items(), *EXT_SIGNATURES.items(), *PRETRAIN_SIGNATURES.items()):
        try:
            fn = getattr(lib, name)
        except AttributeError as e:  # pragma: no cover
            raise TadError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    v = lib.tad_abi_version()
    if v != ABI_VERSION:
        raise TadError(f"ABI mismatch: library reports {v}, binding expects {ABI_VERSION}")
    v = lib.tadx_abi_version()
    if v != EXT_ABI_VERSION:
        raise TadError(f"extension ABI mismatch: library reports {v}, binding expects {EXT_ABI_VERSION}")
    v = lib.tadp_abi_version()
    if v != PRETRAIN_ABI_VERSION:
        raise TadError(f"pre-training ABI mismatch: library reports {v}, binding expects {PRETRAIN_ABI_VERSION}")
    for key in SIDE_LIBS:
        _load_side(key)
    _lib = lib
    return lib


# The libraries beside the first one: key -> (path, signatures, prefix of its entry points, expected <prefix>_abi_version, its name in messages)
SIDE_LIBS = {
    "serve": (SERVE_LIB_PATH, SERVE_SIGNATURES, "tads", SERVE_ABI_VERSION, "serving"),
    "recon": (RECON_LIB_PATH, RECON_SIGNATURES, "tadr", RECON_ABI_VERSION, "reconstruction"),
    "bank": (BANK_LIB_PATH, BANK_SIGNATURES, "tadb", BANK_ABI_VERSION, "stream-bank"),
    "yuv": (YUV_LIB_PATH, YUV_SIGNATURES, "tady", YUV_ABI_VERSION, "YUV-ingest"),
}
_sides = {}


def _load_side(key: str) -> C.CDLL:
    if key in _sides:
        return _sides[key]
    path, signatures, prefix, abi, human = SIDE_LIBS[key]
    if not os.path.exists(path):
        raise TadError(
            f"{path} not found: the {human} library has not been built. Run `python -m simple_tad_amd.build` "
            "(or __graft_entry__.build()). There is no CPU fallback for the MI355X path.")
    lib = C.CDLL(path)
    for name, (res, args) in signatures.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:  # pragma: no cover
            raise TadError(f"{path} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    v = getattr(lib, prefix + "_abi_version")()
    if v != abi:
        raise TadError(f"{human} ABI mismatch: library reports {v}, binding expects {abi}")
    _sides[key] = lib
    return lib


def _side_api(key: str):
    """(load_X, check_X) of a side library: loaded, and checked, together with the first one; it keeps its own error text"""
    def load_side() -> C.CDLL:
        load()
        return _sides[key]

    def check_side(rc: int, what: str = "") -> None:
        if rc != 0:
            msg = getattr(load_side(), SIDE_LIBS[key][2] + "_last_error_string")()
            raise TadError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")

    return load_side, check_side


load_serve, check_serve = _side_api("serve")  # tads_*
load_recon, check_recon = _side_api("recon")  # tadr_*
load_bank, check_bank = _side_api("bank")     # tadb_*
load_yuv, check_yuv = _side_api("yuv")        # tady_*


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().tad_last_error_string()
        raise TadError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")
