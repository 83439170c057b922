"""The pointer alignment contract of the C ABI (include/tad_mi355x.h, "Pointer alignment"), as data.  No GPU use.

One row per entry point of simple_tad_amd._lib.SIGNATURES and per ``c_void_p`` argument except the stream (workspaces, tables, optional
outputs and host-side arrays included), named as the header's prototype names it:

  A(n)      the address must be a multiple of n bytes, else the call is refused with TAD_EINVAL and a message that names the argument.
            n is the widest access the entry point's kernels make through the pointer: 16 = float4 / uint4 loads and stores and the
            16-byte global -> LDS pieces, 8 = packed stores of four 16-bit values (or float2), 4 = the 4-byte words of a uint8 / untyped
            buffer.  A(n, **{"condition": m}): under the stated condition the requirement is m instead (the access width follows a
            shape or a dtype argument); tests/alignment_cases.py builds a case for each.
  ANY       every element-aligned address works and gives the same bits (an f32 pointer on any multiple of 4, a uint8 pointer anywhere):
            the kernels read or write it one element at a time, or carry explicit code for the narrower path.
            ANY(covered="tests/...::test") : an existing test already runs that pointer at every offset; the GPU test does not repeat it.
            ANY(order=True): a reduction whose summation order moves with the address (held to fp64 within its existing bounds, not bits).
  HOST      a host array or an opaque handle: not subject to the rule.

The _f16 twins share their sources with the bf16 entry points, so their rows are the same rows (_lib.F16_TWINS, VARIANT_F16_TWINS).
tests/test_alignment_cpu.py::test_every_pointer_argument_has_a_row fails when a symbol or a pointer argument has no row here.
"""
import ctypes
import os
import re

from simple_tad_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tad_mi355x.h")


class A:
    """required bytes; ``when`` maps a stated condition to the requirement that holds under it"""

    def __init__(self, n, **when):
        assert n in (4, 8, 16, 256) and all(m in (4, 8, 16) for m in when.values())
        self.n, self.when = n, when

    def allowed(self):
        return {self.n, *self.when.values()}

    def __repr__(self):
        return f"A({self.n}" + "".join(f", {k!r}: {v}" for k, v in self.when.items()) + ")"


class _Any:
    def __init__(self, covered=None, order=False):
        self.covered, self.order = covered, order

    def __call__(self, covered=None, order=False):
        return _Any(covered, order)

    def __repr__(self):
        return "ANY"


class _Host:
    def __repr__(self):
        return "HOST"


ANY, HOST = _Any(), _Host()

_ERASE = "tests/test_erasing_gpu.py::test_same_bits_whatever_the_alignment_the_grid_and_the_batch"
_SUMSQ = "tests/test_kernels_gpu.py::test_sumsq_alignment_tails_and_grad_norm_coef"
_SEGNORM = "tests/test_grad_norms_gpu.py::test_every_length_at_every_alignment_against_float64"

_GEMM_WS = A(16)  # f32 partial tiles / slabs read and written as 16-byte pieces

CONTRACT = {
    # ---- casts and transposes (csrc/elementwise.hip)
    "tad_cast_f32_bf16": dict(src=A(16), dst=A(16)),
    "tad_transpose_cast_f32_bf16": dict(src=ANY, dst=ANY),  # one element per lane through an LDS tile
    "tad_transpose_bf16_batched": dict(src=A(16), dst=A(16), table=A(16)),  # table: int4 rows
    # ---- patch matrices (csrc/im2col.hip): wide items (patch % 8 == 0) move 16 bytes, pairs one float2 in and one 4-byte word out
    "tad_im2col_tubelets": dict(x=A(16, **{"patch % 8 != 0": 8}), cols=A(16, **{"patch % 8 != 0": 4})),
    "tad_im2col_tubelets_f32": dict(x=A(16, **{"patch % 8 != 0": 8}), cols=A(16, **{"patch % 8 != 0": 8})),
    "tad_im2col_tubelets_16": dict(x=A(16, **{"patch % 8 != 0": 4}), cols=A(16, **{"patch % 8 != 0": 4})),
    "tad_im2col_tubelets_u8": dict(frames=A(4), cols=A(16)),  # 4-byte words of the uint8 frames
    "tad_im2col_frame_windows": dict(store=A(4), idx=ANY, cols=A(16)),
    # ---- patch embedding (csrc/gemm.hip, csrc/patch_embed.hip)
    "tad_patch_embed_fwd": dict(x=A(16, **{"patch % 8 != 0": 8}), w_bf16=A(16), bias=A(16), pos=A(16), out=A(16), cols=A(16)),
    "tad_patch_embed_fwd_implicit": dict(x=A(16), w_bf16=A(16), bias=A(16), pos=A(16), out=A(16)),
    "tad_patch_embed_gemm": dict(cols=A(16), w_bf16=A(16), bias=A(16), pos=A(16), out=A(16)),
    "tad_patch_embed_bwd": dict(dy_bf16=A(16), cols=A(16), dW=A(16), db=A(16), ws=_GEMM_WS),
    # ---- LayerNorm (csrc/layernorm.hip): float4 rows, 8-byte pieces of 16-bit rows; the row statistics and scales one float at a time
    "tad_layernorm_fwd": dict(x=A(16), gamma=A(16), beta=A(16), y=A(16, **{"16-bit y_dtype": 8}), mean=ANY, rstd=ANY),
    "tad_layernorm_bwd": dict(dy=A(16, **{"16-bit dy_dtype": 8}), x=A(16), gamma=A(16), mean=ANY, rstd=ANY, dres=A(16), dx=A(16), dx_bf16=A(8),
                              dgamma=A(16), dbeta=A(16), colsum_dx=A(16), rowscale=ANY, ws=A(16)),
    # ---- Linear GEMMs (csrc/gemm.hip, gemm_kernels.h): operands by 16-byte LDS-DMA pieces; bias, outputs, pre-activation and residual by
    # 16-byte epilogue accesses; gamma and rowscale element-wise
    "tad_linear_fwd": dict(x=A(16), w=A(16), bias=A(16), y=A(16), preact=A(16), residual=A(16), gamma=ANY, rowscale=ANY, ws=_GEMM_WS),
    "tad_linear_fwd_qkv": dict(x=A(16), w=A(16), q_bias=A(16), v_bias=A(16), y=A(16)),
    "tad_linear_bwd_input": dict(dy=A(16), wT=A(16), dx=A(16), gelu_preact=A(16), ws=_GEMM_WS),
    "tad_linear_bwd_weight": dict(dy=A(16), x=A(16), dW=A(16), db=A(16), ws=_GEMM_WS),
    "tad_linear_bwd_weight_qkv": dict(dy=A(16), x=A(16), dW=A(16), dq_bias=A(16), dv_bias=A(16), ws=_GEMM_WS),
    "tad_linear_bwd_weight_pair": dict(dy1=A(16), x1=A(16), dW1=A(16), db1=A(16), db1b=A(16), dy2=A(16), x2=A(16), dW2=A(16), ws=_GEMM_WS),
    "tad_linear_debug_stamps": dict(buf=HOST),  # kept as a handle for later launches; ablation builds only
    # ---- attention (csrc/attn_fwd.hip, attn_bwd.hip, attn_colsum.hip, attn_f32.hip): 16-byte pieces of the 16-bit / f32 tensors; lse, the clip
    # scales, delta and the colsum's w / out move as single floats (4-byte LDS-DMA pieces, scalar loads and stores)
    "tad_attn_fwd": dict(qkv=A(16), out=A(16), out_lo=A(16), lse=ANY, clip_scale=ANY),
    "tad_attn_bwd": dict(qkv=A(16), out=A(16), out_lo=A(16), dout=A(16), lse=ANY, clip_scale=ANY, dqkv=A(16), delta=ANY),
    "tad_attn_debug_stamps": dict(buf=HOST),
    "tad_attn_colsum": dict(qkv=A(16), lse=ANY, w=ANY, out=ANY),
    "tad_attn_fwd_f32": dict(qkv=A(16), out=A(16), lse=ANY),
    "tad_attn_bwd_f32": dict(qkv=A(16), out=A(16), dout=A(16), lse=ANY, dqkv=A(16), delta=ANY),
    # ---- pooling and column sums (csrc/elementwise.hip, pooled_tail.hip, precise.hip)
    "tad_meanpool_fwd": dict(x=A(16), y=ANY, ws=A(16)),
    "tad_meanpool_bwd": dict(dy=A(16), dx=A(16), dx_bf16=A(8)),
    "tad_colsum_segments": dict(a=A(16), S=A(16), ws=A(16)),
    "tad_pooled_linear": dict(S=A(16), w=A(16), bias=ANY, rowscale=ANY, xbar=ANY, out=ANY),
    "tad_gelu_grad_bcast": dict(t=A(16), h=A(16), dh=A(16)),
    "tad_colsum_bf16": dict(a=A(16), out=A(16), ws=A(16)),
    "tad_colsum_window_f32": dict(a=A(16), out=A(16), ws=A(16)),
    "tad_colsum_f32": dict(a=A(16, **{"N % 4 != 0": 4}), out=ANY),  # the any-N kernel reads single floats
    # ---- element-wise helpers
    "tad_scale_cast_bf16": dict(x=A(16), y=A(8), gamma=A(16), rowscale=ANY),
    "tad_split_bf16x3": dict(x=A(16), out=A(8)),
    "tad_gelu_f32": dict(h=ANY, a=ANY),
    "tad_gelu_bwd_f32": dict(dy=ANY, h=ANY, dh=ANY),
    # ---- fused Block variants (csrc/layerscale.hip): a vector path when everything is 16-byte aligned, an element-wise one otherwise
    "tad_rowscale_transpose_cast": dict(w=ANY, gamma=ANY, out=ANY),
    "tad_layerscale_grads": dict(T=ANY, W=ANY, bias=ANY, cs=ANY, gamma=ANY, dW=ANY, dbias=ANY, dgamma=ANY),
    "tad_branch_dropout_fwd": dict(u=ANY, res=ANY, out=ANY, gamma=ANY, rowscale=ANY),
    "tad_branch_dropout_cast": dict(g=ANY, y=ANY, rowscale=ANY),
    # ---- gradient norms: x is peeled to its first 16-byte boundary, so the order of the additions follows the address
    "tad_sumsq_f32": dict(x=ANY(covered=_SUMSQ, order=True), out=ANY, ws=A(4)),
    "tad_grad_norm_coef": dict(x=ANY(order=True), out3=ANY, ws=A(4)),
    "tad_grad_segnorm_plan_check": dict(table_host=HOST, work_host=HOST),
    "tad_grad_segnorm": dict(grad=ANY(covered=_SEGNORM, order=True), table=A(8), work=A(8), coef=ANY, acc=ANY, last=ANY, counters=ANY, ws=A(4)),
    # ---- optimizer tail
    "tad_adamw_step": dict(param=A(16), grad=A(16), exp_avg=A(16), exp_avg_sq=A(16), param_bf16=A(8), chunk_group=ANY, grad_scale=ANY,
                           sumsq_partials=ANY),
    "tad_ema_update": dict(tensors=ANY, chunks=A(8)),  # chunks: int32 pairs read as one 8-byte row; the tensors' own addresses: scalar path
    # ---- augmentation and losses on the device
    "tad_mixup_plan_check": dict(plan_host=HOST),
    "tad_mixup_clips": dict(x=ANY, plan=ANY),
    "tad_mixup_target": dict(plan=ANY, labels=ANY, out=ANY),
    "tad_soft_target_ce": dict(logits=ANY, target=ANY, labels=ANY, loss=ANY, dlogits=ANY),
    "tad_frame_loss": dict(logits=ANY, labels=ANY, soft=ANY, ttc=ANY, class_alpha=ANY, loss=ANY, dlogits=ANY),
    "tad_erase_plan_check": dict(boxes_host=HOST),
    "tad_erase_clips": dict(x=ANY(covered=_ERASE), boxes=ANY),
    "tad_randaug_plan_check": dict(table_host=HOST),
    "tad_randaug_apply": dict(x=ANY, out=ANY, table=ANY, workspace=A(256)),
    "tad_frames_to_clip": dict(x=ANY, out=ANY),
    "tad_multiscale_crop_plan_check": dict(table_host=HOST),
    "tad_multiscale_crop": dict(x=ANY, out=ANY, workspace=A(4)),  # workspace = the int32 table
    "tad_frame_resize_plan_check": dict(table_host=HOST),
    "tad_frame_resize": dict(x=ANY, out=ANY, workspace=A(4)),
    "tad_spatial_sample_plan_check": dict(table_host=HOST),
    "tad_spatial_sample": dict(x=ANY, out=ANY, workspace=A(4)),
    # ---- MAE pre-training path (csrc/mae.hip): rows move as float4; index tables and the target's pixels one element at a time
    "tad_gather_rows_f32": dict(src=A(16), idx=ANY, out=A(16)),
    "tad_scatter_rows_f32": dict(src=A(16), idx=ANY, out=A(16)),
    "tad_mae_assemble": dict(x_vis=A(16), mask_token=A(16), pos=A(16), vis_idx=ANY, mask_idx=ANY, out=A(16)),
    "tad_mae_target": dict(videos=ANY, mask_idx=ANY, labels=ANY),
    "tad_mse_loss": dict(pred=A(16), target=A(16), partials=ANY, grad=A(16)),
    # ---- evaluation
    "tad_threshold_histogram": dict(probs=ANY, labels=ANY, thresholds=ANY, hist=ANY),
    "tad_group_threshold_histogram": dict(probs=ANY, labels=ANY, member=ANY, thresholds=ANY, hist=ANY),
    "tad_group_rank_stats": dict(labels_sorted=ANY, member_sorted=ANY, run_end=ANY, out_int=ANY, out_ap=ANY),
    # ---- RCCL for C hosts: host-side ids and handles; buf goes to RCCL as it is
    "tad_rccl_unique_id": dict(id128=HOST),
    "tad_rccl_init": dict(id128=HOST),
    "tad_rccl_world_size": dict(comm=HOST),
    "tad_rccl_allreduce": dict(comm=HOST, buf=HOST),
    "tad_rccl_broadcast": dict(comm=HOST, buf=HOST),
    "tad_rccl_destroy": dict(comm=HOST),
}

TWIN_OF = {half: bf for bf, half in (*_lib.F16_TWINS.items(), *_lib.VARIANT_F16_TWINS.items())}
for _half, _bf in TWIN_OF.items():
    CONTRACT[_half] = CONTRACT[_bf]


def prototypes():
    """{symbol: [argument names]} as include/tad_mi355x.h declares them"""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(tad_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        params = m.group(2).strip()
        out[m.group(1)] = [] if params in ("", "void") else [re.findall(r"[A-Za-z_0-9]+", p)[-1] for p in params.split(",")]
    return out


def pointer_arguments(symbol, protos=None):
    """[(position, name)] of the ``c_void_p`` arguments of ``symbol`` except the stream; a twin's arguments carry the names of the bf16
    prototype (``w_f16`` is ``w_bf16``: the messages and the rows name the shared source's parameter)"""
    protos = protos or prototypes()
    own, base = protos[symbol], protos[TWIN_OF.get(symbol, symbol)]
    args = _lib.SIGNATURES[symbol][1]
    assert len(own) == len(base) == len(args), f"{symbol}: the header declares {len(own)} arguments, the binding {len(args)}"
    return [(i, base[i]) for i, a in enumerate(args) if a is ctypes.c_void_p and own[i] != "stream"]


def rows(symbol, protos=None):
    """[(position, name, entry)] of ``symbol`` in signature order"""
    table = CONTRACT[symbol]
    return [(i, name, table[name]) for i, name in pointer_arguments(symbol, protos)]
