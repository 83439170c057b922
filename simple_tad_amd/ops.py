"""torch.autograd glue over the HIP kernels.  Each Function mirrors one reference operator
(modeling_finetune.py) and calls only `simple_tad_amd.kernels` (the C ABI) for arithmetic on
activations; torch is used for memory, streams, autograd bookkeeping and a few O(B) / O(D)
scalar-sized tensors (bias concatenation, drop-path masks).

Data flow of one fused Block (training), M = B*N rows:
    x0 f32 --LN1--> xn1 bf16 --qkv GEMM(+bias)--> qkv bf16 [M,3D] --flash attn--> ao bf16 [M,D]
       --proj GEMM (+bias, +residual x0)--> x1 f32 --LN2--> xn2 bf16
       --fc1 GEMM (+bias, GELU; pre-activation kept)--> a bf16 [M,4D] --fc2 GEMM (+bias, +residual x1)--> x2 f32
The residual stream stays f32 (as under torch autocast); GEMM / attention operands are bf16 with f32 accumulation.
"""
from __future__ import annotations

import contextlib
import threading
import weakref
from typing import Optional

import torch

from . import kernels as K
from ._lib import EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESIDUAL, TadError

# --------------------------------------------------------------------------- bf16 weight copies
# GEMM operands are bf16 copies of the f32 master weights (torch owns the parameters; cached copies must never outlive
# an optimizer step).  ``p._version`` cannot be the only guard: torch's fused / capturable optimizers update parameters through
# ``_fused_adamw_`` WITHOUT bumping the version counter (measured on torch 2.10: version 0 -> 0 across a fused AdamW step).  So:
#   * a forward that will be differentiated (training) always re-derives its copies from the master weights and drops any cached
#     entry for them (``fresh=True``); backward derives the transposed copy at backward time (weights do not change between the
#     two);
#   * only forwards without autograd (inference) reuse cached copies, keyed by (version, data_ptr), and ``invalidate_weight_cache``
#     (called by this package's optimizer wrapper after every step) clears them explicitly;
#   * a FROZEN weight (``requires_grad == False``, ``set_skip_frozen`` on) is in no optimizer, so nothing changes it behind autograd's
#     back: its copies are static (``_static``) in training too, made once and kept until its ``_version`` or storage, the precision
#     mode or a caller's ``invalidate_weight_cache()`` changes.  An optimizer's own step spares them (``keep_static``): it writes only
#     the parameters it holds.
_wcache = {}  # id(param) -> {"ref": weakref, "key": (version, data_ptr), kind: tensor}
_static = {}  # id(param) -> the same layout, for frozen weights in differentiated forwards / backwards
_MAKERS = {}


def invalidate_weight_cache(keep_static: bool = False):
    """Drop every cached bf16 weight copy AND every optimizer-written operand mirror (call after modifying parameters by any means
    that may not bump ``_version``: ``p.data.copy_``, a torch fused optimizer step, EMA swaps).  optim.FusedAdamW calls this and then
    re-registers the mirrors it has just rewritten.  ``keep_static``: for an optimizer's step, which leaves frozen parameters alone --
    the static copies of frozen weights survive."""
    global _weight_epoch
    _weight_epoch += 1
    _wcache.clear()
    if not keep_static:
        _static.clear()
    _mirrors.clear()
    _mirrors_t.clear()


_weight_epoch = 0


def weight_epoch() -> int:
    """bumped by every invalidate_weight_cache(): holders of captured HIP graphs compare it to know when to re-capture"""
    return _weight_epoch


def cached_weight_tensors():
    """every bf16 weight copy currently cached (a captured graph keeps this list so that the addresses it baked in stay allocated)"""
    return [v for tab in (_wcache, _static) for ent in tab.values() for k, v in ent.items() if k not in ("ref", "key")]


def _w2d(p):
    w2 = p.detach().reshape(p.shape[0], -1)
    if w2.dtype != torch.float32:
        w2 = w2.float()
    return w2 if w2.is_contiguous() else w2.contiguous()


_MAKERS["n"] = lambda p: K.cast_bf16(_w2d(p))                                  # [N,K] bf16
_MAKERS["t"] = lambda p: K.transpose_cast_bf16(_w2d(p))                        # [K,N] bf16
_MAKERS["s"] = lambda p: K.split_bf16x3(_w2d(p), role_b=True)                  # [N,3K] split operand ([hi|lo|hi]), precise Linear
_MAKERS["st"] = lambda p: K.split_bf16x3(_w2d(p).t().contiguous(), role_b=True)  # [K,3N] split operand of W^T, precise dX


# Operand mirrors: optim.FusedAdamW writes bf16(p) for every weight in the same pass that updates p and registers the views
# here; a mirror is served only while the parameter still is the tensor (same storage, same version) the optimizer wrote.
_mirrors = {}    # id(param) -> (weakref, bf16 [N,K] view, version, data_ptr)
_mirrors_t = {}  # id(param) -> (weakref, bf16 [K,N] view of W^T, version, data_ptr)


def register_mirror(p: torch.Tensor, view: torch.Tensor, transposed: bool = False):
    pid = id(p)
    tab = _mirrors_t if transposed else _mirrors
    tab[pid] = (weakref.ref(p, lambda _r, pid=pid, tab=tab: tab.pop(pid, None)), view, p._version, p.data_ptr())


def _mirror_of(p, transposed: bool = False):
    ent = (_mirrors_t if transposed else _mirrors).get(id(p))
    if ent is not None and ent[0]() is p and ent[2] == p._version and ent[3] == p.data_ptr() and ent[1].dtype == K.operand_dtype():
        return ent[1]  # (a mirror written in the other 16-bit format -- the precision mode changed after the optimizer was built -- is not served)
    return None


# Gradient sinks: when a parameter's gradient lives in a flat buffer (flat.FlatSpace, set up by parallel.DataParallel or
# optim.FusedAdamW), the weight-gradient GEMM accumulates straight into ``p.grad`` (the kernel's ``accumulate`` mode) instead
# of materialising dW and letting autograd run ``p.grad += dW`` -- one read-modify-write pass over every weight gradient and
# ~80 small launches per step less.  The Function then returns None for that parameter, so autograd's post-accumulate hooks do
# not fire; the sink's ``notify`` callback (DataParallel's bucket logic) is called instead.
_sinks = {}  # id(param) -> (weakref, flat gradient view, notify | None)


def register_grad_sink(p: torch.Tensor, view: torch.Tensor, notify=None):
    pid = id(p)
    _sinks[pid] = (weakref.ref(p, lambda _r, pid=pid: _sinks.pop(pid, None)), view, notify)


def _sink(p):
    """the flat gradient view of p if p.grad currently IS that view (f32, contiguous), else None"""
    if p is None:
        return None
    ent = _sinks.get(id(p))
    if ent is None or ent[0]() is not p or p.grad is None or p.grad.data_ptr() != ent[1].data_ptr() or torch.is_grad_enabled():
        return None  # (grad mode is on inside backward only under create_graph=True: leave that to autograd)
    return ent


def linear_dw(dy, x, w, b=None, loose_bias=False, need=(True, True)):
    """(dW, db) of a Linear for autograd.  With gradient sinks on the parameters the gradients are accumulated in place and None is
    returned in their stead.  ``loose_bias``: the column sums of dy are wanted as a tensor although there is no bias Parameter to
    sink them into (qkv: they are split into q_bias / v_bias afterwards).  ``need`` = (weight, bias): a frozen weight gets no launch
    (``x`` may be None then) and a frozen bias no column sums; a trainable bias beside a frozen weight is one column-sum launch."""
    if not need[1]:
        b, loose_bias = None, False
    if not need[0]:
        return None, (K.colsum_bf16(dy) if (b is not None or loose_bias) else None)
    sw = _sink(w)
    sb = _sink(b) if b is not None else None
    if sw is not None and (b is None or sb is not None):
        db = sb[1] if b is not None else (torch.zeros(w.shape[0], dtype=torch.float32, device=dy.device) if loose_bias else None)
        K.linear_bwd_weight(dy, x, want_bias=db is not None, dW=sw[1].view(w.shape[0], -1), db=db, accumulate=True)
        for ent, prm in ((sw, w), (sb, b)):
            if ent is not None and ent[2] is not None:
                ent[2](prm)
        return None, (db if b is None else None)
    return K.linear_bwd_weight(dy, x, want_bias=(b is not None or loose_bias))


def layernorm_bwd_sunk(dy, x, gamma, mean, rstd, w, b, colsum_param=None, **kw):
    """K.layernorm_bwd whose reductions (dgamma, dbeta and, with ``colsum_param``, the column sums = that bias's gradient) go into
    the parameters' gradient sinks when all of them have one.  Returns (dx, dx_bf16, dgamma|None, dbeta|None, colsum|None)."""
    ents = [_sink(w), _sink(b)] + ([_sink(colsum_param)] if colsum_param is not None else [])
    if all(e is not None for e in ents):
        dx, dxb, _, _, _ = K.layernorm_bwd(dy, x, gamma, mean, rstd, want_colsum=colsum_param is not None,
                                           into=(ents[0][1], ents[1][1], ents[2][1] if colsum_param is not None else None), **kw)
        for ent, prm in zip(ents, (w, b, colsum_param)):
            if ent[2] is not None:
                ent[2](prm)
        return dx, dxb, None, None, None
    return K.layernorm_bwd(dy, x, gamma, mean, rstd, want_colsum=colsum_param is not None, **kw)


def _cached(p: torch.Tensor, kind: str, fresh: bool = False):
    pid = id(p)
    if kind in ("n", "t"):
        m = _mirror_of(p, kind == "t")
        if m is not None:
            return m
    tab = _wcache
    if fresh:
        _wcache.pop(pid, None)
        if p.requires_grad or not _skip_frozen or kind not in ("n", "t"):
            if _static:
                _static.pop(pid, None)  # (a weight that was frozen once and trains again)
            return _MAKERS[kind](p)
        tab = _static  # a frozen weight: nothing updates it between steps
    elif not p.requires_grad and _skip_frozen and kind in ("n", "t") and getattr(_outer, "grad", None):
        # a forward under grad mode none of whose inputs is differentiable (a wholly frozen patch embedding, the blocks of a linear
        # probe) is part of a training step all the same; without grad mode (inference, evaluation) the cache above serves as before
        tab = _static
    ent = tab.get(pid)
    key = (p._version, p.data_ptr())
    if ent is None or ent["ref"]() is not p or ent["key"] != key:
        ent = {"ref": weakref.ref(p, lambda _r, pid=pid, tab=tab: tab.pop(pid, None)), "key": key}
        tab[pid] = ent
    if kind not in ent:
        ent[kind] = _MAKERS[kind](p)
    return ent[kind]


def w_bf16(p, fresh: bool = False):
    return _cached(p, "n", fresh)


def wT_bf16(p, fresh: bool = False):
    return _cached(p, "t", fresh)


def _f32c(t: Optional[torch.Tensor]):
    if t is None:
        return None
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _need_gpu(x: torch.Tensor, what: str):
    if not x.is_cuda:
        raise TadError(f"{what}: input is on {x.device}; the MI355X path runs HIP kernels only (no CPU fallback). "
                       "Move the model and inputs to a GPU.")


def _qkv_bias(q_bias, v_bias):
    if q_bias is None:
        return None
    return torch.cat((q_bias.detach(), torch.zeros_like(v_bias), v_bias.detach())).float().contiguous()


# --------------------------------------------------------------------------- precise mode (parity gate)
def _cached_split(p: torch.Tensor, fresh: bool = False):
    return _cached(p, "s", fresh)


# --------------------------------------------------------------------------- precision mode
_PRECISION = "fast"


def set_precision(mode: str):
    """Numerics of the MFMA path.
    "fast":    bfloat16 operands, f32 accumulation / residual stream / statistics -- the benchmarked default.
    "half":    IEEE-half operands through the same kernels (tad_*_f16): 8x smaller operand rounding at the same MFMA rate.  This is the
               reference's own arithmetic -- torch.cuda.amp.autocast() is float16 on CUDA (engine_for_finetuning.py:67) -- and like
               there the backward pass needs loss scaling: engine.NativeScalerWithGradNormCount scales the loss, and the fused AdamW
               removes the scale and skips overflowed steps (utils.py:386-412).
    "precise": split-bf16 (hi + lo, three MFMA products) Linears, f32 attention and f32 activations -- the parity gate."""
    global _PRECISION
    if mode not in ("fast", "half", "precise"):
        raise ValueError(mode)
    if mode != _PRECISION:
        invalidate_weight_cache()  # cached operand copies are in the old format
    _PRECISION = mode
    K.set_operand_dtype(torch.float16 if mode == "half" else torch.bfloat16)


def get_precision() -> str:
    return _PRECISION


def _no_grad_only(*tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise TadError('precision "precise" is forward-only (parity gate); wrap the call in torch.no_grad()')


def _cached_split_T(p: torch.Tensor, fresh: bool = False):
    return _cached(p, "st", fresh)


def precise_dx(dy, weight):
    """dx [M,K] f32 = dy [M,N] @ W [N,K] with split operands (reduction over 3N); backward only, so the copy is always re-derived"""
    dx, _ = K.linear_fwd(K.split_bf16x3(dy, role_b=False), _cached_split_T(weight, True), None, out_dtype=torch.float32)
    return dx


def precise_dw(dy, x, want_bias=True):
    """dW [N,K] = dy^T x with both operands split and stacked along the reduction (row) dimension; db = column sums of dy"""
    dW, _ = K.linear_bwd_weight(K.split_bf16x3(dy, role_b=False, stack=True), K.split_bf16x3(x, role_b=True, stack=True), want_bias=False)
    return dW, (K.colsum_f32(dy) if want_bias else None)


def precise_linear(x2d, weight, bias, epilogue=EPI_BIAS, residual=None, rowscale=None, rows_per_scale=1, fresh=False):
    xs = K.split_bf16x3(x2d, role_b=False)
    y, _ = K.linear_fwd(xs, _cached_split(weight, fresh), _f32c(bias), out_dtype=torch.float32, epilogue=epilogue, residual=residual,
                        rowscale=rowscale, rows_per_scale=rows_per_scale)
    return y


def precise_attention(x2d, B, N, qkv_w, q_bias, v_bias, proj_w, proj_b, H, scale, residual=None):
    qkv = precise_linear(x2d, qkv_w, _qkv_bias(q_bias, v_bias))
    ao, _ = K.attn_fwd_f32(qkv, B, N, H, scale, d=head_dim_of(qkv_w, H))
    return precise_linear(ao, proj_w, proj_b, EPI_BIAS_RESIDUAL if residual is not None else EPI_BIAS, residual=residual)


def precise_mlp(x2d, fc1_w, fc1_b, fc2_w, fc2_b, residual=None):
    a = precise_linear(x2d, fc1_w, fc1_b, EPI_BIAS_GELU)
    return precise_linear(a, fc2_w, fc2_b, EPI_BIAS_RESIDUAL if residual is not None else EPI_BIAS, residual=residual)


def precise_block(x, n1w, n1b, qkv_w, q_bias, v_bias, proj_w, proj_b, n2w, n2b, fc1_w, fc1_b, fc2_w, fc2_b, H, scale, eps):
    return PreciseBlockFn.apply(x, n1w, n1b, qkv_w, q_bias, v_bias, proj_w, proj_b, n2w, n2b, fc1_w, fc1_b, fc2_w, fc2_b, H, scale, eps)


def precise_patch_embed(x, weight, bias, pos, tubelet, patch):
    return PrecisePatchEmbedFn.apply(x, weight, bias, pos, tubelet, patch)




# --------------------------------------------------------------------------- grad mode seen by the CALLER of a Function
# Inside Function.forward autograd has switched grad mode off and ctx.needs_input_grad is True for every Parameter even under
# torch.no_grad(), so "will this forward be differentiated?" (decides whether cached bf16 weight copies may be reused, whether
# pre-activations / statistics are kept) has to be sampled before apply().
_outer = threading.local()


class _Fn(torch.autograd.Function):
    @classmethod
    def apply(cls, *args, **kwargs):
        prev = getattr(_outer, "grad", None)
        _outer.grad = torch.is_grad_enabled()
        try:
            return super().apply(*args, **kwargs)
        finally:
            _outer.grad = prev


def _differentiated(ctx) -> bool:
    g = getattr(_outer, "grad", None)
    return (True if g is None else g) and any(ctx.needs_input_grad)



# --------------------------------------------------------------------------- frozen parameters
# A parameter with ``requires_grad == False`` (engine.freeze_layers) gets no weight-gradient launch and no bias column sums, its
# Function returns None for it, and the forward keeps none of the operands only that gradient would read (xn1 / xn2 / a of a Block,
# the patch matrix).  The input-gradient chain is the same launches on the same bits.  Off: every gradient is computed and every
# operand kept whatever the flags say, and frozen weights are re-cast every step (the path before the switch existed; tests, A/B runs).
_skip_frozen = True


def set_skip_frozen(enabled: bool):
    """honour ``requires_grad`` per parameter in the 16-bit Functions (default) or, off, compute and save everything.  Sampled by each
    forward: an autograd node's backward follows the setting its own forward ran under."""
    global _skip_frozen
    _skip_frozen = bool(enabled)


def get_skip_frozen() -> bool:
    return _skip_frozen


def _needs(ctx, n: int):
    """per input 0..n-1 of a Function: may its gradient be wanted?  (ctx.needs_input_grad, or all True with the switch off; an absent
    -- None -- parameter is the callers' affair either way)"""
    if not _skip_frozen:
        return (True,) * n
    return tuple(bool(f) for f in ctx.needs_input_grad[:n])


# --------------------------------------------------------------------------- LayerNorm
class LayerNormFn(_Fn):
    """nn.LayerNorm(D, eps) on f32 rows -> f32 (modeling_finetune.py:143,149,270)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        _need_gpu(x, "LayerNorm")
        xc = _f32c(x)
        w, b = _f32c(weight), _f32c(bias)
        y, mean, rstd = K.layernorm_fwd(xc.reshape(-1, xc.shape[-1]), w, b, eps, out_dtype=torch.float32)
        ctx.save_for_backward(xc, w, mean, rstd)
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        xc, w, mean, rstd = ctx.saved_tensors
        D = xc.shape[-1]
        dx, _, dg, db, _ = K.layernorm_bwd(_f32c(dy).reshape(-1, D), xc.reshape(-1, D), w, mean, rstd)
        return dx.reshape(xc.shape), dg, db, None


# --------------------------------------------------------------------------- PatchEmbed (+ pos_embed)
# The implicit patch embedding (tad_patch_embed_fwd_implicit) is taken by forwards without a backward pass once the problem fills the chip: measured
# (tools/bench_kernels.py --only patch, us, explicit / implicit): 32 clips D = 768 264 / 245, D = 384 193 / 152, ONE clip (78 tiles of 128 x 128 on 256
# CUs, 24 dependent K-tiles each) 23 / 33 -- below two tiles per CU the im2col + GEMM pair is faster
IMPLICIT_PATCH_EMBED_MIN_TILES = 512


def _patch_embed_backward(ctx, dy, trailing: int):
    """(dweight, dbias) of a 16-bit patch embedding from its saved patch matrix, then ``trailing`` Nones for the inputs after bias"""
    weight, bias = ctx.params
    need_w, need_b = ctx.need
    need_b = need_b and bias is not None
    if not (need_w or need_b):
        return (None, None) + (None,) * trailing
    dyb = K.cast_bf16(_f32c(dy).reshape(-1, dy.shape[-1]))
    if not need_w:  # a frozen projection: no patch matrix was kept
        return (None, K.colsum_bf16(dyb)) + (None,) * trailing
    (cols,) = ctx.saved_tensors
    if not need_b:
        bias = None
    kw = weight.numel() // weight.shape[0]
    if cols.shape[1] != kw:  # padded K: the gradient of the padding columns is dropped (no in-place sink for a [D, ldk] result)
        dWp, db = K.linear_bwd_weight(dyb, cols, want_bias=bias is not None)
        dW = dWp[:, :kw]
    else:
        dW, db = linear_dw(dyb, cols, weight, bias)
    return (None if dW is None else dW.reshape(weight.shape), db) + (None,) * trailing


class PatchEmbedFn(_Fn):
    """Conv3d(k=s=(tub,p,p)) + flatten/transpose (+ sinusoid pos_embed) (modeling_finetune.py:181-190, 312-313)."""

    @staticmethod
    def forward(ctx, x, weight, bias, pos, tubelet, patch):
        _need_gpu(x, "PatchEmbed")
        xc = _f32c(x)
        # patch sizes whose K = C*tub*p*p is not a multiple of 64 (ViT-L/14: 1176): the patch matrix and the weight operand carry zero
        # columns up to tad_patch_embed_ldk (1216); a pure configuration change for the callers
        ldk = K.patch_embed_ldk(xc.shape[1], tubelet, patch)
        ntok_ = (xc.shape[2] // tubelet) * (xc.shape[3] // patch) * (xc.shape[4] // patch)
        ctx.need = _needs(ctx, 3)[1:]
        keeps_cols = _differentiated(ctx) and ctx.need[0]
        if not keeps_cols and -(-xc.shape[0] * ntok_ // 128) * -(-weight.shape[0] // 128) >= IMPLICIT_PATCH_EMBED_MIN_TILES:
            # nothing is kept for a backward pass (eval / no_grad / inference, or a frozen projection): the implicit GEMM
            # reads the clip itself and writes no patch matrix; bit-identical to the explicit form below, which the training step needs
            # for its weight gradient
            out = K.patch_embed_fwd_implicit(xc, w_bf16(weight, _differentiated(ctx)), _f32c(bias), _f32c(pos), tubelet, patch)
            if out is not None:
                ctx.params = (weight, bias)
                return out
        out, cols = K.patch_embed_fwd(xc, K.pad_k(w_bf16(weight, _differentiated(ctx)), ldk), _f32c(bias), _f32c(pos), tubelet, patch)
        if ctx.need[0]:
            ctx.save_for_backward(cols)
        ctx.params = (weight, bias)
        return out

    @staticmethod
    def backward(ctx, dy):
        return (None,) + _patch_embed_backward(ctx, dy, 3)  # x | weight, bias | pos, tubelet, patch


class PatchEmbed16Fn(_Fn):
    """PatchEmbed on a clip [B,C,T,H,W] that already is in the current 16-bit operand format (a loader that ships bf16 / half clips:
    prefetch.ClipPrefetcher wire="operand"): the patch matrix is a move of the clip's words (K.im2col_tubelets_16) -- the same bits as
    PatchEmbedFn on the upcast clip without its f32 round trip; the same saved ``cols`` and the same backward.  Always the explicit route:
    the implicit GEMM reads f32 clips only."""

    @staticmethod
    def forward(ctx, x, weight, bias, pos, tubelet, patch):
        _need_gpu(x, "PatchEmbed")
        xc = x.detach()
        xc = xc if xc.is_contiguous() else xc.contiguous()
        cols = K.im2col_tubelets_16(xc, tubelet, patch)
        if cols is None:  # a misaligned view: the f32 route computes the same patch matrix
            cols = K.im2col_tubelets(xc.float(), tubelet, patch, dtype=xc.dtype)
        ntok = (xc.shape[2] // tubelet) * (xc.shape[3] // patch) * (xc.shape[4] // patch)
        out = K.patch_embed_gemm(cols, K.pad_k(w_bf16(weight, _differentiated(ctx)), cols.shape[1]), _f32c(bias), _f32c(pos), ntok)
        ctx.need = _needs(ctx, 3)[1:]
        if ctx.need[0]:
            ctx.save_for_backward(cols)
        ctx.params = (weight, bias)
        return out

    @staticmethod
    def backward(ctx, dy):
        return (None,) + _patch_embed_backward(ctx, dy, 3)  # x | weight, bias | pos, tubelet, patch


class PatchEmbedU8Fn(_Fn):
    """PatchEmbed on uint8 frames [B,T,H,W,3]: normalisation (run_inference.py:15-34; dota.py:443-460) fused into the im2col."""

    @staticmethod
    def forward(ctx, frames, weight, bias, pos, tubelet, patch, mean, std, bgr, t_offset):
        _need_gpu(frames, "PatchEmbed")
        fr = frames if frames.is_contiguous() else frames.contiguous()
        B, T, H, W, _ = fr.shape
        cols = K.im2col_tubelets_u8(fr, tubelet, patch, mean, std, bgr, t_offset)   # row stride tad_patch_embed_ldk (zero-padded for /14)
        ntok = (T // tubelet) * (H // patch) * (W // patch)
        out = K.patch_embed_gemm(cols, K.pad_k(w_bf16(weight, _differentiated(ctx)), cols.shape[1]), _f32c(bias), _f32c(pos), ntok)
        ctx.need = _needs(ctx, 3)[1:]
        if ctx.need[0]:
            ctx.save_for_backward(cols)
        ctx.params = (weight, bias)
        return out

    @staticmethod
    def backward(ctx, dy):
        return (None,) + _patch_embed_backward(ctx, dy, 7)  # frames | weight, bias | pos, tubelet, patch, mean, std, bgr, t_offset


class PatchEmbedWindowsFn(_Fn):
    """PatchEmbed on B windows of ONE device-resident frame store (frame_store.FrameWindows): PatchEmbedU8Fn with the patch matrix read
    through an index table [B,T] instead of from materialised clips (K.im2col_frame_windows: bit-identical to
    K.im2col_tubelets_u8(store[idx])); the same saved ``cols`` and the same backward, so training from a store costs nothing extra."""

    @staticmethod
    def forward(ctx, store, idx, weight, bias, pos, tubelet, patch, mean, std, bgr):
        _need_gpu(store, "PatchEmbed")
        B, T = idx.shape
        _, H, W, _ = store.shape
        cols = K.im2col_frame_windows(store, idx, tubelet, patch, mean, std, bgr)   # row stride tad_patch_embed_ldk (zero-padded for /14)
        ntok = (T // tubelet) * (H // patch) * (W // patch)
        out = K.patch_embed_gemm(cols, K.pad_k(w_bf16(weight, _differentiated(ctx)), cols.shape[1]), _f32c(bias), _f32c(pos), ntok)
        ctx.need = _needs(ctx, 4)[2:]
        if ctx.need[0]:
            ctx.save_for_backward(cols)
        ctx.params = (weight, bias)
        return out

    @staticmethod
    def backward(ctx, dy):
        return (None, None) + _patch_embed_backward(ctx, dy, 6)  # store, idx | weight, bias | pos, tubelet, patch, mean, std, bgr


# --------------------------------------------------------------------------- attention / mlp cores (2-D tensors)
def head_dim_of(qkv_w, H):
    return qkv_w.shape[0] // (3 * H)


# The attention forward also writes what the 16-bit rounding of its output dropped (77 MB per ViT-B layer at 32 clips), and the
# backward takes delta = rowsum(dO * O) of the unrounded output: see tad_attn_bwd.  Off: delta from the rounded output, as flash-attn.
_attn_exact_delta = True


_attn_q_prescale = True  # the qkv Linear writes q * scale * log2(e) (False: plain q, the kernels scale their fragments; for A/B runs)


def set_attn_q_prescale(on: bool):
    """takes effect at the next forward; every autograd node remembers the contract its own forward ran under (ctx.qpre), so a toggle
    between a forward and its backward cannot mis-read the saved qkv"""
    global _attn_q_prescale
    _attn_q_prescale = bool(on)


def get_attn_q_prescale() -> bool:
    return _attn_q_prescale


def set_attn_exact_delta(on: bool):
    global _attn_exact_delta
    _attn_exact_delta = bool(on)


_attn_hd80_f32 = False


def set_attn_hd80_f32(on: bool):
    """A/B switch: head_dim 80 attention through the exact-f32 MFMA kernels (the round-3 route) instead of the 16-bit ones"""
    global _attn_hd80_f32
    _attn_hd80_f32 = bool(on)


_attn_capture = None  # the list of the active capture_attention(), or None


def attention_capture_active() -> bool:
    return _attn_capture is not None


@contextlib.contextmanager
def capture_attention(model=None):
    """Context manager that yields a list; while it is active every attention call of an evaluation forward (all block routes go through
    ``_attn_fwd_core``) appends one record ``(qkv, lse, B, N, H, d, scale, q_prescaled)``: what ``kernels.attn_colsum`` needs to recompute
    that layer's softmax (simple_tad_amd/explain.py).  lse is a nullable output of the same forward kernel, so the logits under capture are
    those of the plain evaluation forward, bit for bit.  Evaluation only: raises TadError in "precise" mode, when grad is enabled, when the
    model (``model``, if given, at entry; otherwise its attention modules as they run) is in training mode, on the set_attn_hd80_f32 route
    (qkv is f32 there), and when a capture is already active (captures do not nest)."""
    global _attn_capture
    if _attn_capture is not None:
        raise TadError("capture_attention: a capture is already active (captures do not nest)")
    if _PRECISION == "precise":
        raise TadError('capture_attention: precision "precise" runs the f32 attention kernels, which keep no 16-bit qkv to recompute from')
    if torch.is_grad_enabled():
        raise TadError("capture_attention: evaluation only; wrap the call in torch.no_grad()")
    if model is not None and model.training:
        raise TadError("capture_attention: the model is in training mode (call model.eval(): the records are those of the evaluation forward)")
    records = []
    _attn_capture = records
    try:
        yield records
    finally:
        _attn_capture = None


def _attn_fwd_core(xn, qkv_w, q_bias, v_bias, B, N, H, scale, train, drop=(0.0, 0), rowscale=None):
    """returns qkv, attention output, (lse, rounding residual of the output | None).  drop = (p, seed) of attention dropout.
    rowscale: the per-clip drop-path scale [B] of the residual behind the branch (K.attn_fwd)."""
    hd = head_dim_of(qkv_w, H)
    if hd not in (64, 80):
        raise TadError(f"attention: head_dim {hd} has no kernel (64 and 80 do)")
    cap = _attn_capture
    if cap is not None:  # (refusals before any device work)
        if train or _PRECISION == "precise" or drop[0] > 0:
            raise TadError("capture_attention: evaluation only (no grad, no training mode, not the precise mode)")
        if hd == 80 and _attn_hd80_f32:
            raise TadError("capture_attention: the set_attn_hd80_f32 route keeps an f32 qkv; attn_colsum reads 16-bit operands")
    qb = None if q_bias is None else _f32c(q_bias.detach())
    vb = None if v_bias is None else _f32c(v_bias.detach())
    if hd == 80 and _attn_hd80_f32:
        # The round-3 route for the "huge" configurations (head_dim 80, modeling_finetune.py:390-398), kept for A/B runs
        # (set_attn_hd80_f32): the Linears stay on the 16-bit MFMA GEMMs, the scaled-dot-product core runs through the exact-f32 MFMA
        # kernels (csrc/attn_f32.hip) on an f32 qkv.  Since round 4 head_dim 80 has 16-bit kernels of its own (the branch below).
        qkv = K.linear_fwd_qkv(xn, w_bf16(qkv_w, train), qb, vb, out_dtype=torch.float32)
        ao32, lse = K.attn_fwd_f32(qkv, B, N, H, scale, want_lse=train, d=hd, drop_p=drop[0], seed=drop[1])
        return qkv, K.cast_bf16(ao32), (lse, None)
    # `q = q * self.scale` (modeling_finetune.py:96) rides in the qkv Linear's epilogue, together with log2(e): the attention kernels
    # get their scores from the matrix pipe in log2 units and spend no vector instruction on the scale (the q third of `qkv` is NOT
    # the plain q; only tad_attn_fwd / tad_attn_bwd read it)
    qkv = K.linear_fwd_qkv(xn, w_bf16(qkv_w, train), qb, vb, out_dtype=None, q_prescale=K.q_prescale_of(scale) if _attn_q_prescale else 1.0)
    r = K.attn_fwd(qkv, B, N, H, scale, out_dtype=None, want_lse=train or cap is not None, want_lo=train and _attn_exact_delta,
                   q_prescaled=_attn_q_prescale, drop_p=drop[0], seed=drop[1], d=hd, rowscale=rowscale)
    if cap is not None:
        cap.append((qkv, r[1], B, N, H, hd, float(scale), bool(_attn_q_prescale)))
    return qkv, r[0], (r[1], r[2] if len(r) > 2 else None)


def _attn_bwd_core(d_ao, xn, qkv, ao, lse, qkv_w, has_qkv_bias, B, N, H, scale, dx_dtype, qv_params=None, ao_lo=None, drop=(0.0, 0),
                   q_prescaled=None, pair=None, rowscale=None, need=(True, True, True), pair_need=True):
    """returns dxn, dWqkv, dq_bias, dv_bias (None for what went into gradient sinks).  q_prescaled: the q contract of the forward
    that produced `qkv` (ctx.qpre).  pair = (dy, x, w) of ANOTHER bias-less weight gradient over the same rows with the same K that is due
    (the Block's proj: dy = the 16-bit gradient of its output, x = the attention output): a fifth value is returned then, that Linear's dW
    (None if it went into its gradient sink).  With sinks on all parameters the two weight gradients run as ONE launch
    (K.linear_bwd_weight_pair: a 768 x 768 gradient alone fills the chip with 9 tiles x 28 reduction shares, the pair with 36 x 7).
    need = (qkv weight, q_bias, v_bias), pair_need: which of these gradients are wanted at all (frozen parameters: no launch, None;
    ``xn`` may be None without the weight's).  The pair launch runs when both weights want theirs, the single launch when one does."""
    if q_prescaled is None:
        q_prescaled = _attn_q_prescale
    if qkv.dtype == torch.float32:  # generic head dim (see _attn_fwd_core)
        dqkv = K.cast_bf16(K.attn_bwd_f32(qkv, ao.float(), d_ao.float(), lse, B, N, H, scale, d=head_dim_of(qkv_w, H), drop_p=drop[0],
                                          seed=drop[1]))
    else:
        dqkv = K.attn_bwd(qkv, ao, d_ao, lse, B, N, H, scale, out_lo=ao_lo, q_prescaled=q_prescaled, drop_p=drop[0], seed=drop[1],
                          d=head_dim_of(qkv_w, H), rowscale=rowscale)
    dxn = K.linear_bwd_input(dqkv, wT_bf16(qkv_w, True), out_dtype=dx_dtype)

    def done(*r):  # (+ the pair's weight gradient by itself when it did not ride along)
        return r if pair is None else r + (linear_dw(pair[0], pair[1], pair[2], need=(pair_need, False))[0],)

    need_w, need_q, need_v = need[0], has_qkv_bias and need[1], has_qkv_bias and need[2]
    if not need_w:
        if not (need_q or need_v):
            return done(dxn, None, None, None)
        cs = K.colsum_bf16(dqkv)  # trainable biases beside a frozen weight: the column sums alone
        AH = cs.numel() // 3
        return done(dxn, None, cs[:AH].clone() if need_q else None, cs[2 * AH:].clone() if need_v else None)
    if need_q and need_v and qv_params is not None:
        ents = [_sink(qkv_w), _sink(qv_params[0]), _sink(qv_params[1])]
        if all(e is not None for e in ents):
            # dW, dq_bias and dv_bias accumulate straight into the flat gradient buffer: no [3D] temporary, no slicing copies, no
            # autograd accumulation kernels
            prms = (qkv_w,) + tuple(qv_params)
            sp = _sink(pair[2]) if pair is not None and pair_need else None
            paired = sp is not None and pair[0].dtype == dqkv.dtype and pair[1].shape == xn.shape and pair[0].shape[0] == dqkv.shape[0]
            if paired:
                K.linear_bwd_weight_pair(dqkv, xn, ents[0][1].view(qkv_w.shape[0], -1), ents[1][1], ents[2][1], pair[0], pair[1],
                                         sp[1].view(pair[2].shape[0], -1), accumulate=True)
                ents, prms = ents + [sp], prms + (pair[2],)
            else:
                K.linear_bwd_weight_qkv(dqkv, xn, ents[0][1].view(qkv_w.shape[0], -1), ents[1][1], ents[2][1], accumulate=True)
            for ent, prm in zip(ents, prms):
                if ent[2] is not None:
                    ent[2](prm)
            if paired:
                return dxn, None, None, None, None
            return done(dxn, None, None, None)
    dWqkv, dbqkv = linear_dw(dqkv, xn, qkv_w, None, loose_bias=need_q or need_v)
    if dbqkv is not None:
        AH = dbqkv.numel() // 3
        return done(dxn, dWqkv, dbqkv[:AH].clone() if need_q else None, dbqkv[2 * AH:].clone() if need_v else None)
    return done(dxn, dWqkv, None, None)


class AttentionFn(_Fn):
    """Attention.forward (modeling_finetune.py:86-134): qkv Linear, scaled-dot-product space-time attention, proj."""

    @staticmethod
    def forward(ctx, x, qkv_w, q_bias, v_bias, proj_w, proj_b, H, scale, drop_p=0.0, drop_seed=0):
        _need_gpu(x, "Attention")
        B, N, C = x.shape
        train = _differentiated(ctx)
        ctx.drop = (float(drop_p), int(drop_seed))
        xb = K.cast_bf16(_f32c(x).reshape(B * N, C))
        qkv, ao, (lse, ao_lo) = _attn_fwd_core(xb, qkv_w, q_bias, v_bias, B, N, H, scale, train, ctx.drop)
        ctx.qpre = _attn_q_prescale  # (the contract `qkv` was written under: read back by the backward)
        y, _ = K.linear_fwd(ao, w_bf16(proj_w, train), _f32c(proj_b), out_dtype=torch.float32)
        ctx.need = _needs(ctx, 6)
        if train:
            ctx.save_for_backward(xb if ctx.need[1] else None, qkv, ao, lse, qkv_w, proj_w, ao_lo)
        ctx.meta = (B, N, H, scale, q_bias is not None, proj_b is not None)
        ctx.proj_b = proj_b
        ctx.qv = (q_bias, v_bias)
        return y.reshape(B, N, -1)

    @staticmethod
    def backward(ctx, dy):
        xb, qkv, ao, lse, qkv_w, proj_w, ao_lo = ctx.saved_tensors
        B, N, H, scale, has_qb, has_pb = ctx.meta
        dyb = K.cast_bf16(_f32c(dy).reshape(B * N, -1))
        d_ao = K.linear_bwd_input(dyb, wT_bf16(proj_w, True))
        dWp, dbp = linear_dw(dyb, ao, proj_w, ctx.proj_b, need=ctx.need[4:6])
        dx, dWqkv, dqb, dvb = _attn_bwd_core(d_ao, xb, qkv, ao, lse, qkv_w, has_qb, B, N, H, scale, torch.float32, ctx.qv, ao_lo=ao_lo,
                                             drop=ctx.drop, q_prescaled=ctx.qpre, need=ctx.need[1:4])
        return dx.reshape(B, N, -1), dWqkv, dqb, dvb, dWp, dbp, None, None, None, None


class MlpFn(_Fn):
    """Mlp.forward (modeling_finetune.py:47-54): fc2(GELU_erf(fc1(x)))."""

    @staticmethod
    def forward(ctx, x, fc1_w, fc1_b, fc2_w, fc2_b):
        _need_gpu(x, "Mlp")
        shp = x.shape
        train = _differentiated(ctx)
        # (an input that already is the 16-bit operand -- RMSNormFn's out16 -- is read as it is, and gets its gradient in that format)
        ctx.x16 = x.dtype == K.operand_dtype()
        xb = _op16_rows(x)
        a, h = K.linear_fwd(xb, w_bf16(fc1_w, train), _f32c(fc1_b), out_dtype=None, epilogue=EPI_BIAS_GELU, want_preact=train)
        y, _ = K.linear_fwd(a, w_bf16(fc2_w, train), _f32c(fc2_b), out_dtype=torch.float32)
        ctx.need = _needs(ctx, 5)
        if train:
            ctx.save_for_backward(xb if ctx.need[1] else None, h, a if ctx.need[3] else None, fc1_w, fc2_w)
        ctx.meta = (shp, fc1_b is not None, fc2_b is not None)
        ctx.biases = (fc1_b, fc2_b)
        return y.reshape(*shp[:-1], -1)

    @staticmethod
    def backward(ctx, dy):
        xb, h, a, fc1_w, fc2_w = ctx.saved_tensors
        shp, has_b1, has_b2 = ctx.meta
        dyb = K.cast_bf16(_f32c(dy).reshape(-1, dy.shape[-1]))
        dh = K.linear_bwd_input(dyb, wT_bf16(fc2_w, True), gelu_preact=h)
        dW2, db2 = linear_dw(dyb, a, fc2_w, ctx.biases[1], need=ctx.need[3:5])
        dx = K.linear_bwd_input(dh, wT_bf16(fc1_w, True), out_dtype=None if ctx.x16 else torch.float32)
        dW1, db1 = linear_dw(dh, xb, fc1_w, ctx.biases[0], need=ctx.need[1:3])
        return dx.reshape(shp), dW1, db1, dW2, db2


# --------------------------------------------------------------------------- InternVideo2: RMSNorm, attention with q / k normalisation
# (other_models/InternVideo2_single_modality/models/internvideo2.py; kernels: csrc/rmsnorm.hip through the extension ABI)
_iv2_kernels = True


def set_iv2_kernels(enabled: bool):
    """A/B switch: the two norms of the InternVideo2 family (RMSNormFn, the q / k normalisation inside IV2AttentionFn) through their HIP
    kernels (default) or, off, through the torch expressions of the same arithmetic.  Everything else -- Linears, attention, what is
    saved -- is unchanged.  Sampled by each forward; a node's backward follows its own forward."""
    global _iv2_kernels
    _iv2_kernels = bool(enabled)


def get_iv2_kernels() -> bool:
    return _iv2_kernels


def require_attn_head_dim(hd: int):
    """the refusal of _attn_fwd_core, for callers that must give it before any other work (an InternVideo2 block: before its first norm)"""
    if hd not in (64, 80):
        raise TadError(f"attention: head_dim {hd} has no kernel (64 and 80 do)")


_q_cols = {}  # (A, factor, device) -> f32 [3A]: the factor on the q third, ones elsewhere (the cast of an un-normalised qkv, IV2AttentionFn)


def _q_scale_column(A: int, s: float, device):
    key = (A, float(s), str(device))
    col = _q_cols.get(key)
    if col is None:
        col = torch.ones(3 * A, dtype=torch.float32, device=device)
        col[:A] = s
        _q_cols[key] = col
    return col


def _iv2_no_precise(what: str):
    if _PRECISION == "precise":
        raise TadError(f'{what}: precision "precise" has no route for the InternVideo2 family (use "fast" or "half")')


def _op16_rows(x):
    """x [..., C] as 16-bit operand rows [M, C]: as it is when it already has the operand format, else cast from f32"""
    if x.dtype == K.operand_dtype():
        x = x.detach().reshape(-1, x.shape[-1])
        return x if x.is_contiguous() else x.contiguous()
    return K.cast_bf16(_f32c(x).reshape(-1, x.shape[-1]))


def _rms_torch_fwd(x, g, eps):
    rr = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    return x * rr * g, rr


def _rms_torch_bwd(dy, x, g, rr):
    xh, t = x * rr, dy * g
    return rr * (t - xh * (t * xh).mean(-1, keepdim=True)), (dy * xh).sum(0)


class RMSNormFn(_Fn):
    """RMSNorm.forward (internvideo2.py:119-130) on f32 rows: weight * x * rsqrt(mean(x^2) + eps).  out16: the result is the 16-bit
    operand of the Linear behind it (and the gradient arrives in that format), else f32."""

    @staticmethod
    def forward(ctx, x, weight, eps, out16=False):
        _need_gpu(x, "RMSNorm")
        _iv2_no_precise("RMSNorm")
        xc, w = _f32c(x), _f32c(weight)
        D = xc.shape[-1]
        x2 = xc.reshape(-1, D)
        train = _differentiated(ctx)
        ctx.kernels = _iv2_kernels
        out_dtype = K.operand_dtype() if out16 else torch.float32
        if ctx.kernels:
            y, rr = K.rmsnorm_fwd(x2, w, eps, out_dtype=out_dtype, save_stats=train)
        else:
            y, rr = _rms_torch_fwd(x2, w, eps)
            y = y.to(out_dtype)
        ctx.need = _needs(ctx, 2)
        ctx.weight = weight
        if train:
            ctx.save_for_backward(x2, w, rr)
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, w, rr = ctx.saved_tensors
        D = x2.shape[-1]
        dy2 = dy.detach().reshape(-1, D)
        dy2 = dy2 if dy2.is_contiguous() else dy2.contiguous()
        if not ctx.kernels:
            dx, dg = _rms_torch_bwd(dy2.float(), x2, w, rr)
            return dx.reshape(dy.shape), (dg if ctx.need[1] else None), None, None
        ent = _sink(ctx.weight) if ctx.need[1] else None
        dx, _, dg = K.rmsnorm_bwd(dy2, x2, w, rr, into=None if ent is None else ent[1])
        if ent is not None:
            if ent[2] is not None:
                ent[2](ctx.weight)
            dg = None
        return dx.reshape(dy.shape), (dg if ctx.need[1] else None), None, None


class IV2AttentionFn(_Fn):
    """Attention.forward of InternVideo2 (internvideo2.py:151-219): the qkv Linear (one bias [3A] or none) to f32, RMS normalisation of q
    and k over the full H*d width (gq / gk; None: qk_normalization off), space-time attention, proj.  The softmax scale's q contract
    (get_attn_q_prescale) rides in the normalisation kernel: the norm comes after the Linear, so the Linear's epilogue cannot carry it.
    x: f32, or the 16-bit operand itself (then dx has that format too)."""

    @staticmethod
    def forward(ctx, x, qkv_w, qkv_b, gq, gk, proj_w, proj_b, H, scale, eps):
        _need_gpu(x, "Attention")
        _iv2_no_precise("Attention")
        B, N, C = x.shape
        hd = head_dim_of(qkv_w, H)
        require_attn_head_dim(hd)
        if (gq is None) != (gk is None):
            raise TadError("Attention: q_norm and k_norm come together")
        train = _differentiated(ctx)
        ctx.x16 = x.dtype == K.operand_dtype()
        ctx.kernels = _iv2_kernels
        ctx.qpre = _attn_q_prescale
        s = K.q_prescale_of(scale) if ctx.qpre else 1.0
        A = H * hd
        xb = _op16_rows(x)
        qkv32, _ = K.linear_fwd(xb, w_bf16(qkv_w, train), _f32c(qkv_b), out_dtype=torch.float32)
        rr = g0 = g1 = None
        if gq is None:
            # no normalisation: the cast to the operand format carries the q contract
            qkv = K.scale_cast_op16(qkv32, gamma=None if s == 1.0 else _q_scale_column(A, s, x.device))
            qkv32 = None
        else:
            g0, g1 = _f32c(gq), _f32c(gk)
            if ctx.kernels:
                qkv, rr = K.qk_rmsnorm_fwd(qkv32, g0, g1, eps, q_out_scale=s, save_stats=train)
            else:
                q, k, v = qkv32.split(A, dim=1)
                (qn, rq), (kn, rk) = _rms_torch_fwd(q, g0, eps), _rms_torch_fwd(k, g1, eps)
                qkv = torch.cat((qn * s, kn, v), dim=1).to(K.operand_dtype())
                rr = torch.cat((rq, rk), dim=1).contiguous()
        r = K.attn_fwd(qkv, B, N, H, scale, out_dtype=None, want_lse=train, want_lo=train and _attn_exact_delta, q_prescaled=ctx.qpre, d=hd)
        ao, lse, ao_lo = r[0], r[1], (r[2] if len(r) > 2 else None)
        y, _ = K.linear_fwd(ao, w_bf16(proj_w, train), _f32c(proj_b), out_dtype=torch.float32)
        ctx.need = _needs(ctx, 7)
        if train:
            ctx.save_for_backward(xb if ctx.need[1] else None, qkv32, qkv, ao, lse, ao_lo, rr, g0, g1, qkv_w, proj_w)
        ctx.meta = (B, N, H, hd, scale, s)
        ctx.params = (qkv_b, gq, gk, proj_b)
        return y.reshape(B, N, -1)

    @staticmethod
    def backward(ctx, dy):
        xb, qkv32, qkv, ao, lse, ao_lo, rr, g0, g1, qkv_w, proj_w = ctx.saved_tensors
        B, N, H, hd, scale, s = ctx.meta
        qkv_b, gq, gk, proj_b = ctx.params
        A = H * hd
        dyb = K.cast_bf16(_f32c(dy).reshape(B * N, -1))
        d_ao = K.linear_bwd_input(dyb, wT_bf16(proj_w, True))
        dWp, dbp = linear_dw(dyb, ao, proj_w, proj_b, need=ctx.need[5:7])
        # (the q slot is the gradient of the plain q under either contract: of the normalised q here, s not applied -- tad_mi355x_ext.h)
        dqkv = K.attn_bwd(qkv, ao, d_ao, lse, B, N, H, scale, out_lo=ao_lo, q_prescaled=ctx.qpre, d=hd)
        dgq = dgk = None
        if gq is not None:
            if ctx.kernels:
                dqkv, dgq, dgk = K.qk_rmsnorm_bwd(dqkv, qkv32, g0, g1, rr, q_out_scale=s)
            else:
                dq, dk, dv = dqkv.float().split(A, dim=1)
                q, k, _ = qkv32.split(A, dim=1)
                (dq, dgq), (dk, dgk) = _rms_torch_bwd(dq, q, g0, rr[:, 0:1]), _rms_torch_bwd(dk, k, g1, rr[:, 1:2])
                dqkv = torch.cat((dq, dk, dv), dim=1).to(dqkv.dtype)
            dgq, dgk = (dgq if ctx.need[3] else None), (dgk if ctx.need[4] else None)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = K.linear_bwd_input(dqkv, wT_bf16(qkv_w, True), out_dtype=None if ctx.x16 else torch.float32).reshape(B, N, -1)
        dWqkv, dbqkv = linear_dw(dqkv, xb, qkv_w, qkv_b, need=(ctx.need[1], ctx.need[2] and qkv_b is not None))
        return dx, dWqkv, dbqkv, dgq, dgk, dWp, dbp, None, None, None


# --------------------------------------------------------------------------- fused Block
class _ChainLink:
    """Hand-off between two consecutive fused Blocks, one object per Block forward.  Block i's backward starts by casting the incoming
    residual-stream gradient to bf16 scaled by ITS drop-path scale dp2 -- a pass over an f32 [M, D] tensor that block i+1's LayerNorm
    backward, which produces that very gradient, can emit on the side.

    Forward: ``block_apply`` creates the link of block i, stores it in block i's ctx and hangs it on block i's OUTPUT TENSOR OBJECT;
    block i+1 finds it on its input (``_tad_link``) and keeps it as ``ctx.prev_link``.  Anything in between that produces a new tensor
    (checkpointing, a hook, ``x + 0``) drops the attribute, so the next block simply has no predecessor.
    Backward: block i+1 deposits (bf16 copy, the f32 gradient tensor it returns, that tensor's version) in ITS prev_link -- the
    object only block i's ctx of the SAME forward holds; block i takes the copy only if the gradient autograd hands it is still that
    storage, shape and version.  A second consumer of block i's output makes autograd either allocate a new sum (pointer differs)
    or accumulate in place (version differs): both miss and fall back to the cast pass.  Nothing is keyed by raw pointers in a
    process-wide table, so a stale entry of an earlier iteration can never be picked up by a later one."""
    __slots__ = ("dp2", "deposit", "__weakref__")

    def __init__(self, dp2):
        self.dp2 = dp2
        self.deposit = None


class _ChainState:
    def __init__(self):
        self.enabled = True
        self.hits = 0      # hand-offs taken (tests)
        self.pending = 0   # deposits made and not yet consumed or dropped (tests: must be 0 after a backward pass)


_chain = _ChainState()


def reset_block_chain():
    """kept for API compatibility: the hand-off state lives in per-forward link objects and needs no reset"""


def set_block_chain(enabled: bool):
    """switch the Block-to-Block bf16 gradient hand-off off / on (results are bit-identical either way; for tests and timing)"""
    _chain.enabled = bool(enabled)


def block_apply(x, *args):
    """BlockFn.apply plus the chain bookkeeping on the input / output tensor objects"""
    prev = getattr(x, "_tad_link", None) if _chain.enabled else None
    dp2 = args[14]
    link = _ChainLink(None if dp2 is None else _f32c(dp2)) if (_chain.enabled and torch.is_grad_enabled()) else None
    out = BlockFn.apply(x, *args, prev, link)
    if link is not None and out.requires_grad:
        out._tad_link = link
    return out


class BlockFn(_Fn):
    """Block.forward without layer-scale (modeling_finetune.py:159-163):
         x = x + dp1 * attn(norm1(x));  x = x + dp2 * mlp(norm2(x))
    dp1/dp2 are optional per-sample drop-path scales [B] (mask / keep_prob) or None."""

    @staticmethod
    def forward(ctx, x, n1w, n1b, qkv_w, q_bias, v_bias, proj_w, proj_b, n2w, n2b, fc1_w, fc1_b, fc2_w, fc2_b, dp1, dp2, H, scale,
                eps, prev_link=None, link=None):
        train, x1, a = _block_fwd_to_fc1(ctx, x, n1w, n1b, qkv_w, q_bias, v_bias, proj_w, proj_b, n2w, n2b, fc1_w, fc1_b, fc2_w, fc2_b,
                                         dp1, dp2, H, scale, eps, prev_link, link)
        B, N, D = x.shape
        x2, _ = K.linear_fwd(a, w_bf16(fc2_w, train), _f32c(fc2_b), out_dtype=torch.float32, epilogue=EPI_BIAS_RESIDUAL, residual=x1,
                             rowscale=_f32c(dp2), rows_per_scale=N)
        return x2.reshape(B, N, D)

    @staticmethod
    def backward(ctx, g):
        st = ctx.saved_tensors
        h, a, fc2_w, dp2 = st[13], st[14], st[18], st[20]
        B, N, D = ctx.meta[:3]
        g = _f32c(g).reshape(B * N, D)
        # ---- MLP branch
        gb = None
        dep = ctx.link.deposit if ctx.link is not None else None
        if dep is not None:
            ctx.link.deposit = None
            _chain.pending -= 1
            cand, ref, ver = dep
            if ref.data_ptr() == g.data_ptr() and ref._version == ver and g._version == ver and cand.shape == g.shape:
                gb = cand
                _chain.hits += 1
        if gb is None:
            gb = K.cast_bf16(g) if dp2 is None else K.scale_cast_bf16(g, None, dp2, N)
        dh = K.linear_bwd_input(gb, wT_bf16(fc2_w, True), gelu_preact=h)
        dW2, db2 = linear_dw(gb, a, fc2_w, ctx.biases[2], need=ctx.need[12:14])
        return _block_bwd_from_dh(ctx, st, g, dh, dW2, db2)


def _block_fwd_to_fc1(ctx, x, n1w, n1b, qkv_w, q_bias, v_bias, proj_w, proj_b, n2w, n2b, fc1_w, fc1_b, fc2_w, fc2_b, dp1, dp2, H, scale,
                      eps, prev_link, link):
    """the fused Block up to and including fc1 (+ GELU), and everything its backward needs; returns (train, x1 [M,D] f32, a [M,4D])"""
    _need_gpu(x, "Block")
    B, N, D = x.shape
    M = B * N
    train = _differentiated(ctx)
    x0 = _f32c(x).reshape(M, D)
    g1, b1, g2, b2 = _f32c(n1w), _f32c(n1b), _f32c(n2w), _f32c(n2b)
    xn1, mean1, rstd1 = K.layernorm_fwd(x0, g1, b1, eps, save_stats=train)
    qkv, ao, (lse, ao_lo) = _attn_fwd_core(xn1, qkv_w, q_bias, v_bias, B, N, H, scale, train, rowscale=_f32c(dp1))
    ctx.qpre = _attn_q_prescale  # (the contract `qkv` was written under: read back by the backward)
    x1, _ = K.linear_fwd(ao, w_bf16(proj_w, train), _f32c(proj_b), out_dtype=torch.float32, epilogue=EPI_BIAS_RESIDUAL, residual=x0,
                         rowscale=_f32c(dp1), rows_per_scale=N)
    xn2, mean2, rstd2 = K.layernorm_fwd(x1, g2, b2, eps, save_stats=train)
    a, h = K.linear_fwd(xn2, w_bf16(fc1_w, train), _f32c(fc1_b), out_dtype=None, epilogue=EPI_BIAS_GELU, want_preact=train)
    # inputs 0..13 = x and the thirteen parameters: a frozen Linear weight takes the one operand only ITS gradient reads out of the list
    need = ctx.need = _needs(ctx, 14)
    if train:
        ctx.save_for_backward(x0, g1, mean1, rstd1, xn1 if need[3] else None, qkv, ao, lse, x1, g2, mean2, rstd2, xn2 if need[10] else None,
                              h, a if need[12] else None, qkv_w, proj_w, fc1_w, fc2_w,
                              dp1 if dp1 is None else _f32c(dp1), dp2 if dp2 is None else _f32c(dp2), ao_lo)
    ctx.meta = (B, N, D, H, scale, q_bias is not None)
    ctx.biases = (proj_b, fc1_b, fc2_b)
    ctx.norms = (n1w, n1b, n2w, n2b)
    ctx.qv = (q_bias, v_bias)
    # block chain (_ChainLink): where my backward deposits the bf16 gradient for the block before me / takes the one made for me
    ctx.prev_link = prev_link if train else None
    ctx.link = link if train else None
    return train, x1, a


def _block_bwd_from_dh(ctx, st, g, dh, dW2, db2):
    """the fused Block's backward from the gradient dh of the MLP's hidden layer on: fc1, LN2, the attention branch, LN1 and the deposit
    for the block before.  g [M,D] f32: the gradient of the block's output rows (LN2's residual term)."""
    x0, g1, mean1, rstd1, xn1, qkv, ao, lse, x1, g2, mean2, rstd2, xn2, h, a, qkv_w, proj_w, fc1_w, fc2_w, dp1, dp2, ao_lo = st
    proj_b, fc1_b, fc2_b = ctx.biases
    B, N, D, H, scale, has_qb = ctx.meta
    dxn2 = K.linear_bwd_input(dh, wT_bf16(fc1_w, True))
    need = ctx.need
    dW1, db1 = linear_dw(dh, xn2, fc1_w, fc1_b, need=need[10:12])
    # LN2 backward also emits what the attention branch needs: bf16(drop-path scale * residual-stream grad) and its column
    # sums (= proj bias gradient), so neither a cast pass nor a bias reduction in the dW GEMM is needed
    n1w, n1b, n2w, n2b = ctx.norms
    gmid, gpb, dg2, dbeta2, dbp = layernorm_bwd_sunk(dxn2, x1, g2, mean2, rstd2, n2w, n2b, colsum_param=proj_b if need[7] else None, dres=g,
                                                    want_bf16=True, rowscale=dp1, rows_per_scale=N)
    # ---- attention branch
    d_ao = K.linear_bwd_input(gpb, wT_bf16(proj_w, True))
    # (the proj weight gradient rides with the qkv one: one launch for both, _attn_bwd_core)
    dxn1, dWqkv, dqb, dvb, dWp = _attn_bwd_core(d_ao, xn1, qkv, ao, lse, qkv_w, has_qb, B, N, H, scale, None, ctx.qv, ao_lo=ao_lo, q_prescaled=ctx.qpre,
                                                 pair=(gpb, ao, proj_w), rowscale=dp1, need=need[3:6], pair_need=need[6])
    prev = ctx.prev_link
    if prev is not None:
        gin, ginb, dg1, dbeta1, _ = layernorm_bwd_sunk(dxn1, x0, g1, mean1, rstd1, n1w, n1b, dres=gmid, want_bf16=True, rowscale=prev.dp2,
                                                       rows_per_scale=N)
        if prev.deposit is None:
            _chain.pending += 1
        prev.deposit = (ginb, gin, gin._version)
    else:
        gin, _, dg1, dbeta1, _ = layernorm_bwd_sunk(dxn1, x0, g1, mean1, rstd1, n1w, n1b, dres=gmid)
    return (gin.reshape(B, N, D), dg1, dbeta1, dWqkv, dqb, dvb, dWp, dbp, dg2, dbeta2, dW1, db1, dW2, db2, None, None, None, None,
            None, None, None)


# --------------------------------------------------------------------------- fused Block variants: layer-scale, proj / MLP dropout
# Block.forward with gamma_1 / gamma_2 (init_values > 0) and / or proj_drop / Mlp.drop active (drop_rate > 0, training)
# (modeling_finetune.py:159-166).  Each residual branch is  y = res + s[b] gamma[c] keep[m,c] / (1 - p) u,  u = a W^T + bias:
#   forward   without dropout the residual epilogue of the GEMM takes gamma (TAD_EPI_BIAS_RESIDUAL); with dropout the GEMM writes u in
#             f32 and K.branch_dropout_fwd combines -- the mask is the counter-based hash of attention dropout over (row, column, seed);
#   backward  gb = op16(s keep / (1 - p) g) carries NO gamma: d a = gb (diag(gamma) W) (K.rowscale_transpose_cast writes the operand),
#             T = gb^T a and cs = colsum(gb) from one K.linear_bwd_weight, and K.layerscale_grads turns them into
#             dW = gamma T, dbias = gamma cs, dgamma[n] = <T[n,:], W[n,:]> + bias[n] cs[n] -- u is neither stored nor recomputed.
# Not here: attention dropout in training, the pooled tail and the block-chain hand-off, the precise mode.
_block_variants = True
block_variant_calls = 0  # forwards taken through BlockVariantFn (tests)


def set_block_variants(enabled: bool):
    """layer-scale / proj-MLP-dropout Blocks through BlockVariantFn (default) or, off, composed from the per-operator Functions"""
    global _block_variants
    _block_variants = bool(enabled)


def get_block_variants() -> bool:
    return _block_variants


def block_variant_apply(x, *args):
    global block_variant_calls
    block_variant_calls += 1
    return BlockVariantFn.apply(x, *args)


def _branch_fwd(a, w, b, res, gamma, dp, N, train, p, seed):
    """res + dp gamma dropout(a w^T + b) -> f32 [M,D]"""
    if p > 0.0:
        u, _ = K.linear_fwd(a, w_bf16(w, train), _f32c(b), out_dtype=torch.float32)
        return K.branch_dropout_fwd(u, res, gamma, dp, N, p, seed)
    y, _ = K.linear_fwd(a, w_bf16(w, train), _f32c(b), out_dtype=torch.float32, epilogue=EPI_BIAS_RESIDUAL, residual=res, gamma=gamma,
                        rowscale=dp, rows_per_scale=N)
    return y


def _branch_wT(w, gamma):
    """the [K,N] operand of the branch's input gradient: W^T, with gamma folded in for a layer-scaled branch"""
    return wT_bf16(w, True) if gamma is None else K.rowscale_transpose_cast(_w2d(w), gamma)


def _branch_dw(gb, a, w, b, gamma_p, gamma, need=(True, True, True)):
    """(dW, db, dgamma) of a branch's Linear and layer-scale from gb (16-bit, scaled and masked, without gamma) and the Linear's input a;
    None for what went into gradient sinks.  need = (weight, bias, gamma): with none of the three wanted nothing is launched (``a`` may
    be None without the weight's and gamma's); a frozen one beside a trainable one is computed with it and dropped, except that a bias
    alone is gamma times the column sums."""
    if gamma_p is None:
        return linear_dw(gb, a, w, b, need=need[:2]) + (None,)
    need_b = need[1] and b is not None
    if not (need[0] or need[2]):
        return None, (gamma * K.colsum_bf16(gb) if need_b else None), None
    if not (need[0] and need[2] and (need_b or b is None)):
        # mixed flags inside one layer-scaled branch: T = gb^T a serves dW and dgamma alike, so the launches are those of the
        # all-trainable case (a frozen member has no gradient sink, hence the tensors come back and autograd keeps the wanted ones)
        T, cs = K.linear_bwd_weight(gb, a, want_bias=b is not None)
        dW, db, dg = K.layerscale_grads(T, _w2d(w), _f32c(b), cs, gamma)
        return (dW.reshape(w.shape) if need[0] else None), (db if need_b else None), (dg if need[2] else None)
    T, cs = K.linear_bwd_weight(gb, a, want_bias=b is not None)
    prms = (w, gamma_p) + ((b,) if b is not None else ())
    ents = [_sink(q) for q in prms]
    if all(e is not None for e in ents):
        K.layerscale_grads(T, _w2d(w), _f32c(b), cs, gamma, dW=ents[0][1].view(w.shape[0], -1), dgamma=ents[1][1],
                           dbias=ents[2][1] if b is not None else None, accumulate=True)
        for ent, prm in zip(ents, prms):
            if ent[2] is not None:
                ent[2](prm)
        return None, None, None
    dW, db, dg = K.layerscale_grads(T, _w2d(w), _f32c(b), cs, gamma)
    return dW.reshape(w.shape), db, dg


class BlockVariantFn(_Fn):
    """Block.forward with layer-scale and / or proj / MLP dropout (modeling_finetune.py:153-166):
         x = x + dp1 * gamma_1 * proj_drop(attn(norm1(x)));  x = x + dp2 * gamma_2 * mlp_drop(mlp(norm2(x)))
    gamma_1 / gamma_2: [D] or None; drop_p in [0, 1) with one mask seed per branch; dp1 / dp2 as in BlockFn."""

    @staticmethod
    def forward(ctx, x, n1w, n1b, qkv_w, q_bias, v_bias, proj_w, proj_b, n2w, n2b, fc1_w, fc1_b, fc2_w, fc2_b, gamma_1, gamma_2, drop_p,
                seed_attn, seed_mlp, dp1, dp2, H, scale, eps):
        _need_gpu(x, "Block")
        B, N, D = x.shape
        M = B * N
        train = _differentiated(ctx)
        p = float(drop_p)
        x0 = _f32c(x).reshape(M, D)
        g1, b1, g2, b2 = _f32c(n1w), _f32c(n1b), _f32c(n2w), _f32c(n2b)
        gm1, gm2, s1, s2 = _f32c(gamma_1), _f32c(gamma_2), _f32c(dp1), _f32c(dp2)
        xn1, mean1, rstd1 = K.layernorm_fwd(x0, g1, b1, eps, save_stats=train)
        qkv, ao, (lse, ao_lo) = _attn_fwd_core(xn1, qkv_w, q_bias, v_bias, B, N, H, scale, train, rowscale=s1)
        ctx.qpre = _attn_q_prescale
        x1 = _branch_fwd(ao, proj_w, proj_b, x0, gm1, s1, N, train, p, int(seed_attn))
        xn2, mean2, rstd2 = K.layernorm_fwd(x1, g2, b2, eps, save_stats=train)
        a, h = K.linear_fwd(xn2, w_bf16(fc1_w, train), _f32c(fc1_b), out_dtype=None, epilogue=EPI_BIAS_GELU, want_preact=train)
        x2 = _branch_fwd(a, fc2_w, fc2_b, x1, gm2, s2, N, train, p, int(seed_mlp))
        # inputs 0..15 = x, the thirteen parameters of BlockFn, gamma_1, gamma_2; `a` also serves dgamma_2 (see _branch_dw)
        need = ctx.need = _needs(ctx, 16)
        if train:
            ctx.save_for_backward(x0, g1, mean1, rstd1, xn1 if need[3] else None, qkv, ao, lse, x1, g2, mean2, rstd2,
                                  xn2 if need[10] else None, h, a if need[12] or (gamma_2 is not None and need[15]) else None,
                                  qkv_w, proj_w, fc1_w, fc2_w, s1, s2, ao_lo, gm1, gm2)
        ctx.meta = (B, N, D, H, scale, q_bias is not None, p, int(seed_attn), int(seed_mlp))
        ctx.biases = (proj_b, fc1_b, fc2_b)
        ctx.norms = (n1w, n1b, n2w, n2b)
        ctx.qv = (q_bias, v_bias)
        ctx.gammas = (gamma_1, gamma_2)
        return x2.reshape(B, N, D)

    @staticmethod
    def backward(ctx, g):
        (x0, g1, mean1, rstd1, xn1, qkv, ao, lse, x1, g2, mean2, rstd2, xn2, h, a, qkv_w, proj_w, fc1_w, fc2_w, dp1, dp2, ao_lo, gm1,
         gm2) = ctx.saved_tensors
        B, N, D, H, scale, has_qb, p, seed_attn, seed_mlp = ctx.meta
        proj_b, fc1_b, fc2_b = ctx.biases
        n1w, n1b, n2w, n2b = ctx.norms
        gamma_1, gamma_2 = ctx.gammas
        g = _f32c(g).reshape(B * N, D)
        need = ctx.need
        # ---- MLP branch
        if p > 0.0:
            gb = K.branch_dropout_cast(g, dp2, N, p, seed_mlp)
        else:
            gb = K.cast_bf16(g) if dp2 is None else K.scale_cast_bf16(g, None, dp2, N)
        dh = K.linear_bwd_input(gb, _branch_wT(fc2_w, gm2), gelu_preact=h)
        dW2, db2, dgm2 = _branch_dw(gb, a, fc2_w, fc2_b, gamma_2, gm2, need=(need[12], need[13], need[15]))
        dxn2 = K.linear_bwd_input(dh, wT_bf16(fc1_w, True))
        dW1, db1 = linear_dw(dh, xn2, fc1_w, fc1_b, need=need[10:12])
        # LN2 backward emits op16(dp1 * residual-stream gradient) on the side; under dropout the masked copy needs a pass of its own
        gmid, gpb, dg2, dbeta2, _ = layernorm_bwd_sunk(dxn2, x1, g2, mean2, rstd2, n2w, n2b, dres=g, want_bf16=p == 0.0, rowscale=dp1,
                                                     rows_per_scale=N)
        if p > 0.0:
            gpb = K.branch_dropout_cast(gmid, dp1, N, p, seed_attn)
        # ---- attention branch
        d_ao = K.linear_bwd_input(gpb, _branch_wT(proj_w, gm1))
        dWp, dbp, dgm1 = _branch_dw(gpb, ao, proj_w, proj_b, gamma_1, gm1, need=(need[6], need[7], need[14]))
        dxn1, dWqkv, dqb, dvb = _attn_bwd_core(d_ao, xn1, qkv, ao, lse, qkv_w, has_qb, B, N, H, scale, None, ctx.qv, ao_lo=ao_lo,
                                               q_prescaled=ctx.qpre, rowscale=dp1, need=need[3:6])
        gin, _, dg1, dbeta1, _ = layernorm_bwd_sunk(dxn1, x0, g1, mean1, rstd1, n1w, n1b, dres=gmid)
        return (gin.reshape(B, N, D), dg1, dbeta1, dWqkv, dqb, dvb, dWp, dbp, dg2, dbeta2, dW1, db1, dW2, db2, dgm1, dgm2, None, None,
                None, None, None, None, None, None)


# --------------------------------------------------------------------------- last Block + mean-pool
# The fine-tuning model ends with fc_norm(mean over tokens(last block's output)).  x2 = x1 + dp2 (a W2^T + b2) is linear in a and
# nothing but the token mean reads it, so
#   forward:  mean_n(x2)[b] = mean_n(x1)[b] + dp2[b] ((S[b] / N) W2^T + b2),  S[b] = sum_n a[b,n,:]     -- no fc2 GEMM, no x2;
#   backward: every token of clip b receives dy[b] / N, so the fc2 input-gradient rows of a clip share ONE accumulator row
#             t[b] = gb[b] W2 (gb[b] = op16(dy[b] / N * dp2[b])) and dh = op16(t[clip] * gelu'(h)) is one streaming pass;
#             dW2 = sum_b gb[b]^T S[b], db2 = N sum_b gb[b].
# dh -- and with it everything upstream of the MLP's hidden layer -- is bit-identical to BlockFn + MeanPoolFn (t[b] is the row the
# B*N-row launch computes N times: every plan of gemm_nt sums K in the same order); the pooled output, dW2 and db2 are the same products
# summed in another order (S is never rounded to 16 bits; dW2 / db2 in f32, the B x D pooled fc2 with f64 accumulation: K.pooled_linear).
_pooled_tail = None


def set_pooled_tail(enabled: bool):
    """switch the last-block + mean-pool shortcut off / on (default on; TAD_POOLED_TAIL=0 in the environment, read once, turns it off)"""
    global _pooled_tail
    _pooled_tail = bool(enabled)


def get_pooled_tail() -> bool:
    global _pooled_tail
    if _pooled_tail is None:
        import os
        v = os.environ.get("TAD_POOLED_TAIL", "1").strip()
        _pooled_tail = not (v.isdigit() and int(v) == 0)
    return _pooled_tail


def pooled_tail_ok(fc2_w) -> bool:
    """the switch is on, the precision mode has 16-bit operands, and the shapes are ones the pooled-tail kernels take"""
    return get_pooled_tail() and _PRECISION in ("fast", "half") and K.colsum_segments_ok(fc2_w.shape[1])


class _PoolStats:
    calls = 0  # forwards taken through BlockPoolFn (tests)


def block_pool_apply(x, *args):
    """BlockPoolFn.apply plus the chain bookkeeping on the input tensor object (the pooled output has no successor block)"""
    prev = getattr(x, "_tad_link", None) if _chain.enabled else None
    _PoolStats.calls += 1
    return BlockPoolFn.apply(x, *args, prev, None)


class BlockPoolFn(_Fn):
    """mean over tokens of BlockFn's output: [B, N, D] -> [B, D] f32 (see above)."""

    @staticmethod
    def forward(ctx, x, n1w, n1b, qkv_w, q_bias, v_bias, proj_w, proj_b, n2w, n2b, fc1_w, fc1_b, fc2_w, fc2_b, dp1, dp2, H, scale,
                eps, prev_link=None, link=None):
        train, x1, a = _block_fwd_to_fc1(ctx, x, n1w, n1b, qkv_w, q_bias, v_bias, proj_w, proj_b, n2w, n2b, fc1_w, fc1_b, fc2_w, fc2_b,
                                         dp1, dp2, H, scale, eps, prev_link, link)
        B, N, D = x.shape
        S = K.colsum_segments(a, B, N)
        xbar = K.meanpool_fwd(x1.view(B, N, D))
        ctx.pool_S = S if train and ctx.need[12] else None
        # xbar + dp2 ((S / N) W2^T + b2) on the VALUES of the 16-bit operand copy of W2: the pooled operand is never rounded to 16 bits
        return K.pooled_linear(S, w_bf16(fc2_w, train), _f32c(fc2_b), _f32c(dp2), xbar, N)

    @staticmethod
    def backward(ctx, dy):
        st = ctx.saved_tensors
        h, fc2_w, dp2 = st[13], st[18], st[20]
        S = ctx.pool_S
        B, N, D = ctx.meta[:3]
        fc2_b = ctx.biases[2]
        # the gradient of every output row: dy[b] / N, materialised for LN2's residual term by the kernel MeanPoolFn's backward runs;
        # gb[b] = op16(dy[b] / N * dp2[b]) through the kernels BlockFn's backward casts it with: a row of its operand bit for bit
        g, _ = K.meanpool_bwd(_f32c(dy), N)
        g_rows = g[:, 0, :].contiguous()
        gb = K.cast_bf16(g_rows) if dp2 is None else K.scale_cast_bf16(g_rows, None, dp2, 1)
        t = K.linear_bwd_input(gb, wT_bf16(fc2_w, True), out_dtype=torch.float32)
        dh = K.gelu_grad_bcast(t, h, N)
        # dW2 = gb^T S, db2 = N sum_b gb[b]: f32 products of the 16-bit gb values and the f32 sums, into the gradient sinks as linear_dw does
        need_w, need_b = ctx.need[12], ctx.need[13] and fc2_b is not None
        if not need_w:  # a frozen fc2: S was not kept; a trainable bias beside it still gets its N sum_b gb[b]
            return _block_bwd_from_dh(ctx, st, g.view(B * N, D), dh, None, gb.float().sum(0) * float(N) if need_b else None)
        if not need_b:
            fc2_b = None
        gbf = gb.float()
        sw = _sink(fc2_w)
        sb = _sink(fc2_b) if fc2_b is not None else None
        if sw is not None and (fc2_b is None or sb is not None):
            sw[1].view(fc2_w.shape[0], -1).addmm_(gbf.t(), S)
            if sb is not None:
                sb[1].add_(gbf.sum(0), alpha=float(N))
            for ent, prm in ((sw, fc2_w), (sb, fc2_b)):
                if ent is not None and ent[2] is not None:
                    ent[2](prm)
            dW2, db2 = None, None
        else:
            dW2 = torch.matmul(gbf.t(), S)
            db2 = gbf.sum(0) * float(N) if fc2_b is not None else None
        return _block_bwd_from_dh(ctx, st, g.view(B * N, D), dh, dW2, db2)


# --------------------------------------------------------------------------- plain Linear (f32 rows in / out)
class LinearFn(_Fn):
    """nn.Linear on f32 rows through the 16-bit MFMA GEMM (encoder_to_decoder and the decoder head, modeling_pretrain.py:163,269);
    in the precise mode through the split-bf16 GEMMs."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _need_gpu(x, "Linear")
        shp = x.shape
        train = _differentiated(ctx)
        ctx.params = (weight, bias)
        ctx.shp = shp
        ctx.precise = _PRECISION == "precise"
        if ctx.precise:  # split-bf16 operands on f32 rows, like every other Linear of the parity gate (PreciseBlockFn)
            x2 = _f32c(x).reshape(-1, shp[-1])
            y = precise_linear(x2, weight, bias, fresh=train)
            if train:
                ctx.save_for_backward(x2)
            return y.reshape(*shp[:-1], -1)
        xb = K.cast_bf16(_f32c(x).reshape(-1, shp[-1]))
        y, _ = K.linear_fwd(xb, w_bf16(weight, train), _f32c(bias), out_dtype=torch.float32)
        ctx.need = _needs(ctx, 3)
        if train:
            ctx.save_for_backward(xb if ctx.need[1] else None)
        return y.reshape(*shp[:-1], -1)

    @staticmethod
    def backward(ctx, dy):
        (xb,) = ctx.saved_tensors
        weight, bias = ctx.params
        if ctx.precise:
            dy2 = _f32c(dy).reshape(-1, dy.shape[-1])
            dx = precise_dx(dy2, weight) if ctx.needs_input_grad[0] else None
            dW, db = precise_dw(dy2, xb, want_bias=bias is not None)
            return (None if dx is None else dx.reshape(ctx.shp)), dW, db
        dyb = K.cast_bf16(_f32c(dy).reshape(-1, dy.shape[-1]))
        dx = K.linear_bwd_input(dyb, wT_bf16(weight, True), out_dtype=torch.float32) if ctx.needs_input_grad[0] else None
        dW, db = linear_dw(dyb, xb, weight, bias, need=ctx.need[1:3])
        return (None if dx is None else dx.reshape(ctx.shp)), dW, db


class LinearSplitFn(_Fn):
    """nn.Linear on f32 rows through the split-operand GEMMs (hi + lo, three MFMA products: f32-level accuracy) in EVERY precision mode:
    LinearFn's precise branch as a function of its own.  For the few Linears whose rounding reaches the logits directly -- the
    attention-pooling head of the InternVideo2 family, where 16-bit operands cost more accuracy than the whole encoder in front of them
     and the split costs two D x D GEMMs per step."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _need_gpu(x, "Linear")
        ctx.params = (weight, bias)
        ctx.shp = x.shape
        train = _differentiated(ctx)
        x2 = _f32c(x).reshape(-1, x.shape[-1])
        y = precise_linear(x2, weight, bias, fresh=train)
        ctx.need = _needs(ctx, 3)
        if train:
            ctx.save_for_backward(x2 if ctx.need[1] else None)
        return y.reshape(*x.shape[:-1], -1)

    @staticmethod
    def backward(ctx, dy):
        (x2,) = ctx.saved_tensors
        weight, bias = ctx.params
        dy2 = _f32c(dy).reshape(-1, dy.shape[-1])
        dx = precise_dx(dy2, weight).reshape(ctx.shp) if ctx.needs_input_grad[0] else None
        dW = precise_dw(dy2, x2, want_bias=False)[0] if ctx.need[1] else None
        db = K.colsum_f32(dy2) if (bias is not None and ctx.need[2]) else None
        return dx, dW, db


# --------------------------------------------------------------------------- MAE pre-training path
class GatherRowsFn(_Fn):
    """x[~mask].reshape(B, -1, C) (modeling_pretrain.py:98) with precomputed row indices (b*N + visible token)."""

    @staticmethod
    def forward(ctx, x, idx, B):
        _need_gpu(x, "token gather")
        Bx, N, D = x.shape
        ctx.save_for_backward(idx)
        ctx.shape = (Bx, N, D)
        return K.gather_rows(_f32c(x).reshape(Bx * N, D), idx).reshape(B, -1, D)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        Bx, N, D = ctx.shape
        return K.scatter_rows(_f32c(g).reshape(-1, D), idx, Bx * N).reshape(Bx, N, D), None, None


class MaeAssembleFn(_Fn):
    """cat([x_vis + pos[vis], mask_token + pos[masked]], dim=1) (modeling_pretrain.py:283-287); the positional table is a constant"""

    @staticmethod
    def forward(ctx, x_vis, mask_token, pos, vis_idx, mask_idx):
        _need_gpu(x_vis, "MAE decoder input")
        B, Nv, D = x_vis.shape
        ctx.meta = (B, Nv, mask_idx.numel() // B, D)
        return K.mae_assemble(_f32c(x_vis).reshape(B * Nv, D), _f32c(mask_token).reshape(-1), _f32c(pos).reshape(-1, D), vis_idx, mask_idx, B)

    @staticmethod
    def backward(ctx, g):
        B, Nv, Nm, D = ctx.meta
        g = _f32c(g)
        d_xv = g[:, :Nv].contiguous()
        d_tok = K.colsum_window_f32(g, Nv, Nm).reshape(1, 1, D)  # (the f64 verification kernel on a contiguous copy took 2.3 ms here)
        return d_xv, d_tok, None, None, None


# The entry of the InternVideo2 MAE encoder (internvideo2_pretrain_videomae.py:184-205): a TRAINABLE position table is added, then the
# visible tokens are kept.  Kernels: csrc/visible_tokens.hip through the pre-training ABI (include/tad_mi355x_pretrain.h).
_visible_token_kernels = True


def set_visible_token_kernels(enabled: bool):
    """A/B switch: VisibleTokensFn through its HIP kernels (default) or, off, through the torch expressions of the same arithmetic
    (``x + pos`` over every token, then the index; backward: the index_put into zeros and the dense sum over the batch that autograd
    would run).  Forward and dx are the same bits either way; the table gradient is summed in torch's order when off.  Sampled by each
    forward; a node's backward follows its own forward."""
    global _visible_token_kernels
    _visible_token_kernels = bool(enabled)


def get_visible_token_kernels() -> bool:
    return _visible_token_kernels


class VisibleTokensFn(_Fn):
    """``(x + pos)[~mask].reshape(B, -1, C)`` with the visible tokens given as indices: x [B,N,D] f32, pos [1,N,D] or [N,D] (a Parameter
    or any tensor that may want a gradient), vis_tok [B,Nv] int32 (modeling_pretrain.token_indices) -> [B,Nv,D].  Only the visible rows of
    x are read.  Backward, one launch: dx [B,N,D] with every row written (requested only if x wants a gradient) and the table's
    gradient summed over the clips in the order b = 0, 1, ... (requested only if pos wants one; written straight into pos' gradient
    sink where it has one)."""

    @staticmethod
    def forward(ctx, x, pos, vis_tok):
        _need_gpu(x, "visible tokens")
        xc, pc = _f32c(x), _f32c(pos)
        B, N, D = xc.shape
        if pc.numel() != N * D or vis_tok.dim() != 2 or vis_tok.shape[0] != B:
            raise TadError(f"visible tokens: x {tuple(x.shape)}, pos {tuple(pos.shape)} and vis_tok {tuple(vis_tok.shape)} do not belong together")
        pc = pc.reshape(N, D)
        tok = vis_tok.detach()
        tok = tok if tok.dtype == torch.int32 else tok.to(torch.int32)
        tok = tok if tok.is_contiguous() else tok.contiguous()
        ctx.kernels = _visible_token_kernels
        ctx.need = _needs(ctx, 2)
        ctx.pos = pos
        ctx.meta = (B, N, D)
        if ctx.kernels:
            out = K.visible_tokens_fwd(xc, pc, tok)
            if _differentiated(ctx):
                # slot[b, n]: where token n stands among clip b's visible tokens, -1 if it is masked; built on the device, no sync
                slot = torch.full((B, N), -1, dtype=torch.int32, device=xc.device)
                slot.scatter_(1, tok.long(), torch.arange(tok.shape[1], dtype=torch.int32, device=xc.device).expand(B, -1))
                ctx.save_for_backward(slot)
        else:
            out = (xc + pc)[torch.arange(B, device=xc.device).unsqueeze(1), tok.long()]
            if _differentiated(ctx):
                ctx.save_for_backward(tok)
        return out

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        B, N, D = ctx.meta
        gc = _f32c(g)
        need_x, need_pos = ctx.need
        if not ctx.kernels:
            full = torch.zeros((B, N, D), dtype=torch.float32, device=gc.device)
            full[torch.arange(B, device=gc.device).unsqueeze(1), idx.long()] = gc
            return (full if need_x else None), (full.sum(0).reshape(ctx.pos.shape) if need_pos else None), None
        ent = _sink(ctx.pos) if need_pos else None
        dx, dpos = K.visible_tokens_bwd(gc, idx, want_dx=need_x, want_dpos=need_pos, into=None if ent is None else ent[1])
        if ent is not None:
            if ent[2] is not None:
                ent[2](ctx.pos)
            dpos = None
        return dx, (None if dpos is None else dpos.reshape(ctx.pos.shape)), None


# The entry of the InternVideo2 encoder and the evaluation tail of its half blocks (internvideo2.py): csrc/iv2_serve.hip through the
# serving ABI (include/tad_mi355x_serve.h, libtad_mi355x_serve.so).
_iv2_serve_kernels = True


def set_iv2_serve_kernels(enabled: bool):
    """A/B switch: ClassTokenEntryFn through its HIP kernels, and the InternVideo2 evaluation forward as one loop over fused
    residual + RMSNorm launches (default); or, off, the torch ``cat`` + add (autograd's dense sums on the way back) and the per-block
    module route.  Forward bits of the entry are the same either way; the table's and the class token's gradients are summed over the
    clips in the order b = 0, 1, ... when on and in torch's order when off.  Sampled by each forward; a node's backward follows its own
    forward."""
    global _iv2_serve_kernels
    _iv2_serve_kernels = bool(enabled)


def get_iv2_serve_kernels() -> bool:
    return _iv2_serve_kernels


class ClassTokenEntryFn(_Fn):
    """``cat((cls_token.expand(B, -1, -1), x), 1) + pos``: x [B,N,D] f32, cls_token [1,1,D], pos [1,N+1,D] (a Parameter, or the table
    composed of the sep_pos_embed parts: any tensor that may want a gradient) -> [B,N+1,D].  Backward, one launch: the patch rows'
    gradient (requested only if x wants one) and the sums over the clips in the order b = 0, 1, ... for pos and cls_token (each only if
    wanted; written straight into the gradient sinks where BOTH wanted ones have a sink, else returned as tensors)."""

    @staticmethod
    def forward(ctx, x, cls_token, pos):
        _need_gpu(x, "class token entry")
        xc, cc, pc = _f32c(x), _f32c(cls_token), _f32c(pos)
        B, N, D = xc.shape
        if cc.numel() != D or pc.numel() != (N + 1) * D:
            raise TadError(f"class token entry: x {tuple(x.shape)}, cls_token {tuple(cls_token.shape)} and pos {tuple(pos.shape)} do not belong together")
        ctx.kernels = _iv2_serve_kernels
        ctx.need = _needs(ctx, 3)
        ctx.params = (cls_token, pos)
        ctx.meta = (B, N, D)
        if ctx.kernels:
            return K.class_token_entry_fwd(xc, cc.reshape(D), pc.reshape(N + 1, D))
        return torch.cat((cc.reshape(1, 1, D).expand(B, -1, -1), xc), dim=1) + pc.reshape(1, N + 1, D)

    @staticmethod
    def backward(ctx, g):
        B, N, D = ctx.meta
        cls_token, pos = ctx.params
        gc = _f32c(g)
        need_x, need_cls, need_pos = ctx.need
        if not ctx.kernels:
            return ((gc[:, 1:].contiguous() if need_x else None), (gc[:, :1].sum(0, keepdim=True).reshape(cls_token.shape) if need_cls else None),
                    (gc.sum(0, keepdim=True).reshape(pos.shape) if need_pos else None))
        if not (need_x or need_cls or need_pos):
            return None, None, None
        ent_c, ent_p = (_sink(cls_token) if need_cls else None), (_sink(pos) if need_pos else None)
        if need_cls and need_pos and (ent_c is None) != (ent_p is None):
            ent_c = ent_p = None  # (one accumulate flag in the kernel: a lone sink gets its gradient from autograd)
        dx, dpos, dcls = K.class_token_entry_bwd(gc, want_dpatch=need_x, want_dpos=need_pos, want_dcls=need_cls,
                                                 into_pos=None if ent_p is None else ent_p[1], into_cls=None if ent_c is None else ent_c[1])
        for ent, p in ((ent_c, cls_token), (ent_p, pos)):
            if ent is not None and ent[2] is not None:
                ent[2](p)
        return (dx, (None if dcls is None or ent_c is not None else dcls.reshape(cls_token.shape)),
                (None if dpos is None or ent_p is not None else dpos.reshape(pos.shape)))


class MseLossFn(_Fn):
    """nn.MSELoss()(outputs, labels) (engine_for_pretraining.py:27,70): loss and d(loss)/d(outputs) in one pass"""

    @staticmethod
    def forward(ctx, pred, target):
        _need_gpu(pred, "MSE loss")
        loss, grad = K.mse_loss(_f32c(pred), _f32c(target), want_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(grad)
        ctx.shape = pred.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g).reshape(ctx.shape), None


# --------------------------------------------------------------------------- mean-pool
class MeanPoolFn(_Fn):
    """x.mean(1) over tokens (modeling_finetune.py:325-326)."""

    @staticmethod
    def forward(ctx, x):
        _need_gpu(x, "mean-pool")
        ctx.n = x.shape[1]
        return K.meanpool_fwd(_f32c(x))

    @staticmethod
    def backward(ctx, dy):
        dx, _ = K.meanpool_bwd(_f32c(dy), ctx.n)
        return dx


# --------------------------------------------------------------------------- precise mode: autograd
class PreciseBlockFn(_Fn):
    """Block forward/backward in the precise mode (f32 activations, split-bf16 Linears, f32 attention): the gradient side of the
    parity gate.  Same data flow as BlockFn; no drop-path (verification runs use drop_path_rate = 0)."""

    @staticmethod
    def forward(ctx, x, n1w, n1b, qkv_w, q_bias, v_bias, proj_w, proj_b, n2w, n2b, fc1_w, fc1_b, fc2_w, fc2_b, H, scale, eps):
        _need_gpu(x, "Block")
        B, N, D = x.shape
        M = B * N
        fr = _differentiated(ctx)  # differentiated forward: never reuse cached weight copies (see _cached)
        x0 = _f32c(x).reshape(M, D)
        g1, b1, g2, b2 = _f32c(n1w), _f32c(n1b), _f32c(n2w), _f32c(n2b)
        xn1, mean1, rstd1 = K.layernorm_fwd(x0, g1, b1, eps, out_dtype=torch.float32)
        qkv = precise_linear(xn1, qkv_w, _qkv_bias(q_bias, v_bias), fresh=fr)
        ao, lse = K.attn_fwd_f32(qkv, B, N, H, scale, want_lse=True, d=head_dim_of(qkv_w, H))
        x1 = precise_linear(ao, proj_w, proj_b, EPI_BIAS_RESIDUAL, residual=x0, fresh=fr)
        xn2, mean2, rstd2 = K.layernorm_fwd(x1, g2, b2, eps, out_dtype=torch.float32)
        h = precise_linear(xn2, fc1_w, fc1_b, fresh=fr)
        a = K.gelu_f32(h)
        x2 = precise_linear(a, fc2_w, fc2_b, EPI_BIAS_RESIDUAL, residual=x1, fresh=fr)
        ctx.save_for_backward(x0, g1, mean1, rstd1, xn1, qkv, ao, lse, x1, g2, mean2, rstd2, xn2, h, a, qkv_w, proj_w, fc1_w, fc2_w)
        ctx.meta = (B, N, D, H, scale, q_bias is not None)
        return x2.reshape(B, N, D)

    @staticmethod
    def backward(ctx, g):
        x0, g1, mean1, rstd1, xn1, qkv, ao, lse, x1, g2, mean2, rstd2, xn2, h, a, qkv_w, proj_w, fc1_w, fc2_w = ctx.saved_tensors
        B, N, D, H, scale, has_qb = ctx.meta
        g = _f32c(g).reshape(B * N, D)
        dh = K.gelu_bwd_f32(precise_dx(g, fc2_w), h)
        dW2, db2 = precise_dw(g, a)
        dxn2 = precise_dx(dh, fc1_w)
        dW1, db1 = precise_dw(dh, xn2)
        gmid, _, dg2, dbeta2, _ = K.layernorm_bwd(dxn2, x1, g2, mean2, rstd2, dres=g)
        d_ao = precise_dx(gmid, proj_w)
        dWp, dbp = precise_dw(gmid, ao)
        dqkv = K.attn_bwd_f32(qkv, ao, d_ao, lse, B, N, H, scale, d=head_dim_of(qkv_w, H))
        dxn1 = precise_dx(dqkv, qkv_w)
        dWqkv, dbqkv = precise_dw(dqkv, xn1, want_bias=has_qb)
        dqb = dvb = None
        if has_qb:
            AH = dbqkv.numel() // 3
            dqb, dvb = dbqkv[:AH].clone(), dbqkv[2 * AH:].clone()
        gin, _, dg1, dbeta1, _ = K.layernorm_bwd(dxn1, x0, g1, mean1, rstd1, dres=gmid)
        return (gin.reshape(B, N, D), dg1, dbeta1, dWqkv, dqb, dvb, dWp, dbp, dg2, dbeta2, dW1, db1, dW2, db2, None, None, None)


class PrecisePatchEmbedFn(_Fn):
    @staticmethod
    def forward(ctx, x, weight, bias, pos, tubelet, patch):
        _need_gpu(x, "PatchEmbed")
        B = x.shape[0]
        cols = K.im2col_tubelets_f32(_f32c(x), tubelet, patch)
        ntok = cols.shape[0] // B
        res = _f32c(pos).repeat(B, 1) if pos is not None else None
        kw = weight.numel() // weight.shape[0]
        ws = (_cached_split(weight, _differentiated(ctx)) if cols.shape[1] == kw
              else K.split_bf16x3(K.pad_k(_w2d(weight), cols.shape[1]).contiguous(), role_b=True))  # zero-padded K (patch 14)
        y, _ = K.linear_fwd(K.split_bf16x3(cols, role_b=False), ws, _f32c(bias),
                            out_dtype=torch.float32, epilogue=EPI_BIAS_RESIDUAL if res is not None else EPI_BIAS, residual=res)
        ctx.save_for_backward(cols)
        ctx.wshape = weight.shape
        ctx.has_bias = bias is not None
        return y.reshape(B, ntok, weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        (cols,) = ctx.saved_tensors
        dW, db = precise_dw(_f32c(dy).reshape(-1, dy.shape[-1]), cols, want_bias=ctx.has_bias)
        kw = 1
        for d in ctx.wshape[1:]:
            kw *= d
        return None, dW[:, :kw].reshape(ctx.wshape), db, None, None, None
