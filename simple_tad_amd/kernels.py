"""Tensor-level wrappers over the C ABI: validate shapes on the host, pass raw device
pointers + the current HIP stream.  No arithmetic happens in Python or in torch here.

Every function requires CUDA(=HIP) tensors and raises otherwise -- there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESIDUAL, TAD_BF16, TAD_F16, TAD_F32, check

_workspaces = {}


class LaunchProfiler:
    """Optional per-launch timing with HIP events on the launching stream (used by bench.py for the live roofline figure).
    ``record(kernel, flops, bytes)`` brackets one C-ABI call; ``summary()`` synchronises and aggregates per kernel class."""

    def __init__(self, only=None, stride=1):
        self.items = []
        self.only = set(only) if only else None  # restrict to these kernel classes (keeps the timed region undisturbed)
        # A timed HIP event pair costs ~20 us of queue time on this platform (measured: 192 pairs per step = +2 ms on a 55 ms
        # step), so the bench samples every ``stride``-th launch of a class; a stride coprime with the number of launches per
        # step visits every GEMM shape equally often.
        self.stride = max(1, int(stride))
        self.seen = {}

    def wants(self, kernel):
        if self.only is not None and kernel not in self.only:
            return False
        n = self.seen.get(kernel, 0)
        self.seen[kernel] = n + 1
        return n % self.stride == 0

    def begin(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record(torch.cuda.current_stream())
        return e

    def end(self, start, kernel, flops, nbytes, kernel_launches=1):
        e = torch.cuda.Event(enable_timing=True)
        e.record(torch.cuda.current_stream())
        self.items.append((kernel, start, e, flops, nbytes, kernel_launches))

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for kernel, s, e, flops, nbytes, nk in self.items:
            d = out.setdefault(kernel, {"launches": 0, "calls": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += nk
            d["calls"] += 1
            d["ms"] += s.elapsed_time(e)
            d["flops"] += flops
            d["bytes"] += nbytes
        return out


_prof = None


def set_profiler(p):
    global _prof
    _prof = p


class _timed:
    __slots__ = ("k", "f", "b", "s", "n0")

    def __init__(self, kernel, flops=0.0, nbytes=0.0):
        self.k, self.f, self.b = kernel, flops, nbytes

    def __enter__(self):
        self.s = _prof.begin() if (_prof is not None and _prof.wants(self.k)) else None
        if self.s is not None and self.k == "gemm_nt":
            self.n0 = _lib.load().tad_linear_kernel_launches()

    def __exit__(self, *a):
        if self.s is not None:
            # a Linear call is one gemm_nt kernel launch, or two under the split-tail plan: count kernels, not calls
            n = (_lib.load().tad_linear_kernel_launches() - self.n0) if self.k == "gemm_nt" else 1
            _prof.end(self.s, self.k, self.f, self.b, n)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _req(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise _lib.TadError(f"{name}: expected a GPU tensor (the MI355X path has no CPU fallback), got {t.device}")
    if t.dtype != dtype:
        raise _lib.TadError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.TadError(f"{name}: tensor must be contiguous")


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return TAD_F32
    if t.dtype == torch.bfloat16:
        return TAD_BF16
    if t.dtype == torch.float16:
        return TAD_F16
    raise _lib.TadError(f"unsupported dtype {t.dtype}")


# ----------------------------------------------------------------------------- 16-bit operand format
# Every kernel that touches GEMM / attention operands exists for bfloat16 (tad_*) and for IEEE half (tad_*_f16) -- the same
# kernels compiled for the other format (include/tad_mi355x.h).  A call's format is the dtype of its 16-bit tensors; functions that
# CREATE 16-bit tensors from f32 (casts, LayerNorm, im2col ...) take it from ``dtype=`` or, by default, from the process-wide operand
# format below (ops.set_precision selects it: "fast" -> bfloat16, "half" -> float16).
OP16_DTYPES = (torch.bfloat16, torch.float16)
_op16 = torch.bfloat16


def set_operand_dtype(dtype) -> None:
    global _op16
    if dtype not in OP16_DTYPES:
        raise ValueError(f"operand dtype must be torch.bfloat16 or torch.float16, got {dtype}")
    _op16 = dtype


def operand_dtype():
    return _op16


def _fn(name: str, dtype):
    """the entry point `name` for 16-bit operands of `dtype` (its _f16 twin for torch.float16)"""
    if dtype == torch.float16:
        name = _lib.F16_TWINS.get(name) or _lib.VARIANT_F16_TWINS[name]
    return getattr(_lib.load(), name)


def _req16(t: torch.Tensor, name: str, like=None):
    """a contiguous GPU tensor in one of the two 16-bit operand formats (the same one as ``like`` if given); returns its dtype"""
    if not t.is_cuda:
        raise _lib.TadError(f"{name}: expected a GPU tensor (the MI355X path has no CPU fallback), got {t.device}")
    if t.dtype not in OP16_DTYPES or (like is not None and t.dtype != like):
        raise _lib.TadError(f"{name}: expected {like if like is not None else 'bfloat16 or float16'}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.TadError(f"{name}: tensor must be contiguous")
    return t.dtype


def _out16(out_dtype, op):
    """output dtype of a call with 16-bit operands of format `op`: f32, or that same 16-bit format (None = the operands' own)"""
    if out_dtype is None or out_dtype in OP16_DTYPES:
        if out_dtype is not None and out_dtype != op:
            raise _lib.TadError(f"16-bit output {out_dtype} does not match the operands' format {op}")
        return op
    if out_dtype != torch.float32:
        raise _lib.TadError(f"unsupported output dtype {out_dtype}")
    return out_dtype


def _ws_key(device, stream=None):
    dev = device.index if device.index is not None else torch.cuda.current_device()
    return (dev, (torch.cuda.current_stream(device) if stream is None else stream).cuda_stream)


def workspace(nbytes: int, device) -> torch.Tensor:
    """Grow-only scratch buffer per (device, stream): kernels on one stream run in issue order, so consecutive ops share it; another
    stream (a capture stream) gets its own and never aliases it.  A buffer that is outgrown is retired, not freed, for as long as
    its (device, stream) entry lives -- HIP graphs captured on that stream hold raw pointers into it.  Growth is geometric, so the
    retired buffers together stay below the size of the live one.  Holders of captured graphs warm up ON THE CAPTURE STREAM (so the
    buffer the capture uses exists before the capture starts), keep `workspace_refs` of that stream next to their graphs and call
    `release_workspace` when the stream goes away (inference.SlidingWindow, bench --graph)."""
    key = _ws_key(device)
    ent = _workspaces.get(key)
    if ent is None:
        ent = _workspaces[key] = {"ws": None, "retired": []}
    ws = ent["ws"]
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            ent["retired"].append(ws)
        ws = torch.empty(max(int(nbytes), 2 * (ws.numel() if ws is not None else 0), 1 << 20), dtype=torch.uint8, device=device)
        ent["ws"] = ws
    return ws


def workspace_refs(device, stream=None):
    """every scratch buffer (live and retired) of one (device, stream): what a graph captured on that stream may point into"""
    ent = _workspaces.get(_ws_key(device, stream))
    return [] if ent is None else [t for t in [ent["ws"], ent.get("lin"), *ent["retired"]] if t is not None]


def release_workspace(device, stream=None) -> None:
    """forget the scratch buffers of one (device, stream); they are freed once the last holder of `workspace_refs` lets go"""
    _workspaces.pop(_ws_key(device, stream), None)


# ----------------------------------------------------------------------------- casts
def cast_op16(x: torch.Tensor, out: Optional[torch.Tensor] = None, dtype=None) -> torch.Tensor:
    """f32 -> the 16-bit operand format (``out``'s, ``dtype``, or the process-wide one)"""
    _req(x, torch.float32, "cast_op16.x")
    if out is None:
        out = torch.empty(x.shape, dtype=dtype or _op16, device=x.device)
    op = _req16(out, "cast_op16.out")
    with _timed("cast", 0.0, 6.0 * x.numel()):
        check(_fn("tad_cast_f32_bf16", op)(x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "tad_cast_f32_bf16")
    return out


def transpose_cast_op16(w: torch.Tensor, dtype=None) -> torch.Tensor:
    """w [R,C] f32 -> [C,R] in the 16-bit operand format"""
    _req(w, torch.float32, "transpose_cast.w")
    R, Cc = w.shape
    out = torch.empty((Cc, R), dtype=dtype or _op16, device=w.device)
    check(_fn("tad_transpose_cast_f32_bf16", out.dtype)(w.data_ptr(), out.data_ptr(), R, Cc, _stream()), "tad_transpose_cast")
    return out


cast_bf16, transpose_cast_bf16 = cast_op16, transpose_cast_op16  # (names from before the half format existed)


def transpose_table(mats):
    """Host-side tile list for transpose_bf16_batched: mats = [(element offset, R, C)], every matrix stored [R,C] row-major at
    ``offset`` of the source buffer and written [C,R] at the same offset of the destination.  Returns an int32 [n_tiles, 8] tensor."""
    rows = []
    for off, R, C in mats:
        if R % 8 or C % 8 or off % 8:
            raise _lib.TadError(f"transpose_table: matrix [{R},{C}] at {off} is not made of whole 16-byte chunks")
        for r0 in range(0, R, 64):
            for c0 in range(0, C, 64):
                rows.append((off + r0 * C + c0, off + c0 * R + r0, C, R, min(64, R - r0), min(64, C - c0), 0, 0))
    import numpy as np
    arr = np.asarray(rows, dtype=np.int64).reshape(-1, 8)
    if arr.size and int(arr[:, :2].max()) >= (1 << 32):
        raise _lib.TadError("transpose_table: offsets exceed 2^32 elements")
    return torch.from_numpy(arr.astype(np.uint32).view(np.int32))


def transpose_bf16_batched(src, dst, table):
    """16-bit transposes: moves bit patterns, so one entry point serves both operand formats"""
    _req16(dst, "transpose_batched.dst", like=_req16(src, "transpose_batched.src"))
    if table.dtype != torch.int32 or not table.is_cuda or table.dim() != 2 or table.shape[1] != 8 or not table.is_contiguous():
        raise _lib.TadError("transpose_bf16_batched: table must be a contiguous int32 [n_tiles, 8] device tensor")
    with _timed("cast", 0.0, 4.0 * 4096 * table.shape[0]):
        check(_lib.load().tad_transpose_bf16_batched(src.data_ptr(), dst.data_ptr(), table.data_ptr(), table.shape[0], _stream()),
              "tad_transpose_bf16_batched")
    return dst


def scale_cast_op16(x, gamma=None, rowscale=None, rows_per_scale=1, dtype=None):
    _req(x, torch.float32, "scale_cast.x")
    M, N = x.shape
    out = torch.empty((M, N), dtype=dtype or _op16, device=x.device)
    with _timed("cast", 0.0, 6.0 * M * N):
        check(_fn("tad_scale_cast_bf16", out.dtype)(x.data_ptr(), out.data_ptr(), _p(gamma), _p(rowscale), int(rows_per_scale), M, N,
                                                    _stream()), "tad_scale_cast_bf16")
    return out


scale_cast_bf16 = scale_cast_op16


# ----------------------------------------------------------------------------- fused Block variants (csrc/layerscale.hip)
def rowscale_transpose_cast(w, gamma, dtype=None):
    """w [N,K] f32, gamma [N] f32 -> [K,N] 16-bit: op16(gamma[n] * w[n,k]), the wT operand of linear_bwd_input of a layer-scaled Linear"""
    _req(w, torch.float32, "rowscale_transpose_cast.w")
    _req(gamma, torch.float32, "rowscale_transpose_cast.gamma")
    N, Kk = w.shape
    if gamma.numel() != N:
        raise _lib.TadError(f"rowscale_transpose_cast: gamma has {gamma.numel()} elements, w {N} rows")
    out = torch.empty((Kk, N), dtype=dtype or _op16, device=w.device)
    with _timed("cast", 0.0, 6.0 * N * Kk):
        check(_fn("tad_rowscale_transpose_cast", out.dtype)(w.data_ptr(), gamma.data_ptr(), out.data_ptr(), N, Kk, _stream()),
              "tad_rowscale_transpose_cast")
    return out


def layerscale_grads(T, W, bias, cs, gamma, dW=None, dbias=None, dgamma=None, accumulate=False):
    """dW = gamma[n] T[n,:], dbias = gamma * cs (None without a bias), dgamma[n] = <T[n,:], W[n,:]> + bias[n] cs[n]; with ``dW`` / ``dbias`` /
    ``dgamma`` given (all of them: gradient sinks) and ``accumulate`` they are added to.  Returns (dW, dbias|None, dgamma)."""
    _req(T, torch.float32, "layerscale_grads.T")
    _req(W, torch.float32, "layerscale_grads.W")
    _req(gamma, torch.float32, "layerscale_grads.gamma")
    N, Kk = T.shape
    if tuple(W.shape) != (N, Kk) or gamma.numel() != N:
        raise _lib.TadError(f"layerscale_grads: T {tuple(T.shape)}, W {tuple(W.shape)}, gamma {gamma.numel()}")
    if bias is not None:
        _req(bias, torch.float32, "layerscale_grads.bias")
        if cs is None or bias.numel() != N:
            raise _lib.TadError("layerscale_grads: a bias needs the column sums cs, both [N]")
    if cs is not None:
        _req(cs, torch.float32, "layerscale_grads.cs")
        assert cs.numel() == N
    given = [t is not None for t in (dW, dgamma)] + ([dbias is not None] if bias is not None else [])
    if any(given) and not all(given):
        raise _lib.TadError("layerscale_grads: give all of dW, dbias, dgamma or none")
    if not any(given):
        accumulate = False
        dW = torch.empty((N, Kk), dtype=torch.float32, device=T.device)
        dgamma = torch.empty(N, dtype=torch.float32, device=T.device)
        dbias = torch.empty(N, dtype=torch.float32, device=T.device) if bias is not None else None
    for t, n in ((dW, N * Kk), (dgamma, N)) + (((dbias, N),) if bias is not None else ()):
        _req(t, torch.float32, "layerscale_grads.out")
        assert t.numel() == n
    if bias is None:
        dbias = None
    with _timed("cast", 2.0 * N * Kk, (16.0 if accumulate else 12.0) * N * Kk):
        check(_lib.load().tad_layerscale_grads(T.data_ptr(), W.data_ptr(), _p(bias), _p(cs), gamma.data_ptr(), dW.data_ptr(), _p(dbias),
                                               dgamma.data_ptr(), int(bool(accumulate)), N, Kk, _stream()), "tad_layerscale_grads")
    return dW, dbias, dgamma


def _req_rowscale(rowscale, rows_per_scale, M, name):
    if rowscale is not None:
        _req(rowscale, torch.float32, name + ".rowscale")
        if rows_per_scale <= 0 or rowscale.numel() * rows_per_scale < M:
            raise _lib.TadError(f"{name}: rowscale has {rowscale.numel()} entries of {rows_per_scale} rows for {M} rows")


def branch_dropout_fwd(u, res, gamma=None, rowscale=None, rows_per_scale=1, p: float = 0.0, seed: int = 0):
    """out f32 [M,D] = res + rowscale * gamma * keep / (1 - p) * u; keep[m,c] = hash32(m, c, seed) >= p * 2^32.  Rows whose rowscale is 0 and
    dropped elements are ``res`` bit for bit."""
    _req(u, torch.float32, "branch_dropout_fwd.u")
    _req(res, torch.float32, "branch_dropout_fwd.res")
    M, D = u.shape
    if tuple(res.shape) != (M, D):
        raise _lib.TadError(f"branch_dropout_fwd: u {tuple(u.shape)} vs res {tuple(res.shape)}")
    if gamma is not None:
        _req(gamma, torch.float32, "branch_dropout_fwd.gamma")
        assert gamma.numel() == D
    _req_rowscale(rowscale, rows_per_scale, M, "branch_dropout_fwd")
    out = torch.empty((M, D), dtype=torch.float32, device=u.device)
    with _timed("cast", 0.0, 12.0 * M * D):
        check(_lib.load().tad_branch_dropout_fwd(u.data_ptr(), res.data_ptr(), out.data_ptr(), _p(gamma), _p(rowscale), int(rows_per_scale),
                                                 float(p), int(seed) & 0xFFFFFFFF, M, D, _stream()), "tad_branch_dropout_fwd")
    return out


def branch_dropout_cast(g, rowscale=None, rows_per_scale=1, p: float = 0.0, seed: int = 0, dtype=None):
    """op16(rowscale * keep / (1 - p) * g) [M,D]: scale_cast_op16 under the mask of branch_dropout_fwd (no gamma)"""
    _req(g, torch.float32, "branch_dropout_cast.g")
    M, D = g.shape
    _req_rowscale(rowscale, rows_per_scale, M, "branch_dropout_cast")
    out = torch.empty((M, D), dtype=dtype or _op16, device=g.device)
    with _timed("cast", 0.0, 6.0 * M * D):
        check(_fn("tad_branch_dropout_cast", out.dtype)(g.data_ptr(), out.data_ptr(), _p(rowscale), int(rows_per_scale), float(p),
                                                         int(seed) & 0xFFFFFFFF, M, D, _stream()), "tad_branch_dropout_cast")
    return out


# ----------------------------------------------------------------------------- patch embed
def patch_embed_ldk(C: int, tubelet: int, patch: int) -> int:
    """row stride of the patch matrix / the bf16 weight (K rounded up to 64; == K for /16)"""
    return int(_lib.load().tad_patch_embed_ldk(int(C), int(tubelet), int(patch)))


def pad_k(w: torch.Tensor, ldk: int) -> torch.Tensor:
    """[N, K] -> [N, ldk] with zero columns (the weight operand of a patch-embed GEMM whose K is not a multiple of 64)"""
    return w if w.shape[1] == ldk else torch.nn.functional.pad(w, (0, ldk - w.shape[1]))


def _f3(values):
    """three host floats (a per-channel mean or std) as the C entry points take them"""
    return (C.c_float * 3)(*[float(v) for v in values])


def _patch_matrix(B, Cc, T, H, W, tubelet, patch, dtype, device):
    """(tokens per clip, the empty patch matrix [B*ntok, tad_patch_embed_ldk]) of B clips [Cc,T,H,W]"""
    ntok = (T // tubelet) * (H // patch) * (W // patch)
    return ntok, torch.empty((B * ntok, patch_embed_ldk(Cc, tubelet, patch)), dtype=dtype, device=device)


def im2col_tubelets(x: torch.Tensor, tubelet: int, patch: int, dtype=None) -> torch.Tensor:
    _req(x, torch.float32, "im2col.x")
    B, Cc, T, H, W = x.shape
    _, cols = _patch_matrix(B, Cc, T, H, W, tubelet, patch, dtype or _op16, x.device)
    check(_fn("tad_im2col_tubelets", cols.dtype)(x.data_ptr(), cols.data_ptr(), B, Cc, T, H, W, tubelet, patch, _stream()),
          "tad_im2col_tubelets")
    return cols


def im2col_tubelets_16(x: torch.Tensor, tubelet: int, patch: int) -> Optional[torch.Tensor]:
    """x [B,C,T,H,W] bf16 / half -> the patch matrix in the same format, a move of 16-bit words (tad_im2col_tubelets_16).  Returns None
    when x is a view whose address the kernel's loads cannot take (16 bytes for patch sizes that are multiples of 8, else 4): the caller
    then goes through the f32 route, as for the implicit patch embedding -- it is a choice between two equal results, not an error."""
    op = _req16(x, "im2col_16.x")
    B, Cc, T, H, W = x.shape
    if x.data_ptr() % (4 if patch % 8 else 16):
        return None
    _, cols = _patch_matrix(B, Cc, T, H, W, tubelet, patch, op, x.device)
    with _timed("im2col_16", 0.0, 2.0 * x.numel() + 2.0 * cols.numel()):
        check(_lib.load().tad_im2col_tubelets_16(x.data_ptr(), cols.data_ptr(), B, Cc, T, H, W, tubelet, patch, _stream()),
              "tad_im2col_tubelets_16")
    return cols


def im2col_tubelets_u8(frames: torch.Tensor, tubelet: int, patch: int, mean, std, bgr: bool = False, t_offset: int = 0, dtype=None) -> torch.Tensor:
    """frames [B,T,H,W,3] uint8 -> normalised bf16 patch matrix [B*N, 3*tub*p*p] (tad_im2col_tubelets_u8)"""
    _req(frames, torch.uint8, "im2col_u8.frames")
    if frames.dim() != 5 or frames.shape[-1] != 3:
        raise _lib.TadError(f"im2col_u8: frames must be [B,T,H,W,3] uint8, got {tuple(frames.shape)}")
    B, T, H, W, _ = frames.shape
    _, cols = _patch_matrix(B, 3, T, H, W, tubelet, patch, dtype or _op16, frames.device)
    with _timed("im2col_u8", 0.0, float(frames.numel()) + 2.0 * cols.numel()):
        check(_fn("tad_im2col_tubelets_u8", cols.dtype)(frames.data_ptr(), cols.data_ptr(), B, T, H, W, tubelet, patch, _f3(mean), _f3(std),
                                                 int(bool(bgr)), int(t_offset), _stream()), "tad_im2col_tubelets_u8")
    return cols


def im2col_frame_windows(store: torch.Tensor, idx: torch.Tensor, tubelet: int, patch: int, mean, std, bgr: bool = False, dtype=None) -> torch.Tensor:
    """store [F,H,W,3] uint8, idx [B,T] int32 (device; the CALLER has checked 0 <= idx < F on the host: frame_store.FrameStore.windows)
    -> the normalised 16-bit patch matrix of the B windows store[idx], bit-identical to im2col_tubelets_u8(store[idx])
    (tad_im2col_frame_windows; one entry point, the operand format travels as an argument)"""
    _req(store, torch.uint8, "im2col_frame_windows.store")
    _req(idx, torch.int32, "im2col_frame_windows.idx")
    if store.dim() != 4 or store.shape[-1] != 3:
        raise _lib.TadError(f"im2col_frame_windows: store must be [F,H,W,3] uint8, got {tuple(store.shape)}")
    if idx.dim() != 2 or idx.device != store.device:
        raise _lib.TadError(f"im2col_frame_windows: idx must be [B,T] int32 on {store.device}, got {tuple(idx.shape)} on {idx.device}")
    F, H, W, _ = store.shape
    B, T = idx.shape
    _, cols = _patch_matrix(B, 3, T, H, W, tubelet, patch, dtype or _op16, store.device)
    _req16(cols, "im2col_frame_windows.cols")
    with _timed("im2col_u8", 0.0, float(B * T * H * W * 3) + 2.0 * cols.numel()):
        check(_lib.load().tad_im2col_frame_windows(store.data_ptr(), F, idx.data_ptr(), cols.data_ptr(), _dt(cols), B, T, H, W, tubelet, patch,
                                                   _f3(mean), _f3(std), int(bool(bgr)), _stream()), "tad_im2col_frame_windows")
    return cols


def patch_embed_gemm(cols, w_bf16, bias, pos, ntok: int):
    """cols [B*ntok, K] bf16 -> out [B, ntok, D] f32 = cols w^T + bias (+ pos [ntok, D] broadcast over the batch)"""
    op = _req16(cols, "patch_embed_gemm.cols")
    _req16(w_bf16, "patch_embed_gemm.w", like=op)
    M, Kd = cols.shape
    D, K2 = w_bf16.shape
    if Kd != K2 or M % ntok:
        raise _lib.TadError(f"patch_embed_gemm: cols {tuple(cols.shape)} vs weight {tuple(w_bf16.shape)}, ntok {ntok}")
    if pos is not None:
        _req(pos, torch.float32, "patch_embed_gemm.pos")
        if tuple(pos.shape) != (ntok, D):
            raise _lib.TadError(f"patch_embed_gemm: pos_embed shape {tuple(pos.shape)} != {(ntok, D)}")
    if bias is not None:
        _req(bias, torch.float32, "patch_embed_gemm.bias")
    out = torch.empty((M // ntok, ntok, D), dtype=torch.float32, device=cols.device)
    with _timed("patch_embed_fwd", 2.0 * M * D * Kd, 2.0 * M * Kd + 4.0 * M * D):
        check(_fn("tad_patch_embed_gemm", op)(cols.data_ptr(), w_bf16.data_ptr(), _p(bias), _p(pos), out.data_ptr(), M, ntok, D, Kd,
                                               _stream()), "tad_patch_embed_gemm")
    return out


def patch_embed_fwd(x, w_bf16, bias, pos, tubelet: int, patch: int):
    """x [B,C,T,H,W] f32, w_bf16 [D,K], bias [D] f32|None, pos [N,D] f32|None -> (out [B,N,D] f32, cols [B*N,K] bf16)"""
    _req(x, torch.float32, "patch_embed.x")
    op = _req16(w_bf16, "patch_embed.w")
    B, Cc, T, H, W = x.shape
    D, K = w_bf16.shape
    if K != patch_embed_ldk(Cc, tubelet, patch):
        raise _lib.TadError(f"patch_embed: weight row stride {K} does not match tad_patch_embed_ldk = {patch_embed_ldk(Cc, tubelet, patch)} "
                            f"(C*tub*p*p = {Cc * tubelet * patch * patch} rounded up to 64; kernels.pad_k)")
    ntok = (T // tubelet) * (H // patch) * (W // patch)
    if pos is not None:
        _req(pos, torch.float32, "patch_embed.pos")
        if tuple(pos.shape) != (ntok, D):
            raise _lib.TadError(f"patch_embed: pos_embed shape {tuple(pos.shape)} != {(ntok, D)}")
    if bias is not None:
        _req(bias, torch.float32, "patch_embed.bias")
    cols = torch.empty((B * ntok, K), dtype=op, device=x.device)
    out = torch.empty((B, ntok, D), dtype=torch.float32, device=x.device)
    with _timed("patch_embed_fwd", 2.0 * B * ntok * D * K, 4.0 * x.numel() + 2.0 * 2 * B * ntok * K + 4.0 * B * ntok * D):
        check(_fn("tad_patch_embed_fwd", op)(x.data_ptr(), w_bf16.data_ptr(), _p(bias), _p(pos), out.data_ptr(), cols.data_ptr(),
                                              B, Cc, T, H, W, tubelet, patch, D, _stream()), "tad_patch_embed_fwd")
    return out, cols


def patch_embed_fwd_implicit(x, w_bf16, bias, pos, tubelet: int, patch: int):
    """the same forward without a patch matrix (tad_patch_embed_fwd_implicit: the x operand read straight from the f32 clip); for forwards that keep
    nothing for a backward pass.  Returns out [B,N,D] f32, or None when the implicit kernel does not take the case (patch != 16, a clip of 2 GiB
    and more): the caller then uses patch_embed_fwd"""
    _req(x, torch.float32, "patch_embed.x")
    op = _req16(w_bf16, "patch_embed.w")
    B, Cc, T, H, W = x.shape
    D, K = w_bf16.shape
    if patch != 16 or K != Cc * tubelet * 256 or x.numel() * 4 >= (1 << 31) or D % 4 or T % tubelet or H % 16 or W % 16:
        return None
    ntok = (T // tubelet) * (H // patch) * (W // patch)
    if pos is not None:
        _req(pos, torch.float32, "patch_embed.pos")
        if tuple(pos.shape) != (ntok, D):
            raise _lib.TadError(f"patch_embed: pos_embed shape {tuple(pos.shape)} != {(ntok, D)}")
    if bias is not None:
        _req(bias, torch.float32, "patch_embed.bias")
    out = torch.empty((B, ntok, D), dtype=torch.float32, device=x.device)
    with _timed("patch_embed_fwd", 2.0 * B * ntok * D * K, 4.0 * x.numel() + 4.0 * B * ntok * D):
        check(_fn("tad_patch_embed_fwd_implicit", op)(x.data_ptr(), w_bf16.data_ptr(), _p(bias), _p(pos), out.data_ptr(), B, Cc, T, H, W, tubelet, patch, D,
                                                       _stream()), "tad_patch_embed_fwd_implicit")
    return out


# ----------------------------------------------------------------------------- layernorm
def layernorm_fwd(x, gamma, beta, eps: float, out_dtype=None, save_stats=True):
    """out_dtype: torch.float32, or a 16-bit operand format (None = the process-wide one)"""
    _req(x, torch.float32, "layernorm.x")
    _req(gamma, torch.float32, "layernorm.gamma")
    _req(beta, torch.float32, "layernorm.beta")
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty(x.shape, dtype=out_dtype or _op16, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    with _timed("layernorm_fwd", 0.0, rows * D * (4.0 + y.element_size())):
        check(_fn("tad_layernorm_fwd", y.dtype if y.dtype in OP16_DTYPES else _op16)(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), _dt(y), _p(mean), _p(rstd),
                                            rows, D, float(eps), _stream()), "tad_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dres=None, want_bf16=False, want_colsum=False, rowscale=None, rows_per_scale=1,
                  into=None):
    """returns dx f32, dx_bf16|None, dgamma, dbeta, colsum_dx|None.  rowscale [rows/rows_per_scale]: per-sample scale applied to the
    bf16 copy and the column sums (drop-path).  into=(dgamma, dbeta, colsum|None): accumulate the three reductions into these
    existing f32 tensors (gradient sinks) instead of returning fresh ones."""
    _req(x, torch.float32, "layernorm_bwd.x")
    if dy.dtype not in (torch.float32,) + OP16_DTYPES or not dy.is_contiguous():
        raise _lib.TadError("layernorm_bwd.dy: must be contiguous f32, bf16 or f16")
    op = dy.dtype if dy.dtype in OP16_DTYPES else _op16  # format of the 16-bit copy of dx (and of dy, if it is 16-bit)
    D = x.shape[-1]
    rows = x.numel() // D
    if dres is not None:
        _req(dres, torch.float32, "layernorm_bwd.dres")
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    dxb = torch.empty(x.shape, dtype=op, device=x.device) if want_bf16 else None
    if into is not None:
        dg, db, cs = into
        for t in (dg, db) + ((cs,) if want_colsum else ()):
            _req(t, torch.float32, "layernorm_bwd.into")
            assert t.numel() == D
        if not want_colsum:
            cs = None
    else:
        dg = torch.empty(D, dtype=torch.float32, device=x.device)
        db = torch.empty(D, dtype=torch.float32, device=x.device)
        cs = torch.empty(D, dtype=torch.float32, device=x.device) if want_colsum else None
    if rowscale is not None:
        _req(rowscale, torch.float32, "layernorm_bwd.rowscale")
        assert rowscale.numel() * rows_per_scale >= rows
    lib = _lib.load()
    nbytes = lib.tad_layernorm_bwd_workspace_bytes(rows, D)
    ws = workspace(nbytes, x.device)
    with _timed("layernorm_bwd", 0.0, rows * D * (dy.element_size() + 4.0 + 4.0 + (4.0 if dres is not None else 0.0) + (2.0 if want_bf16 else 0.0))):
        check(_fn("tad_layernorm_bwd", op)(dy.data_ptr(), _dt(dy), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _p(dres),
                                    dx.data_ptr(), _p(dxb), dg.data_ptr(), db.data_ptr(), _p(cs), _p(rowscale), int(rows_per_scale),
                                    int(into is not None), ws.data_ptr(), ws.numel(), rows, D, _stream()), "tad_layernorm_bwd")
    return dx, dxb, dg, db, cs


# ----------------------------------------------------------------------------- RMSNorm, q / k RMS normalisation (extension ABI)
def _ext(name: str):
    return getattr(_lib.load(), name)


def rmsnorm_fwd(x, gamma, eps: float, out_dtype=None, save_stats=True):
    """y = x * rsqrt(mean(x^2) + eps) * gamma.  out_dtype: torch.float32, or a 16-bit operand format (None = the process-wide one).
    Returns y, rrms [rows] | None."""
    _req(x, torch.float32, "rmsnorm.x")
    _req(gamma, torch.float32, "rmsnorm.gamma")
    D = x.shape[-1]
    rows = x.numel() // D
    assert gamma.numel() == D
    y = torch.empty(x.shape, dtype=out_dtype or _op16, device=x.device)
    rrms = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    with _timed("rmsnorm_fwd", 0.0, rows * D * (4.0 + y.element_size())):
        check(_ext("tadx_rmsnorm_fwd")(x.data_ptr(), gamma.data_ptr(), y.data_ptr(), _dt(y), _p(rrms), rows, D, float(eps), _stream()),
              "tadx_rmsnorm_fwd")
    return y, rrms


def rmsnorm_bwd(dy, x, gamma, rrms, dres=None, want_op16=False, into=None):
    """returns dx f32, dx16 | None, dgamma.  dy: f32 or a 16-bit operand format (dx16 takes that format, else the process-wide one).
    into: an existing f32 [D] tensor the gamma gradient is ADDED to (a gradient sink) instead of a fresh one."""
    _req(x, torch.float32, "rmsnorm_bwd.x")
    _req(gamma, torch.float32, "rmsnorm_bwd.gamma")
    _req(rrms, torch.float32, "rmsnorm_bwd.rrms")
    if not dy.is_cuda or dy.dtype not in (torch.float32,) + OP16_DTYPES or not dy.is_contiguous():
        raise _lib.TadError("rmsnorm_bwd.dy: must be a contiguous GPU tensor, f32, bf16 or f16")
    op = dy.dtype if dy.dtype in OP16_DTYPES else _op16
    D = x.shape[-1]
    rows = x.numel() // D
    assert dy.numel() == x.numel() and rrms.numel() == rows and gamma.numel() == D
    if dres is not None:
        _req(dres, torch.float32, "rmsnorm_bwd.dres")
        assert dres.numel() == x.numel()
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    dx16 = torch.empty(x.shape, dtype=op, device=x.device) if want_op16 else None
    if into is not None:
        _req(into, torch.float32, "rmsnorm_bwd.into")
        assert into.numel() == D
        dg = into
    else:
        dg = torch.empty(D, dtype=torch.float32, device=x.device)
    nbytes = _ext("tadx_rmsnorm_bwd_workspace_bytes")(rows, D)
    ws = workspace(nbytes, x.device)
    with _timed("rmsnorm_bwd", 0.0, rows * D * (dy.element_size() + 4.0 + 4.0 + (4.0 if dres is not None else 0.0) + (2.0 if want_op16 else 0.0))):
        check(_ext("tadx_rmsnorm_bwd")(dy.data_ptr(), _dt(dy), x.data_ptr(), gamma.data_ptr(), rrms.data_ptr(), _p(dres), dx.data_ptr(), _p(dx16),
                                       TAD_F16 if op == torch.float16 else TAD_BF16, dg.data_ptr(), int(into is not None), ws.data_ptr(),
                                       ws.numel(), rows, D, _stream()), "tadx_rmsnorm_bwd")
    return dx, dx16, dg


def qk_rmsnorm_fwd(qkv32, gq, gk, eps: float, q_out_scale: float = 1.0, dtype=None, save_stats=True):
    """qkv32 [M,3A] f32 -> qkv16 [M,3A]: q * rq * gq * q_out_scale | k * rk * gk | v, each rounded once; rr [M,2] = (rq, rk) | None.
    q_out_scale: the q contract of attn_fwd (q_prescale_of(scale) for pre-scaled q, else 1)."""
    _req(qkv32, torch.float32, "qk_rmsnorm.qkv32")
    _req(gq, torch.float32, "qk_rmsnorm.gq")
    _req(gk, torch.float32, "qk_rmsnorm.gk")
    M, A3 = qkv32.shape
    A = A3 // 3
    assert A * 3 == A3 and gq.numel() == A and gk.numel() == A
    out = torch.empty((M, A3), dtype=dtype or _op16, device=qkv32.device)
    op = _req16(out, "qk_rmsnorm.out")
    rr = torch.empty((M, 2), dtype=torch.float32, device=qkv32.device) if save_stats else None
    with _timed("qk_rmsnorm_fwd", 0.0, M * A3 * 6.0):
        check(_ext("tadx_qk_rmsnorm_fwd")(qkv32.data_ptr(), gq.data_ptr(), gk.data_ptr(), out.data_ptr(), _dt(out), _p(rr), float(q_out_scale),
                                          M, A, float(eps), _stream()), "tadx_qk_rmsnorm_fwd")
    return out, rr


def qk_rmsnorm_bwd(dqkv16, qkv32, gq, gk, rr, q_out_scale: float = 1.0, into=None):
    """attn_bwd's dqkv [M,3A] back through the two norms: returns the 16-bit gradient of the qkv Linear's output, dgq, dgk.
    into = (dgq, dgk): existing f32 [A] tensors the gamma gradients are ADDED to."""
    op = _req16(dqkv16, "qk_rmsnorm_bwd.dqkv16")
    _req(qkv32, torch.float32, "qk_rmsnorm_bwd.qkv32")
    _req(gq, torch.float32, "qk_rmsnorm_bwd.gq")
    _req(gk, torch.float32, "qk_rmsnorm_bwd.gk")
    _req(rr, torch.float32, "qk_rmsnorm_bwd.rr")
    M, A3 = qkv32.shape
    A = A3 // 3
    assert A * 3 == A3 and dqkv16.numel() == qkv32.numel() and rr.numel() == 2 * M and gq.numel() == A and gk.numel() == A
    out = torch.empty((M, A3), dtype=op, device=qkv32.device)
    if into is not None:
        dgq, dgk = into
        for t in into:
            _req(t, torch.float32, "qk_rmsnorm_bwd.into")
            assert t.numel() == A
    else:
        dgq = torch.empty(A, dtype=torch.float32, device=qkv32.device)
        dgk = torch.empty(A, dtype=torch.float32, device=qkv32.device)
    nbytes = _ext("tadx_qk_rmsnorm_bwd_workspace_bytes")(M, A)
    ws = workspace(nbytes, qkv32.device)
    with _timed("qk_rmsnorm_bwd", 0.0, M * A3 * 8.0 - M * A * 4.0):
        check(_ext("tadx_qk_rmsnorm_bwd")(dqkv16.data_ptr(), _dt(dqkv16), qkv32.data_ptr(), gq.data_ptr(), gk.data_ptr(), rr.data_ptr(),
                                          float(q_out_scale), out.data_ptr(), dgq.data_ptr(), dgk.data_ptr(), int(into is not None),
                                          ws.data_ptr(), ws.numel(), M, A, _stream()), "tadx_qk_rmsnorm_bwd")
    return out, dgq, dgk


# ----------------------------------------------------------------------------- linear
def linear_fwd(x, w, bias=None, out_dtype=None, epilogue=EPI_BIAS, want_preact=False, residual=None, gamma=None,
               rowscale=None, rows_per_scale=1):
    """x [M,K], w [N,K] (both bf16 or both f16) -> y [M,N] (out_dtype: f32, or None = the operands' format); returns (y, preact|None)"""
    op = _req16(x, "linear.x")
    _req16(w, "linear.w", like=op)
    out_dtype = _out16(out_dtype, op)
    if x.shape[1] == w.shape[1] and x.shape[1] % 64:
        x, w = _pad_reduction(x, w)  # reduction length off the 64-deep K-tile (a 1176-wide MAE decoder head of a /14 model): zero columns
    M, K = x.shape
    N, K2 = w.shape
    if K != K2:
        raise _lib.TadError(f"linear: x K={K} vs w K={K2}")
    if bias is not None:
        _req(bias, torch.float32, "linear.bias")
        assert bias.numel() == N
    if residual is not None:
        _req(residual, torch.float32, "linear.residual")
        assert tuple(residual.shape) == (M, N)
    y = torch.empty((M, N), dtype=out_dtype, device=x.device)
    pre = torch.empty((M, N), dtype=op, device=x.device) if want_preact else None
    ws, wsb = _linear_ws(M, N, K, x.device)
    # algorithmic bytes of the launch: both operands once, the output once, plus what the epilogue reads (f32 residual) / writes (16-bit pre-activation)
    with _timed("gemm_nt", 2.0 * M * N * K, 2.0 * (M * K + N * K) + y.element_size() * M * N + (4.0 * M * N if residual is not None else 0.0)
                + (2.0 * M * N if want_preact else 0.0)):
        check(_fn("tad_linear_fwd", op)(x.data_ptr(), w.data_ptr(), _p(bias), y.data_ptr(), _dt(y), epilogue, _p(pre), _p(residual),
                                         _p(gamma), _p(rowscale), int(rows_per_scale), ws, wsb, M, N, K, _stream()), "tad_linear_fwd")
    return y, pre


# Split-K tails of the Linear GEMMs (include/tad_mi355x.h: tad_linear_fwd's `ws`): a per-(device, stream) scratch buffer is handed to the
# Linear calls unless switched off here (experiments).  parallel.DataParallel leaves it ON at world sizes > 1: it pins the deferred
# three-launch form (tad_linear_tuning("splitk_defer", 1)), which is ordered by kernel boundaries and needs no co-residency beside an
# overlapped RCCL kernel; only the in-launch combine ("splitk_defer", 0) does.
_linear_splitk = True


def set_linear_splitk(on: bool):
    global _linear_splitk
    _linear_splitk = bool(on)


def _linear_ws(M, N, K, device):
    if not _linear_splitk:
        return None, 0
    nbytes = _lib.load().tad_linear_workspace_bytes(M, N, K)
    if not nbytes:
        return None, 0
    return linear_workspace(nbytes, device).data_ptr(), nbytes


def _pad_reduction(a, b, mult: int = 64):
    """zero-pad the shared last (reduction) dimension of two operands to a multiple of the GEMM's K-tile: the product is unchanged"""
    pad = (-a.shape[1]) % mult
    return torch.nn.functional.pad(a, (0, pad)).contiguous(), torch.nn.functional.pad(b, (0, pad)).contiguous()


LINEAR_TUNING_DEFAULTS = dict(persistent=1, direct_epilogue=1, split_tail=1, splitk_tail=1, group_m=0, variant=0, tn_pdeep=0, splitk_defer=1, tn_w4=1, w4_plain=640, w4_epilogues=4, tail_192=1, short_k=1, tn_pair=1)


def linear_workspace(nbytes: int, device) -> torch.Tensor:
    """scratch of the split-K Linear tails, one per (device, stream): a buffer of its own (neither buffer's growth retires the other)
    inside the SAME per-(device, stream) entry as `workspace`, so that `workspace_refs` reports it to holders of captured graphs and
    `release_workspace` drops it with the rest"""
    key = _ws_key(device)
    ent = _workspaces.get(key)
    if ent is None:
        ent = _workspaces[key] = {"ws": None, "retired": []}
    buf = ent.get("lin")
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            ent["retired"].append(buf)
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        ent["lin"] = buf
    return buf


def linear_kernel_launches() -> int:
    """gemm_nt kernel launches issued so far (tad_linear_kernel_launches)"""
    return int(_lib.load().tad_linear_kernel_launches())


def linear_tuning(**knobs):
    """Scheduling knobs of the Linear GEMMs (include/tad_mi355x.h: tad_linear_tuning); timing only, never results."""
    for k, v in knobs.items():
        check(_lib.load().tad_linear_tuning(k.encode(), int(v)), f"tad_linear_tuning({k}={v})")


def linear_tuning_get(key: str) -> int:
    """current value of a tad_linear_tuning knob"""
    v = C.c_int(0)
    check(_lib.load().tad_linear_tuning_get(key.encode(), C.byref(v)), f"tad_linear_tuning_get({key})")
    return int(v.value)


def _plan_rows(call, fields, what):
    cap = 8
    while True:
        buf = (C.c_int32 * (cap * len(fields)))()
        n = call(buf, cap)
        if n != -3:  # TAD_ENOSPACE: a problem cut into many row ranges
            break
        cap *= 8
    if n < 0:
        check(n, what)
    return [dict(zip(fields, buf[i * len(fields):(i + 1) * len(fields)])) for i in range(n)]


def linear_plan(M, N, K, epilogue=0, out_16bit=True, residual=False, res_mod=0, rowscale=False, rows_per_scale=1, colscale_cols=0, ws_bytes=0):
    """The kernel launches the Linear y [M,N] = x [M,K] w^T would run as under the current knobs, in order: a list of dicts with the keys
    _lib.LINEAR_PLAN_FIELDS (include/tad_mi355x.h: tad_linear_plan).  Launches nothing and needs no GPU.  epilogue: 0 bias, 1 GELU, 2 residual,
    3 GELU backward; for linear_bwd_input(dy [M,N], wT [K,N]) the problem is (M, K, N)."""
    lib = _lib.load()
    return _plan_rows(lambda buf, cap: lib.tad_linear_plan(M, N, K, int(epilogue), int(out_16bit), int(residual), int(res_mod), int(rowscale), int(rows_per_scale),
                                                           int(colscale_cols), int(ws_bytes), buf, cap), _lib.LINEAR_PLAN_FIELDS, "tad_linear_plan")


def linear_bwd_weight_plan(M, N, K, N2=0, ws_bytes=0):
    """The GEMM launches of linear_bwd_weight (N2 = 0) or linear_bwd_weight_pair (dW [N,K] and [N2,K]) given a workspace of ws_bytes: a list of
    dicts with the keys _lib.LINEAR_BWD_WEIGHT_PLAN_FIELDS plus "ws_bytes" (include/tad_mi355x.h: tad_linear_bwd_weight_plan)"""
    lib = _lib.load()
    rows = _plan_rows(lambda buf, cap: lib.tad_linear_bwd_weight_plan(M, N, N2, K, int(ws_bytes), buf, cap), _lib.LINEAR_BWD_WEIGHT_PLAN_FIELDS,
                      "tad_linear_bwd_weight_plan")
    for r in rows:
        r["ws_bytes"] = (r["ws_hi"] << 31) + r["ws_lo"]
    return rows


def linear_bwd_input(dy, wT, out_dtype=None, gelu_preact=None):
    """dy [M,N], wT [K,N] (both bf16 or both f16) -> dx [M,K]"""
    op = _req16(dy, "linear_bwd_input.dy")
    _req16(wT, "linear_bwd_input.wT", like=op)
    out_dtype = _out16(out_dtype, op)
    if dy.shape[1] == wT.shape[1] and dy.shape[1] % 64:
        dy, wT = _pad_reduction(dy, wT)
    M, N = dy.shape
    K, N2 = wT.shape
    assert N == N2, (N, N2)
    if gelu_preact is not None:
        _req16(gelu_preact, "linear_bwd_input.gelu_preact", like=op)
        assert tuple(gelu_preact.shape) == (M, K)
    dx = torch.empty((M, K), dtype=out_dtype, device=dy.device)
    ws, wsb = _linear_ws(M, K, N, dy.device)
    with _timed("gemm_nt", 2.0 * M * N * K, 2.0 * (M * N + N * K) + dx.element_size() * M * K + (2.0 * M * K if gelu_preact is not None else 0.0)):
        check(_fn("tad_linear_bwd_input", op)(dy.data_ptr(), wT.data_ptr(), dx.data_ptr(), _dt(dx), _p(gelu_preact), ws, wsb, M, N, K,
                                               _stream()), "tad_linear_bwd_input")
    return dx


def linear_bwd_weight(dy, x, want_bias=True, dW=None, db=None, accumulate=False):
    """dy [M,N] bf16, x [M,K] bf16 -> dW [N,K] f32, db [N] f32|None"""
    op = _req16(dy, "linear_bwd_weight.dy")
    _req16(x, "linear_bwd_weight.x", like=op)
    M, N = dy.shape
    M2, K = x.shape
    assert M == M2
    if N % 8:
        # the GEMM moves dy's rows in 16-byte pieces (N % 8 == 0, refused otherwise).  Another width -- the MAE decoder head of a 14 x 14
        # patch: 588 pixels -- gets zero columns up to the next multiple of 8, as linear_bwd_input's reduction gets them from
        # _pad_reduction: the rows of dW and the entries of db they produce are dropped, the others are the same sums on the same bits.
        # Given outputs (gradient sinks) receive the slices by one copy or, with accumulate, one add.
        tW, tb = linear_bwd_weight(torch.nn.functional.pad(dy, (0, (-N) % 8)).contiguous(), x, want_bias=want_bias)
        tW, tb = tW[:N], (tb[:N] if want_bias else None)
        if dW is None:
            dW, accumulate = tW, False
        else:
            dW.add_(tW) if accumulate else dW.copy_(tW)
        if want_bias:
            if db is None:
                db = tb
            else:
                db.add_(tb) if accumulate else db.copy_(tb)
        return dW, (db if want_bias else None)
    if dW is None:
        dW = torch.empty((N, K), dtype=torch.float32, device=dy.device)
        accumulate = False
    if want_bias and db is None:
        db = torch.empty(N, dtype=torch.float32, device=dy.device)
    lib = _lib.load()
    ws = workspace(lib.tad_linear_bwd_weight_workspace_bytes(M, N, K), dy.device)
    with _timed("gemm_tn", 2.0 * M * N * K, 2.0 * (M * N + M * K) + 4.0 * N * K):
        check(_fn("tad_linear_bwd_weight", op)(dy.data_ptr(), x.data_ptr(), dW.data_ptr(), _p(db) if want_bias else None, int(accumulate),
                                        ws.data_ptr(), ws.numel(), M, N, K, _stream()), "tad_linear_bwd_weight")
    return dW, (db if want_bias else None)


LOG2E = 1.4426950408889634


def q_prescale_of(scale: float) -> float:
    """the factor the attention kernels expect on a pre-scaled q: softmax scale * log2(e) (scores in log2 units)"""
    return float(scale) * LOG2E


def linear_fwd_qkv(x, w, q_bias, v_bias, out_dtype=None, q_prescale: float = 1.0):
    """qkv Linear with bias = cat(q_bias, 0, v_bias) (modeling_finetune.py:89-92) taken from the two parameters directly.
    q_prescale != 1: the q third of the output is multiplied by it before the rounding to the output type (`q = q * self.scale`,
    modeling_finetune.py:96, folded into the Linear; attn_fwd / attn_bwd then take q_prescaled=True)"""
    op = _req16(x, "linear_qkv.x")
    _req16(w, "linear_qkv.w", like=op)
    out_dtype = _out16(out_dtype, op)
    M, K = x.shape
    N, K2 = w.shape
    if K != K2:
        raise _lib.TadError(f"linear_qkv: x K={K} vs w K={K2}")
    if q_bias is not None:
        _req(q_bias, torch.float32, "linear_qkv.q_bias")
        _req(v_bias, torch.float32, "linear_qkv.v_bias")
        assert q_bias.numel() == v_bias.numel() == N // 3
    y = torch.empty((M, N), dtype=out_dtype, device=x.device)
    with _timed("gemm_nt", 2.0 * M * N * K, 2.0 * (M * K + N * K) + y.element_size() * M * N):
        check(_fn("tad_linear_fwd_qkv", op)(x.data_ptr(), w.data_ptr(), _p(q_bias), _p(v_bias), y.data_ptr(), _dt(y), float(q_prescale), M, N, K,
                                            _stream()), "tad_linear_fwd_qkv")
    return y


def linear_bwd_weight_qkv(dy, x, dW, dq_bias, dv_bias, accumulate):
    """weight gradient of the qkv Linear with the bias column sums split into dq_bias / dv_bias [N/3] (in place)"""
    op = _req16(dy, "linear_bwd_weight_qkv.dy")
    _req16(x, "linear_bwd_weight_qkv.x", like=op)
    M, N = dy.shape
    M2, K = x.shape
    assert M == M2 and dq_bias.numel() == dv_bias.numel() == N // 3
    lib = _lib.load()
    ws = workspace(lib.tad_linear_bwd_weight_workspace_bytes(M, N, K), dy.device)
    with _timed("gemm_tn", 2.0 * M * N * K, 2.0 * (M * N + M * K) + 4.0 * N * K):
        check(_fn("tad_linear_bwd_weight_qkv", op)(dy.data_ptr(), x.data_ptr(), dW.data_ptr(), dq_bias.data_ptr(), dv_bias.data_ptr(), int(accumulate),
                                            ws.data_ptr(), ws.numel(), M, N, K, _stream()), "tad_linear_bwd_weight_qkv")
    return dW


def linear_bwd_weight_pair(dy1, x1, dW1, db1, db1b, dy2, x2, dW2, accumulate):
    """two weight gradients over the same rows with the same K in one call (tad_linear_bwd_weight_pair): dW1 [N1,K] (+)= dy1^T x1 with its
    bias column sums (db1 [N1] | None; db1b given: the first / last third to db1 / db1b), dW2 [N2,K] (+)= dy2^T x2.  In place."""
    op = _req16(dy1, "linear_bwd_weight_pair.dy1")
    for t, n in ((x1, "x1"), (dy2, "dy2"), (x2, "x2")):
        _req16(t, "linear_bwd_weight_pair." + n, like=op)
    M, N1 = dy1.shape
    N2 = dy2.shape[1]
    K = x1.shape[1]
    assert x1.shape[0] == M and dy2.shape[0] == M and x2.shape == (M, K), "linear_bwd_weight_pair: the two problems share M and K"
    assert dW1.shape == (N1, K) and dW2.shape == (N2, K) and dW1.dtype == dW2.dtype == torch.float32
    lib = _lib.load()
    ws = workspace(max(lib.tad_linear_bwd_weight_workspace_bytes(M, n, K) for n in (N1, N2, N1 + N2)), dy1.device)
    with _timed("gemm_tn", 2.0 * M * (N1 + N2) * K, 2.0 * (M * (N1 + N2) + 2 * M * K) + 4.0 * (N1 + N2) * K):
        check(_fn("tad_linear_bwd_weight_pair", op)(dy1.data_ptr(), x1.data_ptr(), dW1.data_ptr(), _p(db1), _p(db1b), N1, dy2.data_ptr(), x2.data_ptr(),
                                                    dW2.data_ptr(), N2, int(accumulate), ws.data_ptr(), ws.numel(), M, K, _stream()),
              "tad_linear_bwd_weight_pair")


def colsum_bf16(a, out=None):
    op = _req16(a, "colsum.a")
    M, N = a.shape
    if N % 8:  # (16-byte row chunks: zero columns up to the next multiple of 8, dropped again -- as linear_bwd_weight)
        s = colsum_bf16(torch.nn.functional.pad(a, (0, (-N) % 8)).contiguous())[:N]
        return s if out is None else out.copy_(s)
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=a.device)
    lib = _lib.load()
    ws = workspace(lib.tad_colsum_workspace_bytes(M, N), a.device)
    with _timed("colsum", 0.0, 2.0 * M * N):
        check(_fn("tad_colsum_bf16", op)(a.data_ptr(), out.data_ptr(), 0, ws.data_ptr(), ws.numel(), M, N, _stream()), "tad_colsum_bf16")
    return out


# ----------------------------------------------------------------------------- attention
def attn_fwd(qkv, B: int, N: int, H: int, scale: float, out_dtype=None, want_lse=True, want_lo=False, q_prescaled=False, drop_p: float = 0.0,
             seed: int = 0, d: int = 64, rowscale=None):
    """qkv [B*N, 3*H*d] bf16 or f16 (packed [B,N,3,H,d], d = 64 or 80) -> out [B*N, H*d], lse [B,H,N] f32.  want_lo: returns
    (out, lse, out_lo) with out_lo = what the 16-bit rounding of out dropped (for attn_bwd's delta).  q_prescaled: the q third already
    carries scale * log2(e) (linear_fwd_qkv's q_prescale = q_prescale_of(scale)).  rowscale [B] f32 | None: the per-clip drop-path scale
    of the residual behind this attention (tad_attn_fwd's clip_scale): clips with scale 0 are filled (out = 0), not computed"""
    op = _req16(qkv, "attn.qkv")
    out_dtype = _out16(out_dtype, op)
    if qkv.numel() != B * N * 3 * H * d:
        raise _lib.TadError(f"attn_fwd: qkv has {qkv.numel()} elements, expected {B * N * 3 * H * d}")
    out = torch.empty((B * N, H * d), dtype=out_dtype, device=qkv.device)
    lse = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device) if want_lse else None
    lo = torch.empty_like(out) if (want_lo and out.dtype in OP16_DTYPES) else None
    _req_clip_scale(rowscale, B)
    with _timed("attn_fwd", 4.0 * B * H * N * N * d, 2.0 * (4 + (lo is not None)) * B * N * H * d):
        check(_fn("tad_attn_fwd", op)(qkv.data_ptr(), out.data_ptr(), _dt(out), _p(lo), _p(lse), _p(rowscale), B, N, H, int(d), float(scale),
                                      int(bool(q_prescaled)), float(drop_p), int(seed) & 0xffffffff, _stream()), "tad_attn_fwd")
    return (out, lse, lo) if want_lo else (out, lse)


def _req_clip_scale(rowscale, B: int):
    if rowscale is not None:
        _req(rowscale, torch.float32, "attn.rowscale")
        if rowscale.numel() != B:
            raise _lib.TadError(f"attn: rowscale has {rowscale.numel()} elements, expected one per clip ({B})")


def attn_tuning(**knobs):
    """Scheduling knobs of the attention kernels (include/tad_mi355x.h: tad_attn_tuning); timing only, never results."""
    for k, v in knobs.items():
        check(_lib.load().tad_attn_tuning(k.encode(), int(v)), f"tad_attn_tuning({k}={v})")


def attn_tuning_get(key: str) -> int:
    """current value of a tad_attn_tuning knob"""
    v = C.c_int(0)
    check(_lib.load().tad_attn_tuning_get(key.encode(), C.byref(v)), f"tad_attn_tuning_get({key})")
    return int(v.value)


def attn_plan(B: int, N: int, H: int, d: int = 64, backward=False, out_16bit=True, q_prescaled=False, drop_p: float = 0.0, rowscale=False, out_lo=False):
    """The kernel launches attn_fwd (or, backward=True, attn_bwd: dQ then dK/dV) would make under the current knobs: a list of dicts with the keys
    _lib.ATTN_PLAN_FIELDS (include/tad_mi355x.h: tad_attn_plan).  rowscale / out_lo (bool): the operand is given.  Launches nothing, needs no GPU."""
    lib = _lib.load()
    return _plan_rows(lambda buf, cap: lib.tad_attn_plan(int(bool(backward)), B, N, H, int(d), int(bool(out_16bit)), int(bool(q_prescaled)), float(drop_p),
                                                         int(bool(rowscale)), int(bool(out_lo)), buf, cap), _lib.ATTN_PLAN_FIELDS, "tad_attn_plan")


def attn_bwd(qkv, out, dout, lse, B: int, N: int, H: int, scale: float, out_lo=None, q_prescaled=False, drop_p: float = 0.0, seed: int = 0,
             d: int = 64, rowscale=None):
    """dqkv; its q slot is the gradient of the PLAIN q whether or not the q of `qkv` is pre-scaled.  rowscale: as in attn_fwd (the dout rows
    of a clip with scale 0 are zeros: so is its dqkv, stored without being computed)"""
    op = _req16(qkv, "attn_bwd.qkv")
    for t, n in ((out, "out"), (dout, "dout")) + (((out_lo, "out_lo"),) if out_lo is not None else ()):
        _req16(t, "attn_bwd." + n, like=op)
        if t.numel() != B * N * H * d:
            raise _lib.TadError(f"attn_bwd: {n} has {t.numel()} elements, expected {B * N * H * d}")
    _req(lse, torch.float32, "attn_bwd.lse")
    if qkv.numel() != B * N * 3 * H * d or lse.numel() != B * H * N:
        raise _lib.TadError("attn_bwd: qkv / lse element count mismatch")
    _req_clip_scale(rowscale, B)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((_lib.load().tad_attn_bwd_scratch_bytes(B, N, H) // 4,), dtype=torch.float32, device=qkv.device)  # -rowsum(dout*out), -lse/scale
    with _timed("attn_bwd", 8.0 * B * H * N * N * d, 2.0 * (8 + (out_lo is not None)) * B * N * H * d):
        check(_fn("tad_attn_bwd", op)(qkv.data_ptr(), out.data_ptr(), _p(out_lo), dout.data_ptr(), lse.data_ptr(), _p(rowscale), dqkv.data_ptr(),
                                       delta.data_ptr(), B, N, H, int(d), float(scale), int(bool(q_prescaled)), float(drop_p), int(seed) & 0xffffffff, _stream()),
              "tad_attn_bwd")
    return dqkv


def attn_colsum(qkv, lse, w, B: int, N: int, H: int, scale: float, q_prescaled=False, d: int = 64):
    """out[b,h,j] = sum_i w[b,i] * P[b,h,i,j] with P = exp(scale q.k - lse) recomputed from qkv [B*N, 3*H*d] (as attn_fwd takes it) and the
    lse [B,H,N] it is handed; w [B,N] f32 -> out [B,H,N] f32.  No N x N tensor, f32 throughout, bit-reproducible (tad_attn_colsum)"""
    op = _req16(qkv, "attn_colsum.qkv")
    _req(lse, torch.float32, "attn_colsum.lse")
    _req(w, torch.float32, "attn_colsum.w")
    if qkv.numel() != B * N * 3 * H * d:
        raise _lib.TadError(f"attn_colsum: qkv has {qkv.numel()} elements, expected {B * N * 3 * H * d}")
    if lse.numel() != B * H * N or w.numel() != B * N:
        raise _lib.TadError(f"attn_colsum: lse has {lse.numel()} elements and w {w.numel()}, expected {B * H * N} and {B * N}")
    if lse.device != qkv.device or w.device != qkv.device:
        raise _lib.TadError("attn_colsum: qkv, lse and w must live on one device")
    out = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device)
    with _timed("attn_colsum", 2.0 * B * H * N * N * d, 2.0 * 2 * B * N * H * d + 4.0 * (2 * B * H * N + B * N)):
        check(_lib.load().tad_attn_colsum(qkv.data_ptr(), _dt(qkv), lse.data_ptr(), w.data_ptr(), out.data_ptr(), B, N, H, int(d), float(scale),
                                          int(bool(q_prescaled)), _stream()), "tad_attn_colsum")
    return out


# ----------------------------------------------------------------------------- mean-pool
def meanpool_fwd(x):
    _req(x, torch.float32, "meanpool.x")
    B, N, D = x.shape
    y = torch.empty((B, D), dtype=torch.float32, device=x.device)
    ws = workspace(B * _lib.POOL_SPLIT * D * 4, x.device)
    check(_lib.load().tad_meanpool_fwd(x.data_ptr(), y.data_ptr(), ws.data_ptr(), B, N, D, _stream()), "tad_meanpool_fwd")
    return y


def meanpool_bwd(dy, N: int, want_bf16=False):
    _req(dy, torch.float32, "meanpool_bwd.dy")
    B, D = dy.shape
    dx = torch.empty((B, N, D), dtype=torch.float32, device=dy.device)
    dxb = torch.empty((B, N, D), dtype=_op16, device=dy.device) if want_bf16 else None
    check(_fn("tad_meanpool_bwd", _op16)(dy.data_ptr(), dx.data_ptr(), _p(dxb), B, N, D, _stream()), "tad_meanpool_bwd")
    return dx, dxb


# ----------------------------------------------------------------------------- pooled tail (ops.BlockPoolFn)
def colsum_segments_ok(K: int) -> bool:
    """shapes tad_colsum_segments / tad_gelu_grad_bcast take (else: the general path)"""
    return K % 8 == 0


def colsum_segments(a, B: int, N: int):
    """a [B*N, K] 16-bit -> S [B, K] f32, S[b] = sum of the N rows of clip b (f32 accumulation, fixed order)"""
    op = _req16(a, "colsum_segments.a")
    M, Kc = a.shape
    assert M == B * N, (M, B, N)
    S = torch.empty((B, Kc), dtype=torch.float32, device=a.device)
    ws = workspace(B * _lib.POOL_SPLIT * Kc * 4, a.device)
    with _timed("colsum", 0.0, 2.0 * M * Kc):
        check(_lib.load().tad_colsum_segments(a.data_ptr(), _dt(a), S.data_ptr(), ws.data_ptr(), ws.numel(), B, N, Kc, _stream()),
              "tad_colsum_segments")
    return S


def pooled_linear(S, w, bias, rowscale, xbar, N: int):
    """xbar [B, D] + rowscale[b] * ((S [B, K] @ w [D, K]^T) / N + bias): f32 sums times 16-bit weights, f64 accumulation, f32 [B, D]"""
    _req(S, torch.float32, "pooled_linear.S")
    _req(xbar, torch.float32, "pooled_linear.xbar")
    _req16(w, "pooled_linear.w")
    B, Kc = S.shape
    D = w.shape[0]
    assert w.shape[1] == Kc and tuple(xbar.shape) == (B, D), (tuple(S.shape), tuple(w.shape), tuple(xbar.shape))
    for name, t, n in (("bias", bias, D), ("rowscale", rowscale, B)):
        if t is not None:
            _req(t, torch.float32, "pooled_linear." + name)
            assert t.numel() == n, (name, t.numel(), n)
    out = torch.empty((B, D), dtype=torch.float32, device=S.device)
    check(_lib.load().tad_pooled_linear(S.data_ptr(), w.data_ptr(), _dt(w), _p(bias), _p(rowscale), xbar.data_ptr(), out.data_ptr(), B, N, D, Kc,
                                        _stream()), "tad_pooled_linear")
    return out


def gelu_grad_bcast(t, h, N: int):
    """t [B, K] f32 (one accumulator row of the fc2 input gradient per clip), h [B*N, K] 16-bit pre-activations ->
    dh [B*N, K] = op16(t[clip] * gelu'(h)): what linear_bwd_input(..., gelu_preact=h) writes when the N rows of a clip are equal"""
    _req(t, torch.float32, "gelu_grad_bcast.t")
    op = _req16(h, "gelu_grad_bcast.h")
    B, Kc = t.shape
    assert tuple(h.shape) == (B * N, Kc), (tuple(h.shape), B, N, Kc)
    dh = torch.empty((B * N, Kc), dtype=op, device=h.device)
    with _timed("cast", 0.0, 4.0 * B * N * Kc):
        check(_lib.load().tad_gelu_grad_bcast(t.data_ptr(), h.data_ptr(), dh.data_ptr(), _dt(h), B, N, Kc, _stream()), "tad_gelu_grad_bcast")
    return dh


def sumsq(x, out):
    _req(x, torch.float32, "sumsq.x")
    lib = _lib.load()
    ws = workspace(lib.tad_sumsq_workspace_bytes(), x.device)
    check(lib.tad_sumsq_f32(x.data_ptr(), x.numel(), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "tad_sumsq_f32")
    return out


def grad_norm_coef(x, inv_scale: float, max_norm: float = 0.0, out=None):
    """[norm of x with the loss scale removed, grad_scale coefficient for adamw_step (0 = skip: overflow), found-inf flag] as one f32[3]
    device tensor (tad_grad_norm_coef); nothing is read back"""
    _req(x, torch.float32, "grad_norm_coef.x")
    lib = _lib.load()
    if out is None:
        out = torch.empty(3, dtype=torch.float32, device=x.device)
    ws = workspace(lib.tad_sumsq_workspace_bytes(), x.device)
    with _timed("sumsq", 0.0, 4.0 * x.numel()):
        check(lib.tad_grad_norm_coef(x.data_ptr(), x.numel(), float(inv_scale), float(max_norm or 0.0), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                     _stream()), "tad_grad_norm_coef")
    return out


# ----------------------------------------------------------------------------- per-head gradient norms: segmented sum of squares
def _segnorm_dtypes():
    import numpy as np
    return (np.dtype([("offset", "<i8"), ("length", "<i8"), ("slot", "<i4"), ("first_work", "<i4")]),   # tad_segnorm_seg, 24 bytes
            np.dtype([("offset", "<i8"), ("length", "<i8")]))                                           # tad_segnorm_work, 16 bytes


def grad_segnorm_plan_check(table, work, n: int, nslots: int) -> None:
    """tad_grad_segnorm_plan_check on HOST copies of the two tables (int64 CPU tensors [nseg,3] / [nwork,2]); runs without a GPU"""
    for t, words, name in ((table, 3, "table"), (work, 2, "work")):
        if t.device.type != "cpu" or t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != words or not t.is_contiguous():
            raise _lib.TadError(f"grad_segnorm_plan_check.{name}: expected a contiguous int64 CPU tensor [rows,{words}], got "
                                f"{t.dtype}{list(t.shape)} on {t.device}")
    check(_lib.load().tad_grad_segnorm_plan_check(table.data_ptr(), table.shape[0], work.data_ptr(), work.shape[0], int(n), int(nslots)),
          "tad_grad_segnorm_plan_check")


def grad_segnorm_tables(segments, n: int, nslots: int):
    """Host-side tables of grad_segnorm (include/tad_mi355x.h): ``segments`` = (offset, length, slot) triples over a flat buffer of
    ``n`` floats.  Every segment is cut, in order, into work items of at most SEGNORM_WORK_MAX floats.  Returns the int64 CPU tensors
    (table [nseg,3] = the 24-byte rows {offset, length, slot | first_work}, work [nwork,2]), checked by tad_grad_segnorm_plan_check.
    Built once per model; nothing is built per step."""
    import numpy as np
    seg_t, work_t = _segnorm_dtypes()
    segments = [(int(o), int(ln), int(s)) for o, ln, s in segments]
    if not segments:
        raise _lib.TadError("grad_segnorm_tables: no segments")
    big = 2 ** 31
    if any(not (-big <= s < big) for _, _, s in segments):
        raise _lib.TadError("grad_segnorm_tables: a slot does not fit 32 bits")
    mx = _lib.SEGNORM_WORK_MAX
    tab = np.zeros(len(segments), dtype=seg_t)
    items = []
    for k, (o, ln, s) in enumerate(segments):
        tab[k] = (o, ln, s, len(items))
        items.extend((o + a, min(mx, ln - a)) for a in range(0, max(ln, 0), mx))
        if len(items) >= big:
            raise _lib.TadError("grad_segnorm_tables: too many work items")
    wk = np.array(items, dtype=work_t) if items else np.zeros(0, dtype=work_t)
    table = torch.from_numpy(tab.view(np.int64).reshape(len(segments), 3).copy())
    work = torch.from_numpy(wk.view(np.int64).reshape(len(items), 2).copy())
    grad_segnorm_plan_check(table, work, n, nslots)
    return table, work


def grad_segnorm(grad, table, work, acc, last, counters, coef=None):
    """One collect (tad_grad_segnorm: a reduce and a finish launch, no host synchronisation): for every segment of the device tables
    ``table`` / ``work`` (copies of grad_segnorm_tables()'s) ``last[slot] = coef * ||grad[segment]||`` and ``acc[slot] += last[slot]``;
    ``coef`` = a device f32 tensor of one element or None (1.0).  ``counters`` int32 [3] = {steps_added, steps_skipped,
    nonfinite_values}.  The tables are not re-checked here: grad_segnorm_tables() checked them when they were created."""
    _req(grad, torch.float32, "grad_segnorm.grad")
    _req(table, torch.int64, "grad_segnorm.table")
    _req(work, torch.int64, "grad_segnorm.work")
    _req(acc, torch.float64, "grad_segnorm.acc")
    _req(last, torch.float32, "grad_segnorm.last")
    _req(counters, torch.int32, "grad_segnorm.counters")
    if table.dim() != 2 or table.shape[1] != 3 or work.dim() != 2 or work.shape[1] != 2 or table.shape[0] == 0:
        raise _lib.TadError(f"grad_segnorm: expected the device copies of grad_segnorm_tables(), got {list(table.shape)} and {list(work.shape)}")
    if acc.numel() != last.numel() or counters.numel() != 3:
        raise _lib.TadError(f"grad_segnorm: acc [{acc.numel()}] and last [{last.numel()}] must have one entry per slot, counters [3]")
    if coef is not None:
        _req(coef, torch.float32, "grad_segnorm.coef")
        if coef.numel() != 1:
            raise _lib.TadError(f"grad_segnorm.coef: expected one f32 on the device, got {list(coef.shape)}")
    if any(t.device != grad.device for t in (table, work, acc, last, counters) + (() if coef is None else (coef,))):
        raise _lib.TadError("grad_segnorm: every operand must live on the gradient buffer's device")
    lib = _lib.load()
    nwork = work.shape[0]
    ws = workspace(lib.tad_grad_segnorm_workspace_bytes(nwork), grad.device)
    with _timed("grad_segnorm", 0.0, 4.0 * grad.numel()):
        check(lib.tad_grad_segnorm(grad.data_ptr(), grad.numel(), table.data_ptr(), table.shape[0], work.data_ptr(), nwork, _p(coef),
                                   acc.data_ptr(), last.data_ptr(), counters.data_ptr(), acc.numel(), ws.data_ptr(), ws.numel(), _stream()),
              "tad_grad_segnorm")
    return last


def adamw_step(param, grad, exp_avg, exp_avg_sq, chunk_group, group_lr, group_wd, group_step, beta1, beta2, eps, param_bf16=None,
               grad_scale=None, sumsq_partials=None):
    """Fused AdamW over flat f32 buffers (tad_adamw_step); group_lr / group_wd / group_step are host sequences, one entry per
    parameter group (group_step: 1-based update count of the group's tensors after this call)."""
    for t, nm in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _req(t, torch.float32, "adamw." + nm)
    n = param.numel()
    if not (grad.numel() == n and exp_avg.numel() == n and exp_avg_sq.numel() == n):
        raise _lib.TadError("adamw_step: flat buffers differ in length")
    chunks = (n + _lib.ADAMW_CHUNK - 1) // _lib.ADAMW_CHUNK
    if chunk_group.dtype != torch.uint8 or chunk_group.numel() != chunks or not chunk_group.is_cuda:
        raise _lib.TadError(f"adamw_step: chunk_group must be a uint8 device tensor with {chunks} entries")
    op = torch.bfloat16
    if param_bf16 is not None:
        op = _req16(param_bf16, "adamw.param_bf16")
        assert param_bf16.numel() == n
    if sumsq_partials is not None:
        _req(sumsq_partials, torch.float32, "adamw.sumsq_partials")
        assert sumsq_partials.numel() == chunks
    if grad_scale is not None:
        _req(grad_scale, torch.float32, "adamw.grad_scale")
    ng = len(group_lr)
    assert len(group_wd) == ng and len(group_step) == ng
    lr = (C.c_float * ng)(*[float(v) for v in group_lr])
    wd = (C.c_float * ng)(*[float(v) for v in group_wd])
    st = (C.c_int32 * ng)(*[int(v) for v in group_step])
    with _timed("adamw", 0.0, 30.0 * n):
        check(_fn("tad_adamw_step", op)(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), _p(param_bf16),
                                         chunk_group.data_ptr(), n, lr, wd, ng, st, float(beta1), float(beta2), float(eps),
                                         _p(grad_scale), _p(sumsq_partials), _stream()), "tad_adamw_step")


def ema_table(pairs):
    """Host-side tables of ema_update: pairs = [(ema address, model address, numel)] of f32 tensors.  Returns (tensors int64
    [n_tensors, 4], chunks int32 [n_chunks, 2]) as ONE int64 CPU tensor (tensors first, chunks behind them) and the two counts.
    A pair whose addresses are misaligned by the same amount is split into a scalar head of up to 3 elements and a 16-byte aligned
    body, so that a view starting at an odd element still takes the float4 path."""
    rows = []
    for e, m, n in pairs:
        if n <= 0:
            continue
        if e % 4 or m % 4:
            raise _lib.TadError("ema_table: f32 tensors must be 4-byte aligned")
        h = ((16 - e % 16) % 16) // 4 if e % 16 == m % 16 else 0
        h = min(h, n)
        if h:
            rows.append((e, m, h, 0))
        if n > h:
            rows.append((e + 4 * h, m + 4 * h, n - h, 0))
    if not rows:
        raise _lib.TadError("ema_table: no elements")
    chunks = [(t, c) for t, r in enumerate(rows) for c in range((r[2] + _lib.EMA_CHUNK - 1) // _lib.EMA_CHUNK)]
    import numpy as np
    tens = np.asarray(rows, dtype=np.uint64).view(np.int64).reshape(-1)
    chk = np.asarray(chunks, dtype=np.int32).reshape(-1)
    if len(chunks) >= (1 << 31):
        raise _lib.TadError("ema_table: too many chunks")
    return torch.from_numpy(np.concatenate([tens, chk.view(np.int64)])), len(rows), len(chunks)


def ema_update(table, n_tensors: int, n_chunks: int, decay: float, n_elements: int = 0):
    """ema = ema * decay + (1 - decay) * model over every pair of ``table`` (a device copy of ema_table's buffer), ONE launch
    (tad_ema_update).  ``1 - decay`` is taken in double here, as the reference's Python expression does."""
    if not table.is_cuda or table.dtype != torch.int64 or not table.is_contiguous() or table.numel() != 4 * n_tensors + n_chunks:
        raise _lib.TadError("ema_update: table must be the contiguous int64 device copy of ema_table()")
    d = float(decay)
    with _timed("ema", 0.0, 12.0 * n_elements):
        check(_lib.load().tad_ema_update(table.data_ptr(), n_tensors, table.data_ptr() + 32 * n_tensors, n_chunks, d, 1.0 - d, _stream()),
              "tad_ema_update")


# ----------------------------------------------------------------------------- Mixup / CutMix and the soft-target loss
def mixup_plan_table(rows, T: int, H: int, W: int):
    """Host-side plan table of mixup_clips / mixup_target: rows = one (kind, w_self, w_other, (t0, t1, y0, y1, x0, x1), lam,
    one_minus_lam) per sample, coefficients already rounded to f32 by the caller.  Returns the int32 CPU tensor [B, MIXUP_PLAN_WORDS],
    checked by tad_mixup_plan_check (kinds, finite coefficients, boxes inside the clip, even B); runs without a GPU."""
    import numpy as np
    tab = np.zeros((len(rows), _lib.MIXUP_PLAN_WORDS), dtype=np.int32)
    fl = tab.view(np.float32)
    for s, (kind, w_self, w_other, box, lam, oml) in enumerate(rows):
        tab[s, 0] = kind
        fl[s, 1], fl[s, 2] = w_self, w_other
        tab[s, 3:9] = box
        fl[s, 9], fl[s, 10] = lam, oml
    check(_lib.load().tad_mixup_plan_check(tab.ctypes.data, len(rows), T, H, W), "tad_mixup_plan_check")
    return torch.from_numpy(tab)


def _req_plan(plan, B, name):
    _req(plan, torch.int32, name)
    if tuple(plan.shape) != (B, _lib.MIXUP_PLAN_WORDS):
        raise _lib.TadError(f"{name}: expected the device copy of mixup_plan_table() for {B} samples, got {tuple(plan.shape)}")


def mixup_clips(x, plan):
    """Mix the contiguous f32 clip batch x [B,C,T,H,W] IN PLACE as the device plan table says (tad_mixup_clips, ONE launch, no
    temporary); returns x.  The caller bumps x's version counter if autograd is to see the write."""
    _req(x, torch.float32, "mixup_clips.x")
    if x.dim() != 5:
        raise _lib.TadError(f"mixup_clips.x: expected [B,C,T,H,W], got {tuple(x.shape)}")
    B, Cc, T, H, W = x.shape
    _req_plan(plan, B, "mixup_clips.plan")
    with _timed("mixup", 0.0, 8.0 * x.numel()):
        check(_lib.load().tad_mixup_clips(x.data_ptr(), plan.data_ptr(), B, Cc, T, H, W, _stream()), "tad_mixup_clips")
    return x


def mixup_target(plan, labels, num_classes: int, on_value: float, off_value: float):
    """the soft targets [B, num_classes] f32 of the plan's per-sample lam (tad_mixup_target); labels int64 [B] on the device"""
    _req(labels, torch.int64, "mixup_target.labels")
    B = labels.numel()
    _req_plan(plan, B, "mixup_target.plan")
    out = torch.empty((B, int(num_classes)), dtype=torch.float32, device=labels.device)
    check(_lib.load().tad_mixup_target(plan.data_ptr(), labels.data_ptr(), out.data_ptr(), B, int(num_classes), float(on_value),
                                       float(off_value), _stream()), "tad_mixup_target")
    return out


def erase_box_table(boxes, B: int, T: int, H: int, W: int):
    """Host-side box table of erase_clips: boxes = one (sample, mode, t0, t1, y0, y1, x0, x1) per box, in the order the reference
    writes them (where boxes of a sample overlap the last one wins).  Returns the int32 CPU tensor [n, ERASE_BOX_WORDS], checked by
    tad_erase_plan_check (modes, samples inside the batch, boxes inside the clip); runs without a GPU."""
    import numpy as np
    tab = np.zeros((len(boxes), _lib.ERASE_BOX_WORDS), dtype=np.int32)
    for k, row in enumerate(boxes):
        tab[k, :8] = row
    if len(boxes):
        check(_lib.load().tad_erase_plan_check(tab.ctypes.data, len(boxes), B, T, H, W), "tad_erase_plan_check")
    return torch.from_numpy(tab)


def erase_clips(x, boxes, seed: int):
    """Erase the boxes of the device table ``boxes`` (a copy of erase_box_table()) from the contiguous f32 clip batch x [B,C,T,H,W] IN
    PLACE (tad_erase_clips, ONE launch that only stores); ``seed`` keys the counter-based noise (include/tad_mi355x.h).  Returns x; an
    empty table launches nothing.  The caller bumps x's version counter if autograd is to see the write."""
    _req(x, torch.float32, "erase_clips.x")
    if x.dim() != 5:
        raise _lib.TadError(f"erase_clips.x: expected [B,C,T,H,W], got {tuple(x.shape)}")
    _req(boxes, torch.int32, "erase_clips.boxes")
    if boxes.dim() != 2 or boxes.shape[1] != _lib.ERASE_BOX_WORDS:
        raise _lib.TadError(f"erase_clips.boxes: expected the device copy of erase_box_table(), got {tuple(boxes.shape)}")
    B, Cc, T, H, W = x.shape
    n = boxes.shape[0]
    if n == 0:
        return x
    with _timed("erase", 0.0, 0.0):
        check(_lib.load().tad_erase_clips(x.data_ptr(), boxes.data_ptr(), n, int(seed) & 0xffffffff, B, Cc, T, H, W, _stream()),
              "tad_erase_clips")
    return x


# ----------------------------------------------------------------------------- RandAugment on uint8 frames
def randaug_table(layers, B: int, T: int):
    """Host-side table of randaug_apply: ``layers`` = per layer one row per clip, (sample, op, iarg, farg, coefficients (six Python
    floats) or None, fill (r, g, b), bicubic mask (bit t: frame t is resampled BICUBIC)).  Returns (int32 CPU tensor
    [n_layers, B, RANDAUG_ROW_WORDS], bit mask of the layers that need per-frame statistics), checked by tad_randaug_plan_check (known
    ops, every sample once per layer, argument ranges, finite values); runs without a GPU."""
    import numpy as np
    tab = np.zeros((len(layers), B, _lib.RANDAUG_ROW_WORDS), dtype=np.int32)
    stats = 0
    for l, rows in enumerate(layers):
        if len(rows) != B:
            raise _lib.TadError(f"randaug_table: layer {l} has {len(rows)} rows for a batch of {B} clips")
        for k, (sample, op, iarg, farg, coefs, fill, bicubic) in enumerate(rows):
            row = tab[l, k]
            row[0], row[1], row[2] = sample, op, iarg
            u = row.view(np.uint32)
            u[3] = (int(fill[0]) & 255) | (int(fill[1]) & 255) << 8 | (int(fill[2]) & 255) << 16
            u[4], u[5] = int(bicubic) & 0xffffffff, (int(bicubic) >> 32) & 0xffffffff
            row.view(np.float32)[6] = farg
            if coefs is not None:
                row[8:20] = np.asarray(coefs, dtype=np.float64).view(np.int32)
            if op in _lib.RA_STATS_OPS:
                stats |= 1 << l
    check(_lib.load().tad_randaug_plan_check(tab.ctypes.data, tab.size, len(layers), B, T), "tad_randaug_plan_check")
    return torch.from_numpy(tab), stats


def _req_frames(x, name):
    _req(x, torch.uint8, name)
    if x.dim() != 5 or x.shape[-1] != 3 or x.numel() == 0:
        raise _lib.TadError(f"{name}: expected uint8 frames [B,T,H,W,3], got {tuple(x.shape)}")


def _clip_out(name, out, shape, dtype, device):
    """The output of a frame kernel: a new tensor of ``shape``, or the caller's ``out`` (any contiguous view: a ring slot, a slice of
    a frame store) held to that shape, ``dtype`` and device."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _req(out, dtype, f"{name}.out")
    if tuple(out.shape) != shape or out.device != device:
        raise _lib.TadError(f"{name}.out: expected {shape} on {device}, got {tuple(out.shape)} on {out.device}")
    return out


def _norm_pair(name, mean, std):
    """(mean, std) as the C entry points take them, (None, None) without them; one without the other is an error"""
    if (mean is None) != (std is None):
        raise _lib.TadError(f"{name}: mean and std come together")
    return (None, None) if mean is None else (_f3(mean), _f3(std))


def _req_table(name, table, shape, nbytes, what, device):
    """``table`` is the device copy of ``name``_table()'s tensor: int32 words of ``shape``, the ``nbytes`` bytes of the call's
    workspace, on the device of its frames"""
    _req(table, torch.int32, f"{name}.table")
    if tuple(table.shape) != shape or nbytes == 0 or table.device != device:
        raise _lib.TadError(f"{name}.table: expected the device copy of {name}_table() for {what}, got {tuple(table.shape)} on {table.device}")


def randaug_apply(x, table, stats_layers: int):
    """Carry the device table ``table`` (a copy of randaug_table()'s, [n_layers, B, RANDAUG_ROW_WORDS]) out on the contiguous uint8
    frames x [B,T,H,W,3] (tad_randaug_apply: per layer one apply launch, plus one statistics launch where ``stats_layers`` has the
    layer's bit).  Returns a new tensor; x is only read."""
    _req_frames(x, "randaug_apply.x")
    B, T, H, W, _ = x.shape
    _req(table, torch.int32, "randaug_apply.table")
    if table.dim() != 3 or tuple(table.shape[1:]) != (B, _lib.RANDAUG_ROW_WORDS):
        raise _lib.TadError(f"randaug_apply.table: expected the device copy of randaug_table() for {B} clips, got {tuple(table.shape)}")
    L = table.shape[0]
    lib = _lib.load()
    out = torch.empty_like(x)
    nbytes = lib.tad_randaug_workspace_bytes(L, B, T, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    with _timed("randaug", 0.0, 2.0 * L * x.numel()):
        check(lib.tad_randaug_apply(x.data_ptr(), out.data_ptr(), table.data_ptr() if L else None, L, int(stats_layers) & 0xffffffff,
                                    ws.data_ptr(), nbytes, B, T, H, W, _stream()), "tad_randaug_apply")
    return out


def frames_to_clip(x, mean, std, out=None):
    """f32 clips [B,3,T,H,W] = ((float)x / 255 - mean[c]) / std[c] of the contiguous uint8 frames x [B,T,H,W,3] (tad_frames_to_clip,
    ONE launch; IEEE division): torchvision's ToTensor, the reference's tensor_normalize and its permute, bit for bit."""
    _req_frames(x, "frames_to_clip.x")
    B, T, H, W, _ = x.shape
    out = _clip_out("frames_to_clip", out, (B, 3, T, H, W), torch.float32, x.device)
    with _timed("frames_to_clip", 0.0, 13.0 * B * T * H * W):
        check(_lib.load().tad_frames_to_clip(x.data_ptr(), out.data_ptr(), _f3(mean), _f3(std), B, T, H, W, _stream()), "tad_frames_to_clip")
    return out


# ----------------------------------------------------------------------------- multi-scale crop + PIL BILINEAR resize of uint8 frames
def multiscale_crop_table(rows, hsets, vsets, B: int, Hs: int, Ws: int, S_h: int, S_w: int):
    """Host-side table of multiscale_crop (include/tad_mi355x.h): ``rows`` = one (sample, x0, y0, w, h, hset, vset) per clip;
    ``hsets`` / ``vsets`` = coefficient sets (in, ksize, bounds [out][2], kk [out][ksize]) towards S_w / S_h outputs.  Returns the
    int32 CPU tensor of tad_multiscale_crop_workspace_bytes / 4 words, checked by tad_multiscale_crop_plan_check (word counts, every
    sample once, crops inside the source, counts <= ksize <= 17, set indices in range); runs without a GPU."""
    import numpy as np
    lib = _lib.load()
    nh, nv = len(hsets), len(vsets)
    if len(rows) != B or not (1 <= nh <= _lib.MSC_MAX_SETS and 1 <= nv <= _lib.MSC_MAX_SETS):
        raise _lib.TadError(f"multiscale_crop_table: {len(rows)} rows for {B} clips, {nh} horizontal and {nv} vertical sets "
                            f"(1 .. {_lib.MSC_MAX_SETS} each)")
    tab = np.zeros(lib.tad_multiscale_crop_workspace_bytes(B, nh, nv, S_h, S_w) // 4, dtype=np.int32)
    tab[:B * _lib.MSC_ROW_WORDS].reshape(B, _lib.MSC_ROW_WORDS)[:, :7] = np.asarray(rows, dtype=np.int64).reshape(B, 7)
    at = B * _lib.MSC_ROW_WORDS
    for sets, out in ((hsets, S_w), (vsets, S_h)):
        slot = _lib.MSC_SET_HEAD + out * (2 + _lib.MSC_MAX_KSIZE)
        for n_in, ksize, bounds, kk in sets:
            bounds, kk = np.asarray(bounds, dtype=np.int32), np.asarray(kk, dtype=np.int32)
            if not 1 <= ksize <= _lib.MSC_MAX_KSIZE or bounds.shape != (out, 2) or kk.shape != (out, ksize):
                raise _lib.TadError(f"multiscale_crop_table: a set of ksize {ksize} (1 .. {_lib.MSC_MAX_KSIZE}) with bounds "
                                    f"{bounds.shape} and kk {kk.shape} for {out} outputs")
            tab[at:at + 3] = n_in, out, ksize
            tab[at + _lib.MSC_SET_HEAD:at + _lib.MSC_SET_HEAD + 2 * out] = bounds.reshape(-1)
            tab[at + _lib.MSC_SET_HEAD + 2 * out:at + _lib.MSC_SET_HEAD + (2 + ksize) * out] = kk.reshape(-1)
            at += slot
    check(lib.tad_multiscale_crop_plan_check(tab.ctypes.data, tab.size, B, nh, nv, Hs, Ws, S_h, S_w), "tad_multiscale_crop_plan_check")
    return torch.from_numpy(tab)


def multiscale_crop(x, table, n_hsets: int, n_vsets: int, S_h: int, S_w: int, mean=None, std=None, out=None):
    """Crop and resize the contiguous uint8 frames x [B,T,Hs,Ws,3] as the device table ``table`` (a copy of multiscale_crop_table()'s:
    the call's workspace, only read) says (tad_multiscale_crop, ONE launch).  Without ``mean`` / ``std``: uint8 [B,T,S_h,S_w,3];
    with them: the normalised f32 clips [B,3,T,S_h,S_w], the bits frames_to_clip gives on the uint8 result.  x is only read."""
    _req_frames(x, "multiscale_crop.x")
    B, T, Hs, Ws, _ = x.shape
    lib = _lib.load()
    nbytes = lib.tad_multiscale_crop_workspace_bytes(B, n_hsets, n_vsets, S_h, S_w)
    _req_table("multiscale_crop", table, (nbytes // 4,), nbytes, f"{B} clips ({nbytes} bytes)", x.device)
    m, s = _norm_pair("multiscale_crop", mean, std)
    f32 = m is not None
    out = _clip_out("multiscale_crop", out, (B, 3, T, S_h, S_w) if f32 else (B, T, S_h, S_w, 3), torch.float32 if f32 else torch.uint8, x.device)
    with _timed("multiscale_crop", 0.0, float(x.numel() + out.numel() * out.element_size())):
        check(lib.tad_multiscale_crop(x.data_ptr(), out.data_ptr(), int(f32), m, s, table.data_ptr(), nbytes, B, T, Hs, Ws, S_h, S_w,
                                      n_hsets, n_vsets, _stream()), "tad_multiscale_crop")
    return out


# ----------------------------------------------------------------------------- the loader's cubic resize of uint8 frames, behind pad_wide_clips
def _write_cubic_sets(who: str, tab, at: int, groups) -> int:
    """The cubic sets of ``groups`` = ((sets, out), ...), each set (in, first [out], k [out][4]), into the int32 table ``tab`` from word
    ``at``, back to back as csrc/cubic_resize.h lays them out: {in, out, 0, 0}, first, k.  Returns the word behind the last one."""
    import numpy as np
    for sets, out in groups:
        for n_in, first, kk in sets:
            first, kk = np.asarray(first, dtype=np.int32), np.asarray(kk, dtype=np.int32)
            if first.shape != (out,) or kk.shape != (out, 4):
                raise _lib.TadError(f"{who}: a set with first {first.shape} and k {kk.shape} for {out} outputs")
            tab[at:at + 2] = n_in, out
            tab[at + _lib.FR_SET_HEAD:at + _lib.FR_SET_HEAD + out] = first
            tab[at + _lib.FR_SET_HEAD + out:at + _lib.FR_SET_HEAD + 5 * out] = kk.reshape(-1)
            at += _lib.FR_SET_HEAD + 5 * out
    return at


def frame_resize_table(rows, hset, vsets, B: int, H: int, W: int, S_h: int, S_w: int):
    """Host-side table of frame_resize (include/tad_mi355x.h): ``rows`` = one (sample, mode, pad_top, pad_bottom, alpha, colour, vset)
    per clip, alpha a float and colour three bytes (one per stored channel); ``hset`` = (in, first [S_w], k [S_w][4]) and ``vsets`` =
    such sets towards S_h outputs, one per distinct virtual height.  Returns the int32 CPU tensor of tad_frame_resize_workspace_bytes
    / 4 words, checked by tad_frame_resize_plan_check (word count, every sample once, pads within H, sets stated for the extents
    they serve, taps next to their source, sum |k| <= 2818); runs without a GPU."""
    import numpy as np
    lib = _lib.load()
    nv = len(vsets)
    if len(rows) != B or not 1 <= nv <= _lib.FR_MAX_SETS:
        raise _lib.TadError(f"frame_resize_table: {len(rows)} rows for {B} clips, {nv} vertical sets (1 .. {_lib.FR_MAX_SETS})")
    tab = np.zeros(lib.tad_frame_resize_workspace_bytes(B, nv, S_h, S_w) // 4, dtype=np.int32)
    head = tab[:B * _lib.FR_ROW_WORDS].reshape(B, _lib.FR_ROW_WORDS)
    for i, (sample, mode, pad_top, pad_bottom, alpha, colour, vset) in enumerate(rows):
        c = [int(v) for v in colour]
        if len(c) != 3 or not all(0 <= v <= 255 for v in c):
            raise _lib.TadError(f"frame_resize_table: row {i}: colour {colour!r} must hold three bytes")
        words = [int(sample), int(mode), int(pad_top), int(pad_bottom), int(np.float32(alpha).view(np.int32)), c[0] | c[1] << 8 | c[2] << 16, int(vset)]
        if any(abs(w) >= 2 ** 31 for w in words):
            raise _lib.TadError(f"frame_resize_table: row {i} does not fit 32 bits")
        head[i, :7] = words
    _write_cubic_sets("frame_resize_table", tab, B * _lib.FR_ROW_WORDS, (([hset], S_w), (vsets, S_h)))
    check(lib.tad_frame_resize_plan_check(tab.ctypes.data, tab.size, B, nv, H, W, S_h, S_w), "tad_frame_resize_plan_check")
    return torch.from_numpy(tab)


def frame_resize(x, table, n_vsets: int, S_h: int, S_w: int, mean=None, std=None, out=None):
    """Resize (cubic, behind the virtual pad bands the table states) the contiguous uint8 frames x [B,T,H,W,3] as the device table
    ``table`` (a copy of frame_resize_table()'s: the call's workspace, only read) says (tad_frame_resize, ONE launch).  Without
    ``mean`` / ``std``: uint8 [B,T,S_h,S_w,3]; with them: the normalised f32 clips [B,3,T,S_h,S_w], the bits frames_to_clip gives on
    the uint8 result.  ``out`` may be any contiguous view of that shape (a ring slot, a slice of a frame store).  x is only read."""
    _req_frames(x, "frame_resize.x")
    B, T, H, W, _ = x.shape
    lib = _lib.load()
    nbytes = lib.tad_frame_resize_workspace_bytes(B, n_vsets, S_h, S_w)
    _req_table("frame_resize", table, (nbytes // 4,), nbytes, f"{B} clips ({nbytes} bytes)", x.device)
    m, s = _norm_pair("frame_resize", mean, std)
    f32 = m is not None
    out = _clip_out("frame_resize", out, (B, 3, T, S_h, S_w) if f32 else (B, T, S_h, S_w, 3), torch.float32 if f32 else torch.uint8, x.device)
    with _timed("frame_resize", 0.0, float(x.numel() + out.numel() * out.element_size())):
        check(lib.tad_frame_resize(x.data_ptr(), out.data_ptr(), int(f32), m, s, table.data_ptr(), nbytes, B, T, H, W, S_h, S_w, n_vsets,
                                   _stream()), "tad_frame_resize")
    return out


# ----------------------------------------------------------------------------- ragged ingest: K frames of K sizes into K slots of a frame store
def ingest_table(rows, hsets, vsets, src_bytes: int, F: int, S_h: int, S_w: int):
    """Host-side table of ingest_frames (include/tad_mi355x_bank.h): ``rows`` = one (src_off, h, w, slot, hset, vset, flags) per frame;
    ``hsets`` / ``vsets`` = [(in, first [out], k [out][4])] towards S_w / S_h outputs, one per distinct width / height
    (``frame_resize.cubic_coeffs``).  Returns the int32 CPU tensor, checked by tadb_ingest_plan_check (word count, frames inside
    ``src_bytes`` at multiples of 4, every slot inside [0, F) and named once, sets stated for the extents they serve, taps next to their
    source, sum |k| <= 2818, known flags); runs without a GPU."""
    import numpy as np
    lib = _lib.load_bank()
    K, nh, nv = len(rows), len(hsets), len(vsets)
    if not (1 <= K <= _lib.BANK_MAX_FRAMES and 1 <= nh <= _lib.BANK_MAX_SETS and 1 <= nv <= _lib.BANK_MAX_SETS):
        raise _lib.TadError(f"ingest_table: {K} frames (1 .. {_lib.BANK_MAX_FRAMES}), {nh} horizontal and {nv} vertical sets (1 .. {_lib.BANK_MAX_SETS} each)")
    if int(S_h) < 1 or int(S_w) < 1:
        raise _lib.TadError(f"ingest_table: S_h={S_h} S_w={S_w} must be positive")
    tab = np.zeros(K * _lib.BANK_ROW_WORDS + nh * (_lib.FR_SET_HEAD + 5 * S_w) + nv * (_lib.FR_SET_HEAD + 5 * S_h), dtype=np.int32)
    r = np.asarray(rows, dtype=np.int64).reshape(K, 7)
    if (np.abs(r) >= 2 ** 31).any():
        raise _lib.TadError("ingest_table: a row does not fit 32 bits")
    tab[:K * _lib.BANK_ROW_WORDS].reshape(K, _lib.BANK_ROW_WORDS)[:, :7] = r
    _write_cubic_sets("ingest_table", tab, K * _lib.BANK_ROW_WORDS, ((hsets, S_w), (vsets, S_h)))
    _lib.check_bank(lib.tadb_ingest_plan_check(tab.ctypes.data, tab.size, K, nh, nv, int(src_bytes), int(F), int(S_h), int(S_w)),
                    "tadb_ingest_plan_check")
    return torch.from_numpy(tab)


def _ingest_args(who: str, src, src_bytes: int, store, table):
    """the tensors of a ragged ingest launch; returns the store's (F, S_h, S_w)"""
    _req(src, torch.uint8, f"{who}.src")
    _req(store, torch.uint8, f"{who}.store")
    _req(table, torch.int32, f"{who}.table")
    if store.dim() != 4 or store.shape[-1] != 3 or store.numel() == 0:
        raise _lib.TadError(f"{who}.store: expected a uint8 frame store [F,S_h,S_w,3], got {tuple(store.shape)}")
    if src.dim() != 1 or table.dim() != 1 or src.device != store.device or table.device != store.device:
        raise _lib.TadError(f"{who}: src and table must be 1-D tensors on {store.device}")
    if int(src_bytes) < 1 or src.numel() < (int(src_bytes) + 3) // 4 * 4:
        raise _lib.TadError(f"{who}.src: {src.numel()} bytes do not hold src_bytes={src_bytes} rounded up to a multiple of 4")
    return store.shape[:3]


def ingest_frames(src, src_bytes: int, store, table, K: int, n_hsets: int, n_vsets: int):
    """Resize the K packed uint8 frames of ``src`` (1-D uint8 on the GPU; frame k is [h_k, w_k, 3] at the multiple of 4 its row of the
    table names) to the store's S_h x S_w and write each to the slot its row names, as the device table ``table`` (a copy of
    ingest_table()'s) says: tadb_ingest_frames, ONE launch for frames of any mix of sizes.  ``src`` must hold ``src_bytes`` rounded up to a
    multiple of 4 (pixels come in as the aligned words that hold them).  store: contiguous uint8 [F,S_h,S_w,3], written in the named slots
    only.  Returns store."""
    F, S_h, S_w = _ingest_args("ingest_frames", src, src_bytes, store, table)
    with _timed("ingest_frames", 0.0, float(src_bytes + K * S_h * S_w * 3)):
        _lib.check_bank(_lib.load_bank().tadb_ingest_frames(src.data_ptr(), int(src_bytes), store.data_ptr(), F, table.data_ptr(), table.numel(),
                                                            int(K), int(n_hsets), int(n_vsets), S_h, S_w, _stream()), "tadb_ingest_frames")
    return store


def ingest_yuv_table(rows, hsets, vsets, csets, src_bytes: int, F: int, S_h: int, S_w: int):
    """Host-side table of ingest_yuv (include/tad_mi355x_yuv.h): ``rows`` = one (y_off, y_pitch, u_off, v_off, c_pitch, c_step, h, w,
    slot, hset, vset, cset, flags) per frame; ``hsets`` / ``vsets`` as for ingest_table; ``csets`` = [(y_off, cy, cvr, cug, cvg, cub)]
    (``stream_bank.colour_set``).  Returns the int32 CPU tensor, checked by tady_ingest_plan_check (word count, every plane inside
    ``src_bytes`` with pitches that hold its rows, every slot inside [0, F) and named once, sets stated for the extents they serve, taps
    next to their source, sum |k| <= 2818, colour sets inside the int32 bound, known flags); runs without a GPU."""
    import numpy as np
    lib = _lib.load_yuv()
    K, nh, nv, nc = len(rows), len(hsets), len(vsets), len(csets)
    if not (1 <= K <= _lib.YUV_MAX_FRAMES and 1 <= nh <= _lib.YUV_MAX_SETS and 1 <= nv <= _lib.YUV_MAX_SETS and 1 <= nc <= _lib.YUV_MAX_CSETS):
        raise _lib.TadError(f"ingest_yuv_table: {K} frames (1 .. {_lib.YUV_MAX_FRAMES}), {nh} horizontal and {nv} vertical sets (1 .. {_lib.YUV_MAX_SETS} each), "
                            f"{nc} colour sets (1 .. {_lib.YUV_MAX_CSETS})")
    if int(S_h) < 1 or int(S_w) < 1:
        raise _lib.TadError(f"ingest_yuv_table: S_h={S_h} S_w={S_w} must be positive")
    R = _lib.YUV_ROW_WORDS
    tab = np.zeros(K * R + nh * (_lib.FR_SET_HEAD + 5 * S_w) + nv * (_lib.FR_SET_HEAD + 5 * S_h) + nc * _lib.YUV_CSET_WORDS, dtype=np.int32)
    r = np.asarray(rows, dtype=np.int64).reshape(K, 13)
    c = np.asarray(csets, dtype=np.int64).reshape(nc, 6)
    if (np.abs(r) >= 2 ** 31).any() or (np.abs(c) >= 2 ** 31).any():
        raise _lib.TadError("ingest_yuv_table: a row or a colour set does not fit 32 bits")
    tab[:K * R].reshape(K, R)[:, :13] = r
    at = _write_cubic_sets("ingest_yuv_table", tab, K * R, ((hsets, S_w), (vsets, S_h)))
    tab[at:].reshape(nc, _lib.YUV_CSET_WORDS)[:, :6] = c
    _lib.check_yuv(lib.tady_ingest_plan_check(tab.ctypes.data, tab.size, K, nh, nv, nc, int(src_bytes), int(F), int(S_h), int(S_w)),
                   "tady_ingest_plan_check")
    return torch.from_numpy(tab)


def ingest_yuv(src, src_bytes: int, store, table, K: int, n_hsets: int, n_vsets: int, n_csets: int):
    """Convert the K packed 4:2:0 YUV frames of ``src`` (1-D uint8 on the GPU; the planes of frame k lie where its row of the table
    says) to 8-bit RGB by the table's colour sets, resize each to the store's S_h x S_w and write it to the slot its row names, as the
    device table ``table`` (a copy of ingest_yuv_table()'s) says: tady_ingest_yuv, ONE launch for frames of any mix of sizes and
    layouts.  ``src`` must hold ``src_bytes`` rounded up to a multiple of 4 (samples come in as the aligned words that hold them).
    store: contiguous uint8 [F,S_h,S_w,3], written in the named slots only.  Returns store."""
    F, S_h, S_w = _ingest_args("ingest_yuv", src, src_bytes, store, table)
    with _timed("ingest_yuv", 0.0, float(src_bytes + K * S_h * S_w * 3)):
        _lib.check_yuv(_lib.load_yuv().tady_ingest_yuv(src.data_ptr(), int(src_bytes), store.data_ptr(), F, table.data_ptr(), table.numel(),
                                                       int(K), int(n_hsets), int(n_vsets), int(n_csets), S_h, S_w, _stream()), "tady_ingest_yuv")
    return store


# ----------------------------------------------------------------------------- fine-tune spatial sampling: window, bilinear resize, crop, flip
def spatial_sample_table(rows, B: int, T: int, H: int, W: int, S: int):
    """Host-side table of spatial_sample (include/tad_mi355x.h): ``rows`` = one (sample, i, j, h, w, rh, rw, oy, ox, flip) per (clip,
    frame), sample = clip * T + frame.  The axis scales are stated here, as f32 quotients ``float32(h) / float32(rh)`` and
    ``float32(w) / float32(rw)``.  Returns the int32 CPU tensor [B * T, SS_ROW_WORDS], checked by tad_spatial_sample_plan_check (word
    count, every frame once, windows inside the source and inside the resized grid, positive finite scales); runs without a GPU."""
    import numpy as np
    n = B * T
    if len(rows) != n:
        raise _lib.TadError(f"spatial_sample_table: {len(rows)} rows for {B} clips of {T} frames")
    tab = np.zeros((n, _lib.SS_ROW_WORDS), dtype=np.int32)
    if n:
        r = np.asarray(rows, dtype=np.int64).reshape(n, 10)
        if (np.abs(r) >= 2 ** 31).any():
            raise _lib.TadError("spatial_sample_table: a row does not fit 32 bits")
        tab[:, :10] = r
        with np.errstate(divide="ignore", invalid="ignore"):
            tab[:, 10] = (r[:, 3].astype(np.float32) / r[:, 5].astype(np.float32)).view(np.int32)
            tab[:, 11] = (r[:, 4].astype(np.float32) / r[:, 6].astype(np.float32)).view(np.int32)
    check(_lib.load().tad_spatial_sample_plan_check(tab.ctypes.data, tab.size, B, T, H, W, S), "tad_spatial_sample_plan_check")
    return torch.from_numpy(tab)


def spatial_sample(x, table, S: int, mean=None, std=None, out=None):
    """Carry the device table ``table`` (a copy of spatial_sample_table()'s: the call's workspace, only read) out on the contiguous f32
    clips x [B,3,T,H,W] or, with ``mean`` / ``std``, on the contiguous uint8 frames x [B,T,H,W,3] (tad_spatial_sample, ONE launch).
    Returns the f32 clips [B,3,T,S,S]; from uint8 frames they have the bits of the f32 route on frames_to_clip(x).  x is only read."""
    m, s = _norm_pair("spatial_sample", mean, std)
    u8 = isinstance(x, torch.Tensor) and x.dtype == torch.uint8
    if u8:
        _req_frames(x, "spatial_sample.x")
        if mean is None:
            raise _lib.TadError("spatial_sample: uint8 frames need mean and std")
        B, T, H, W, _ = x.shape
    else:
        _req(x, torch.float32, "spatial_sample.x")
        if x.dim() != 5 or x.shape[1] != 3 or x.numel() == 0:
            raise _lib.TadError(f"spatial_sample.x: expected f32 clips [B,3,T,H,W] or uint8 frames [B,T,H,W,3], got {tuple(x.shape)}")
        if mean is not None:
            raise _lib.TadError("spatial_sample: f32 clips are normalised already; mean and std go with uint8 frames")
        B, _, T, H, W = x.shape
    lib = _lib.load()
    nbytes = lib.tad_spatial_sample_workspace_bytes(B, T)
    _req_table("spatial_sample", table, (B * T, _lib.SS_ROW_WORDS), nbytes, f"{B} clips of {T} frames", x.device)
    out = _clip_out("spatial_sample", out, (B, 3, T, S, S), torch.float32, x.device)
    with _timed("spatial_sample", 0.0, float(x.numel() * x.element_size() + out.numel() * 4)):
        check(lib.tad_spatial_sample(x.data_ptr(), int(u8), out.data_ptr(), m, s, table.data_ptr(), nbytes, B, T, H, W, S, _stream()),
              "tad_spatial_sample")
    return out


def soft_target_ce(logits, target=None, labels=None, smoothing: float = 0.0):
    """(loss [1], dlogits [B,classes]) of the batch-mean soft-target cross entropy over f32 logits, ONE launch (tad_soft_target_ce):
    ``target`` f32 [B,classes], or int64 ``labels`` [B] smoothed on the fly."""
    _req(logits, torch.float32, "soft_target_ce.logits")
    if logits.dim() != 2:
        raise _lib.TadError(f"soft_target_ce.logits: expected [B,classes], got {tuple(logits.shape)}")
    B, ncls = logits.shape
    if target is not None:
        _req(target, torch.float32, "soft_target_ce.target")
        if target.shape != logits.shape:
            raise _lib.TadError(f"soft_target_ce.target: expected {tuple(logits.shape)}, got {tuple(target.shape)}")
    if labels is not None:
        _req(labels, torch.int64, "soft_target_ce.labels")
        if tuple(labels.shape) != (B,):
            raise _lib.TadError(f"soft_target_ce.labels: expected [{B}], got {tuple(labels.shape)}")
    loss = torch.empty((1,), dtype=torch.float32, device=logits.device)
    dlogits = torch.empty((B, ncls), dtype=torch.float32, device=logits.device)
    check(_lib.load().tad_soft_target_ce(logits.data_ptr(), _p(target), _p(labels), float(smoothing), loss.data_ptr(), dlogits.data_ptr(),
                                         B, ncls, _stream()), "tad_soft_target_ce")
    return loss, dlogits


def frame_loss(kind: str, logits, labels=None, soft=None, ttc=None, class_alpha=None, alpha: float = 1.0, gamma: float = 2.0,
               multiplier: float = 1.0, alpha_pre: float = 0.1, alpha_post: float = 0.5, delta: float = 0.01):
    """(loss [1], dlogits [B,classes]) of one of the frame fine-tuning losses over f32 logits, ONE launch (tad_frame_loss):
    ``kind`` in focal | focal2 | exponential | 2bce | smoothap; int64 ``labels`` [B], f32 ``soft`` [B,2], f32 ``ttc`` [B], f32
    ``class_alpha`` [classes] -- each kind takes exactly its own operands (include/tad_mi355x.h)."""
    if kind not in _lib.FRAME_LOSS_KINDS:
        raise _lib.TadError(f"frame_loss: unknown kind {kind!r} (one of {sorted(_lib.FRAME_LOSS_KINDS)})")
    _req(logits, torch.float32, "frame_loss.logits")
    if logits.dim() != 2:
        raise _lib.TadError(f"frame_loss.logits: expected [B,classes], got {tuple(logits.shape)}")
    B, ncls = logits.shape
    for t, dtype, shape, name in ((labels, torch.int64, (B,), "labels"), (soft, torch.float32, (B, 2), "soft"), (ttc, torch.float32, (B,), "ttc"),
                                  (class_alpha, torch.float32, (ncls,), "class_alpha")):
        if t is not None:
            _req(t, dtype, "frame_loss." + name)
            if tuple(t.shape) != shape or t.device != logits.device:
                raise _lib.TadError(f"frame_loss.{name}: expected {list(shape)} on {logits.device}, got {list(t.shape)} on {t.device}")
    loss = torch.empty((1,), dtype=torch.float32, device=logits.device)
    dlogits = torch.empty((B, ncls), dtype=torch.float32, device=logits.device)
    check(_lib.load().tad_frame_loss(_lib.FRAME_LOSS_KINDS[kind], logits.data_ptr(), _p(labels), _p(soft), _p(ttc), _p(class_alpha), float(alpha),
                                     float(gamma), float(multiplier), float(alpha_pre), float(alpha_post), float(delta), loss.data_ptr(),
                                     dlogits.data_ptr(), B, ncls, _stream()), "tad_frame_loss")
    return loss, dlogits


# ----------------------------------------------------------------------------- MAE pre-training path
def _idx(t, name):
    if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous():
        raise _lib.TadError(f"{name}: expected a contiguous int32 GPU tensor")
    return t


def gather_rows(src, idx, bound_check=True):
    """out[r] = src[idx[r]]; src [R,D] f32, idx [n] int32"""
    _req(src, torch.float32, "gather_rows.src")
    _idx(idx, "gather_rows.idx")
    R, D = src.shape
    out = torch.empty((idx.numel(), D), dtype=torch.float32, device=src.device)
    with _timed("gather", 0.0, 8.0 * idx.numel() * D):
        check(_lib.load().tad_gather_rows_f32(src.data_ptr(), idx.data_ptr(), out.data_ptr(), idx.numel(), D, _stream()), "tad_gather_rows_f32")
    return out


def scatter_rows(src, idx, n_rows):
    """out [n_rows, D] zeros except out[idx[r]] = src[r] (unique indices)"""
    _req(src, torch.float32, "scatter_rows.src")
    _idx(idx, "scatter_rows.idx")
    n, D = src.shape
    assert idx.numel() == n
    out = torch.zeros((n_rows, D), dtype=torch.float32, device=src.device)
    with _timed("gather", 0.0, 8.0 * n * D):
        check(_lib.load().tad_scatter_rows_f32(src.data_ptr(), idx.data_ptr(), out.data_ptr(), n, D, _stream()), "tad_scatter_rows_f32")
    return out


def mae_assemble(x_vis, mask_token, pos, vis_idx, mask_idx, B):
    """decoder input [B, Nv+Nm, D] = cat(x_vis + pos[vis], mask_token + pos[masked])"""
    _req(x_vis, torch.float32, "mae_assemble.x_vis")
    _req(mask_token, torch.float32, "mae_assemble.mask_token")
    _req(pos, torch.float32, "mae_assemble.pos")
    _idx(vis_idx, "mae_assemble.vis_idx")
    _idx(mask_idx, "mae_assemble.mask_idx")
    D = x_vis.shape[-1]
    Nv, Nm = vis_idx.numel() // B, mask_idx.numel() // B
    if x_vis.numel() != B * Nv * D or mask_token.numel() != D or pos.shape[-1] != D or pos.numel() // D < Nv + Nm:
        raise _lib.TadError("mae_assemble: inconsistent shapes")
    out = torch.empty((B, Nv + Nm, D), dtype=torch.float32, device=x_vis.device)
    with _timed("gather", 0.0, 12.0 * out.numel()):
        check(_lib.load().tad_mae_assemble(x_vis.data_ptr(), mask_token.data_ptr(), pos.data_ptr(), vis_idx.data_ptr(), mask_idx.data_ptr(),
                                           out.data_ptr(), B, Nv, Nm, D, _stream()), "tad_mae_assemble")
    return out


def visible_tokens_fwd(x, pos, tok):
    """out [B,Nv,D] = x[b, tok[b,i]] + pos[tok[b,i]]: x [B,N,D] f32, pos [N,D] f32, tok [B,Nv] int32 with values in [0, N), distinct per
    clip (device data: not checked).  The pre-training ABI, include/tad_mi355x_pretrain.h."""
    _req(x, torch.float32, "visible_tokens.x")
    _req(pos, torch.float32, "visible_tokens.pos")
    _idx(tok, "visible_tokens.tok")
    if x.dim() != 3 or pos.dim() != 2 or tok.dim() != 2 or tok.shape[0] != x.shape[0] or pos.shape != x.shape[1:]:
        raise _lib.TadError(f"visible_tokens: inconsistent shapes x {tuple(x.shape)}, pos {tuple(pos.shape)}, tok {tuple(tok.shape)}")
    B, N, D = x.shape
    Nv = tok.shape[1]
    out = torch.empty((B, Nv, D), dtype=torch.float32, device=x.device)
    with _timed("visible_tokens_fwd", 0.0, 12.0 * out.numel()):
        check(_ext("tadp_visible_tokens_fwd")(x.data_ptr(), pos.data_ptr(), tok.data_ptr(), out.data_ptr(), B, N, Nv, D, _stream()),
              "tadp_visible_tokens_fwd")
    return out


def visible_tokens_bwd(g, slot, want_dx=True, want_dpos=True, into=None):
    """(dx [B,N,D] | None, dpos [N,D] | None) from g [B,Nv,D] f32 and slot [B,N] int32 (the inverse of tok, -1 = not visible), one launch.
    dx has every row written (+0 where a token is masked); dpos sums the clips in the order b = 0, 1, ....
    into: an existing f32 tensor of N*D elements the table gradient is ADDED to (a gradient sink) instead of a fresh one."""
    _req(g, torch.float32, "visible_tokens_bwd.g")
    _idx(slot, "visible_tokens_bwd.slot")
    if g.dim() != 3 or slot.dim() != 2 or slot.shape[0] != g.shape[0]:
        raise _lib.TadError(f"visible_tokens_bwd: inconsistent shapes g {tuple(g.shape)}, slot {tuple(slot.shape)}")
    B, Nv, D = g.shape
    N = slot.shape[1]
    dx = torch.empty((B, N, D), dtype=torch.float32, device=g.device) if want_dx else None
    dpos = None
    if into is not None:
        _req(into, torch.float32, "visible_tokens_bwd.into")
        assert want_dpos and into.numel() == N * D
        dpos = into
    elif want_dpos:
        dpos = torch.empty((N, D), dtype=torch.float32, device=g.device)
    with _timed("visible_tokens_bwd", 0.0, 4.0 * D * (B * Nv + (B * N if want_dx else 0) + (N if dpos is not None else 0))):
        check(_ext("tadp_visible_tokens_bwd")(g.data_ptr(), slot.data_ptr(), _p(dx), _p(dpos), int(into is not None), B, N, Nv, D, _stream()),
              "tadp_visible_tokens_bwd")
    return dx, dpos


# ----------------------------------------------------------------------------- serving ABI (libtad_mi355x_serve.so, tads_*)
def _serve(name: str):
    return getattr(_lib.load_serve(), name)


def class_token_entry_fwd(patch, cls, pos):
    """out [B,N+1,D] = cat((cls.expand(B,1,D), patch), 1) + pos: patch [B,N,D] f32, cls [D] f32, pos [N+1,D] f32.  One pass.
    The serving ABI, include/tad_mi355x_serve.h."""
    _req(patch, torch.float32, "class_token_entry.patch")
    _req(cls, torch.float32, "class_token_entry.cls")
    _req(pos, torch.float32, "class_token_entry.pos")
    if patch.dim() != 3 or cls.numel() != patch.shape[2] or pos.dim() != 2 or pos.shape != (patch.shape[1] + 1, patch.shape[2]):
        raise _lib.TadError(f"class_token_entry: inconsistent shapes patch {tuple(patch.shape)}, cls {tuple(cls.shape)}, pos {tuple(pos.shape)}")
    B, N, D = patch.shape
    out = torch.empty((B, N + 1, D), dtype=torch.float32, device=patch.device)
    with _timed("class_token_entry_fwd", 0.0, 4.0 * D * (B * N + N + 2 + B * (N + 1))):
        _lib.check_serve(_serve("tads_class_token_entry_fwd")(patch.data_ptr(), cls.data_ptr(), pos.data_ptr(), out.data_ptr(), B, N, D, _stream()),
                         "tads_class_token_entry_fwd")
    return out


def class_token_entry_bwd(g, want_dpatch=True, want_dpos=True, want_dcls=True, into_pos=None, into_cls=None):
    """(dpatch [B,N,D] | None, dpos [N+1,D] | None, dcls [D] | None) from g [B,N+1,D] f32, one launch.  dpos / dcls sum the clips in the
    order b = 0, 1, ....  into_pos / into_cls: existing f32 tensors of (N+1)*D / D elements the sums are ADDED to (gradient sinks)
    instead of fresh ones.  The kernel has ONE accumulate flag: where both sums are wanted, both have a sink or neither has."""
    _req(g, torch.float32, "class_token_entry_bwd.g")
    if g.dim() != 3 or g.shape[1] < 2:
        raise _lib.TadError(f"class_token_entry_bwd: g {tuple(g.shape)} is no [B,N+1,D] gradient")
    B, N1, D = g.shape
    N = N1 - 1
    for t, n, what in ((into_pos, N1 * D, "into_pos"), (into_cls, D, "into_cls")):
        if t is not None:
            _req(t, torch.float32, "class_token_entry_bwd." + what)
            assert t.numel() == n
    want_dpos, want_dcls = want_dpos or into_pos is not None, want_dcls or into_cls is not None
    dpatch = torch.empty((B, N, D), dtype=torch.float32, device=g.device) if want_dpatch else None
    dpos = into_pos if into_pos is not None else (torch.empty((N1, D), dtype=torch.float32, device=g.device) if want_dpos else None)
    dcls = into_cls if into_cls is not None else (torch.empty(D, dtype=torch.float32, device=g.device) if want_dcls else None)
    fn = _serve("tads_class_token_entry_bwd")
    nbytes = 4.0 * D * (B * N1 + (B * N if want_dpatch else 0) + (N1 if dpos is not None else 0))
    if want_dpos and want_dcls and (into_pos is None) != (into_cls is None):
        raise _lib.TadError("class_token_entry_bwd: one accumulate flag serves dpos and dcls: give both a sink or neither")
    with _timed("class_token_entry_bwd", 0.0, nbytes):
        acc = int(into_pos is not None or into_cls is not None)
        _lib.check_serve(fn(g.data_ptr(), _p(dpatch), _p(dpos), _p(dcls), acc, B, N, D, _stream()), "tads_class_token_entry_bwd")
    return dpatch, (dpos if want_dpos else None), (dcls if want_dcls else None)


def residual_rmsnorm(x, y, ls_gamma=None, norm_gamma=None, eps: float = 1e-6, out=None, xn_dtype=None):
    """(x_out f32, xn | None): x_out = x + y * ls_gamma (ls_gamma None: x + y) and, with norm_gamma, xn = RMSNorm(x_out) * norm_gamma in a
    16-bit operand format (xn_dtype; None = the process-wide one), one pass over the rows.  x, y [..., D] f32; out: where x_out goes (may
    be x itself, not y; None = a fresh tensor).  Evaluation only: nothing is kept for a backward."""
    _req(x, torch.float32, "residual_rmsnorm.x")
    _req(y, torch.float32, "residual_rmsnorm.y")
    D = x.shape[-1]
    rows = x.numel() // D
    if y.shape != x.shape:
        raise _lib.TadError(f"residual_rmsnorm: x {tuple(x.shape)} and y {tuple(y.shape)} differ")
    for t, what in ((ls_gamma, "ls_gamma"), (norm_gamma, "norm_gamma")):
        if t is not None:
            _req(t, torch.float32, "residual_rmsnorm." + what)
            assert t.numel() == D
    if out is None:
        out = torch.empty_like(x)
    else:
        _req(out, torch.float32, "residual_rmsnorm.out")
        assert out.shape == x.shape
    xn = torch.empty(x.shape, dtype=xn_dtype or _op16, device=x.device) if norm_gamma is not None else None
    with _timed("residual_rmsnorm", 0.0, rows * D * (12.0 + (0 if xn is None else xn.element_size()))):
        _lib.check_serve(_serve("tads_residual_rmsnorm_fwd")(x.data_ptr(), y.data_ptr(), _p(ls_gamma), _p(norm_gamma), out.data_ptr(), _p(xn),
                                                             0 if xn is None else _dt(xn), rows, D, float(eps), _stream()),
                         "tads_residual_rmsnorm_fwd")
    return out, xn


def mae_target(videos, mask_idx, tubelet, patch, mean, std, normalize_target=True):
    """videos [B,3,T,H,W] f32 (normalised) -> labels [B, Nm, tub*p*p*3] f32 for the masked tokens (engine_for_pretraining.py:51-66)"""
    _req(videos, torch.float32, "mae_target.videos")
    _idx(mask_idx, "mae_target.mask_idx")
    B, Cc, T, H, W = videos.shape
    if Cc != 3:
        raise _lib.TadError("mae_target: clips must have 3 channels")
    Nm = mask_idx.numel() // B
    labels = torch.empty((B, Nm, tubelet * patch * patch * 3), dtype=torch.float32, device=videos.device)
    with _timed("mae_target", 0.0, 8.0 * labels.numel()):
        check(_lib.load().tad_mae_target(videos.data_ptr(), mask_idx.data_ptr(), labels.data_ptr(), B, Nm, T, H, W, tubelet, patch, _f3(mean),
                                         _f3(std), int(bool(normalize_target)), _stream()), "tad_mae_target")
    return labels


def mae_reconstruct(videos, pred, slot, tubelet, patch, mean, std, normalize_target=True, visible_gain=1.0, want_frames=True,
                    want_err=True):
    """(frames uint8 [B,T,H,W,3] | None, err f32 [B,N] | None): the inverse of ``mae_target``, one launch.  videos [B,3,T,H,W] f32
    (normalised); pred [B, Nm, tub*p*p*3] f32 in mae_target's layout (None or empty: nothing is masked); slot [B,N] int32: the row of
    pred inside its clip that predicts the token, -1 = visible.  Visible patches are the clip's own pixels times ``visible_gain``,
    masked ones the prediction, de-standardised with the patch's statistics when ``normalize_target``; err is the token's mean
    (pred - target)^2, 0 where it is visible.  The reconstruction ABI, include/tad_mi355x_recon.h."""
    _req(videos, torch.float32, "mae_reconstruct.videos")
    _idx(slot, "mae_reconstruct.slot")
    if videos.dim() != 5 or videos.shape[1] != 3:
        raise _lib.TadError(f"mae_reconstruct: videos {tuple(videos.shape)} is no [B,3,T,H,W] clip")
    B, _, T, H, W = videos.shape
    if slot.dim() != 2 or slot.shape[0] != B:
        raise _lib.TadError(f"mae_reconstruct: slot {tuple(slot.shape)} is no [B={B}, N] table")
    N = slot.shape[1]
    Nm = 0
    if pred is not None and pred.numel():
        _req(pred, torch.float32, "mae_reconstruct.pred")
        width = tubelet * patch * patch * 3
        if pred.numel() % (B * width):
            raise _lib.TadError(f"mae_reconstruct: pred {tuple(pred.shape)} is no [B={B}, n_mask, {width}] prediction")
        Nm = pred.numel() // (B * width)
    else:
        pred = None
    if not (want_frames or want_err):
        raise _lib.TadError("mae_reconstruct: neither frames nor err is wanted")
    if tubelet > 0 and patch > 0 and (T // tubelet) * (H // patch) * (W // patch) != N:
        raise _lib.TadError(f"mae_reconstruct: slot has {N} columns, the clip {(T // tubelet) * (H // patch) * (W // patch)} tokens")
    frames = torch.empty((B, T, H, W, 3), dtype=torch.uint8, device=videos.device) if want_frames else None
    err = torch.empty((B, N), dtype=torch.float32, device=videos.device) if want_err else None
    with _timed("mae_reconstruct", 0.0, 4.0 * videos.numel() + 4.0 * B * Nm * tubelet * patch * patch * 3 + (videos.numel() if want_frames else 0)):
        _lib.check_recon(_lib.load_recon().tadr_mae_reconstruct(videos.data_ptr(), _p(pred), slot.data_ptr(), _p(frames), _p(err), B, Nm, T, H, W,
                                                                 int(tubelet), int(patch), _f3(mean), _f3(std), int(bool(normalize_target)),
                                                                 float(visible_gain), _stream()), "tadr_mae_reconstruct")
    return frames, err


def mse_loss(pred, target, want_grad=True):
    """returns (loss scalar tensor, grad|None) of nn.MSELoss()(pred, target)"""
    _req(pred, torch.float32, "mse.pred")
    _req(target, torch.float32, "mse.target")
    n = pred.numel()
    if target.numel() != n:
        raise _lib.TadError("mse_loss: pred and target differ in size")
    lib = _lib.load()
    partials = torch.empty(lib.tad_mse_loss_blocks(n), dtype=torch.float32, device=pred.device)
    grad = torch.empty_like(pred) if want_grad else None
    with _timed("mse", 0.0, (12.0 if want_grad else 8.0) * n):
        check(lib.tad_mse_loss(pred.data_ptr(), target.data_ptr(), n, partials.data_ptr(), _p(grad), _stream()), "tad_mse_loss")
    return partials.sum() / n, grad


def device_info():
    cu, clk, ldsb = C.c_int(), C.c_int(), C.c_int()
    name = C.create_string_buffer(64)
    check(_lib.load().tad_device_info(C.byref(cu), C.byref(clk), C.byref(ldsb), name, 64), "tad_device_info")
    return {"cu_count": cu.value, "clock_khz": clk.value, "lds_bytes_per_cu": ldsb.value, "arch": name.value.decode()}


# ----------------------------------------------------------------------------- precise mode (parity gate)
def split_bf16x3(x, role_b: bool, stack: bool = False, dtype=torch.bfloat16):
    """x [M,K] f32 -> 16-bit [M,3K] ([hi|hi|lo] or [hi|lo|hi]) or, stacked, [3M,K]; hi = op16(x), lo = op16(x - hi)"""
    _req(x, torch.float32, "split.x")
    M, K = x.shape
    out = torch.empty((3 * M, K) if stack else (M, 3 * K), dtype=dtype, device=x.device)
    check(_fn("tad_split_bf16x3", dtype)(x.data_ptr(), out.data_ptr(), M, K, int(role_b), int(stack), _stream()), "tad_split_bf16x3")
    return out


def im2col_tubelets_f32(x, tubelet: int, patch: int):
    _req(x, torch.float32, "im2col_f32.x")
    B, Cc, T, H, W = x.shape
    _, cols = _patch_matrix(B, Cc, T, H, W, tubelet, patch, torch.float32, x.device)
    check(_lib.load().tad_im2col_tubelets_f32(x.data_ptr(), cols.data_ptr(), B, Cc, T, H, W, tubelet, patch, _stream()),
          "tad_im2col_tubelets_f32")
    return cols


def attn_fwd_f32(qkv, B: int, N: int, H: int, scale: float, want_lse=False, d: int = 64, drop_p: float = 0.0, seed: int = 0):
    """f32 attention on the matrix pipe (precise mode; head dims without a 16-bit kernel: d = 80; attention dropout: drop_p, seed)"""
    _req(qkv, torch.float32, "attn_f32.qkv")
    if qkv.numel() != B * N * 3 * H * d:
        raise _lib.TadError("attn_fwd_f32: qkv element count mismatch")
    out = torch.empty((B * N, H * d), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device) if want_lse else None
    with _timed("attn_f32", 4.0 * B * H * N * N * d, 4.0 * 4 * B * N * H * d):
        check(_lib.load().tad_attn_fwd_f32(qkv.data_ptr(), out.data_ptr(), _p(lse), B, N, H, int(d), float(scale), float(drop_p),
                                           int(seed) & 0xffffffff, _stream()), "tad_attn_fwd_f32")
    return out, lse


def attn_bwd_f32(qkv, out, dout, lse, B: int, N: int, H: int, scale: float, d: int = 64, drop_p: float = 0.0, seed: int = 0):
    for t, n in ((qkv, "qkv"), (out, "out"), (dout, "dout"), (lse, "lse")):
        _req(t, torch.float32, "attn_bwd_f32." + n)
    if qkv.numel() != B * N * 3 * H * d or out.numel() != B * N * H * d or dout.numel() != out.numel():
        raise _lib.TadError("attn_bwd_f32: element count mismatch")
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device)
    with _timed("attn_f32", 8.0 * B * H * N * N * d, 4.0 * 8 * B * N * H * d):
        check(_lib.load().tad_attn_bwd_f32(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), delta.data_ptr(),
                                           B, N, H, int(d), float(scale), float(drop_p), int(seed) & 0xffffffff, _stream()), "tad_attn_bwd_f32")
    return dqkv


def gelu_f32(h):
    _req(h, torch.float32, "gelu_f32.h")
    a = torch.empty_like(h)
    check(_lib.load().tad_gelu_f32(h.data_ptr(), a.data_ptr(), h.numel(), _stream()), "tad_gelu_f32")
    return a


def gelu_bwd_f32(dy, h):
    _req(dy, torch.float32, "gelu_bwd_f32.dy")
    _req(h, torch.float32, "gelu_bwd_f32.h")
    dh = torch.empty_like(h)
    check(_lib.load().tad_gelu_bwd_f32(dy.data_ptr(), h.data_ptr(), dh.data_ptr(), h.numel(), _stream()), "tad_gelu_bwd_f32")
    return dh


def colsum_window_f32(a, r0, rc):
    """a [B, R, N] f32 -> [N]: sum over the batch and rows r0 .. r0+rc-1 (no copy of the window)"""
    _req(a, torch.float32, "colsum_window.a")
    B, R, N = a.shape
    out = torch.empty(N, dtype=torch.float32, device=a.device)
    lib = _lib.load()
    ws = workspace(lib.tad_colsum_workspace_bytes(B * rc, N), a.device)
    check(lib.tad_colsum_window_f32(a.data_ptr(), out.data_ptr(), 0, ws.data_ptr(), ws.numel(), B, R, N, int(r0), int(rc), _stream()),
          "tad_colsum_window_f32")
    return out


def colsum_f32(a):
    _req(a, torch.float32, "colsum_f32.a")
    M, N = a.shape
    out = torch.empty(N, dtype=torch.float32, device=a.device)
    check(_lib.load().tad_colsum_f32(a.data_ptr(), out.data_ptr(), M, N, _stream()), "tad_colsum_f32")
    return out
