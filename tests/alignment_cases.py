"""Valid, in-contract calls of the C entry points, as data: what tests/test_alignment_cpu.py misaligns one pointer at a time (fake
addresses, every call refused before a launch) and what tests/test_alignment_gpu.py runs on real tensors inside the guard arena.  No GPU
use here; the workspace sizes come from the library's own *_workspace_bytes queries, which need no device.

A case lists the arguments in signature order.  A pointer argument is a P (name as in tests/alignment_contract.py, element type,
shape, role, optional host data), None for an absent optional pointer; everything else is passed as it stands.  Shapes are the
smallest legal ones with ragged tiles: tests/test_numeric_edges_gpu.LIN_SMALL for the GEMMs, tests/test_guarded_gpu.ATT-like
attention shapes with a key tail.
"""
import ctypes as C

from simple_tad_amd import _lib

import alignment_contract as AC

ITEM = {"f32": 4, "op16": 2, "u16": 2, "i32": 4, "i64": 8, "u64": 8, "u8": 1, "f64": 8}
OP_CODE = {"bf16": _lib.TAD_BF16, "f16": _lib.TAD_F16}
LIN_SMALL = (70, 408, 128)  # M, N, Kd: tests/test_numeric_edges_gpu.LIN_SMALL


class P:
    """a device pointer argument.  data: callable(torch, generator) -> host tensor of ``shape`` (default: standard normal values for the
    floating-point types); index_range: the guards of an integer tensor hold values in [0, index_range)"""

    def __init__(self, name, dtype, shape, role="input", data=None, index_range=None):
        assert dtype in ITEM and role in ("input", "output", "inout", "workspace")
        self.name, self.dtype, self.shape, self.role, self.data, self.index_range = name, dtype, tuple(shape), role, data, index_range

    @property
    def nbytes(self):
        n = ITEM[self.dtype]
        for s in self.shape:
            n *= s
        return n


class Case:
    def __init__(self, symbol, cid, args, align=None, gpu=True):
        """align: {argument: bytes} where the requirement of this case is a conditional one of the table's row; gpu=False: the case
        describes a call whose device tables the GPU control does not build (its valid calls are the entry point's own tests)"""
        self.symbol, self.cid, self.args, self.align, self.gpu = symbol, cid, list(args), dict(align or {}), gpu

    def pointers(self):
        """[(position, P)] of the pointer arguments present"""
        return [(i, a) for i, a in enumerate(self.args) if isinstance(a, P)]

    def required(self, name):
        row = AC.CONTRACT[self.symbol][name]
        if not isinstance(row, AC.A):
            return None
        n = self.align.get(name, row.n)
        assert n in row.allowed(), f"{self.symbol} {self.cid}: {name} = {n} is not a requirement the table states ({row})"
        return n

    def __repr__(self):
        return f"{self.symbol}[{self.cid}]"


def f3(*v):
    return (C.c_float * 3)(*v)


MEAN3, STD3 = f3(0.485, 0.456, 0.406), f3(0.229, 0.224, 0.225)


def ws(name, nbytes):
    return P(name, "u8", (max(int(nbytes), 16),), "workspace")


def _lib_():
    return _lib.load()


def idx(n, hi):
    return lambda torch, g: torch.randperm(hi, generator=g)[:n].to(torch.int32) if n <= hi else torch.randint(0, hi, (n,), generator=g, dtype=torch.int32)


def const(*vals):
    return lambda torch, g: torch.tensor(vals, dtype=torch.float32)


# ------------------------------------------------------------------ builders: fmt ("bf16" | "f16") -> cases of the bf16-named entry point
def cast(fmt):
    return [Case("tad_cast_f32_bf16", "tail", [P("src", "f32", (19,)), P("dst", "op16", (19,), "output"), 19, None])]


def transpose_cast(fmt):
    return [Case("tad_transpose_cast_f32_bf16", "5x7", [P("src", "f32", (5, 7)), P("dst", "op16", (7, 5), "output"), 5, 7, None])]


def transpose_batched(fmt):
    table = lambda torch, g: torch.tensor([[0, 0, 16, 8, 8, 16, 0, 0]], dtype=torch.int32)  # one 8 x 16 matrix, one tile  # noqa: E731
    return [Case("tad_transpose_bf16_batched", "8x16", [P("src", "u16", (8, 16), data=lambda torch, g: torch.arange(128, dtype=torch.int16).reshape(8, 16)),
                                                        P("dst", "u16", (16, 8), "output"), P("table", "i32", (1, 8), data=table, index_range=1), 1, None])]


def _clip(B=1, C_=3, T=2, HW=8):
    return (B, C_, T, HW, HW)


def im2col(fmt, symbol="tad_im2col_tubelets", src="f32", dst="op16", pair_align=(8, 4)):
    out = []
    for patch, cid in ((8, "wide"), (6, "pairs")):
        K = 3 * 2 * patch * patch
        ldk = (K + 63) // 64 * 64
        al = {} if patch == 8 else {"x": pair_align[0], "cols": pair_align[1]}
        out.append(Case(symbol, cid, [P("x", src, _clip(HW=patch)), P("cols", dst, (1, K if patch == 8 and dst == "f32" else ldk), "output"),
                                      1, 3, 2, patch, patch, 2, patch, None], al))
    return out


def im2col_f32(fmt):
    return im2col(fmt, "tad_im2col_tubelets_f32", "f32", "f32", (8, 8))


def im2col_16(fmt):
    return im2col(fmt, "tad_im2col_tubelets_16", "u16", "u16", (4, 4))


def _frames(torch, g, shape):
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)


def im2col_u8(fmt):
    return [Case("tad_im2col_tubelets_u8", "wide", [P("frames", "u8", (1, 2, 8, 8, 3), data=lambda t, g: _frames(t, g, (1, 2, 8, 8, 3))),
                                                   P("cols", "op16", (1, 384), "output"), 1, 2, 8, 8, 2, 8, MEAN3, STD3, 0, 1, None])]


def frame_windows(fmt):
    return [Case("tad_im2col_frame_windows", f"wide_{f}", [P("store", "u8", (3, 8, 8, 3), data=lambda t, g: _frames(t, g, (3, 8, 8, 3))), 3,
                                                          P("idx", "i32", (2,), data=lambda t, g: t.tensor([2, 0], dtype=t.int32), index_range=3),
                                                          P("cols", "u16", (1, 384), "output"), OP_CODE[f], 1, 2, 8, 8, 2, 8, MEAN3, STD3, 0, None])
            for f in ("bf16", "f16")]


def patch_embed_fwd(fmt):
    D = 16
    return [Case("tad_patch_embed_fwd", "p8", [P("x", "f32", _clip(B=2)), P("w_bf16", "op16", (D, 384)), P("bias", "f32", (D,)), P("pos", "f32", (1, D)),
                                               P("out", "f32", (2, D), "output"), P("cols", "op16", (2, 384), "output"), 2, 3, 2, 8, 8, 2, 8, D, None]),
            # patch 6: K = 216 in rows of ldk = 256, the weight zero-padded to that stride
            Case("tad_patch_embed_fwd", "p6", [P("x", "f32", _clip(B=2, HW=6)), P("w_bf16", "op16", (D, 256), data=lambda t, g: t.cat([t.randn(D, 216, generator=g), t.zeros(D, 40)], 1)),
                                               P("bias", "f32", (D,)), P("pos", "f32", (1, D)), P("out", "f32", (2, D), "output"), P("cols", "op16", (2, 256), "output"),
                                               2, 3, 2, 6, 6, 2, 6, D, None], {"x": 8})]


def patch_embed_implicit(fmt):
    D = 16
    return [Case("tad_patch_embed_fwd_implicit", "p16", [P("x", "f32", _clip(B=2, HW=16)), P("w_bf16", "op16", (D, 1536)), P("bias", "f32", (D,)),
                                                         P("pos", "f32", (1, D)), P("out", "f32", (2, D), "output"), 2, 3, 2, 16, 16, 2, 16, D, None])]


def patch_embed_gemm(fmt):
    M, ntok, D, K = 6, 3, 20, 64
    return [Case("tad_patch_embed_gemm", "small", [P("cols", "op16", (M, K)), P("w_bf16", "op16", (D, K)), P("bias", "f32", (D,)), P("pos", "f32", (ntok, D)),
                                                   P("out", "f32", (M, D), "output"), M, ntok, D, K, None])]


def patch_embed_bwd(fmt):
    M, D, K = 70, 24, 64
    n = _lib_().tad_patch_embed_bwd_workspace_bytes(M, D, K)
    return [Case("tad_patch_embed_bwd", "small", [P("dy_bf16", "op16", (M, D)), P("cols", "op16", (M, K)), P("dW", "f32", (D, K), "output"),
                                                  P("db", "f32", (D,), "output"), ws("ws", n), n, M, D, K, None])]


def layernorm_fwd(fmt):
    rows, D = 5, 20
    mk = lambda y, code: [P("x", "f32", (rows, D)), P("gamma", "f32", (D,)), P("beta", "f32", (D,)), P("y", y, (rows, D), "output"), code,  # noqa: E731
                          P("mean", "f32", (rows,), "output"), P("rstd", "f32", (rows,), "output"), rows, D, 1e-6, None]
    return [Case("tad_layernorm_fwd", "y_f32", mk("f32", _lib.TAD_F32)), Case("tad_layernorm_fwd", "y_16", mk("op16", OP_CODE[fmt]), {"y": 8})]


def layernorm_bwd(fmt):
    rows, D, per = 37, 20, 8
    n = _lib_().tad_layernorm_bwd_workspace_bytes(rows, D)
    rs = lambda t, g: t.tensor([1.0, 0.0, 1.25, 0.5, 2.0])  # noqa: E731
    pos = lambda t, g: t.rand(rows, generator=g) + 0.5  # noqa: E731
    mk = lambda dy, code: [P("dy", dy, (rows, D)), code, P("x", "f32", (rows, D)), P("gamma", "f32", (D,)), P("mean", "f32", (rows,)),  # noqa: E731
                           P("rstd", "f32", (rows,), data=pos), P("dres", "f32", (rows, D)), P("dx", "f32", (rows, D), "output"),
                           P("dx_bf16", "op16", (rows, D), "output"), P("dgamma", "f32", (D,), "inout"), P("dbeta", "f32", (D,), "inout"),
                           P("colsum_dx", "f32", (D,), "inout"), P("rowscale", "f32", (5,), data=rs), per, 1, ws("ws", n), n, rows, D, None]
    return [Case("tad_layernorm_bwd", "dy_f32", mk("f32", _lib.TAD_F32)), Case("tad_layernorm_bwd", "dy_16", mk("op16", OP_CODE[fmt]), {"dy": 8})]


def linear_fwd(fmt):
    M, N, K = LIN_SMALL
    x, w, b = (lambda: P("x", "op16", (M, K))), (lambda: P("w", "op16", (N, K), data=lambda t, g: t.randn(N, K, generator=g) * 0.05)), (lambda: P("bias", "f32", (N,)))
    rs = lambda t, g: t.tensor([0.0 if i % 3 == 0 else 1.25 for i in range(10)])  # noqa: E731
    return [
        Case("tad_linear_fwd", "bias_16", [x(), w(), b(), P("y", "op16", (M, N), "output"), OP_CODE[fmt], _lib.EPI_BIAS, None, None, None, None, 1, None, 0, M, N, K, None]),
        Case("tad_linear_fwd", "gelu_preact", [x(), w(), b(), P("y", "op16", (M, N), "output"), OP_CODE[fmt], _lib.EPI_BIAS_GELU, P("preact", "op16", (M, N), "output"),
                                               None, None, None, 1, None, 0, M, N, K, None]),
        Case("tad_linear_fwd", "residual_f32", [x(), w(), b(), P("y", "f32", (M, N), "output"), _lib.TAD_F32, _lib.EPI_BIAS_RESIDUAL, None, P("residual", "f32", (M, N)),
                                                P("gamma", "f32", (N,)), P("rowscale", "f32", (10,), data=rs), 7, ws("ws", 8192), 8192, M, N, K, None]),
    ]


def linear_fwd_qkv(fmt):
    M, N, K = LIN_SMALL
    return [Case("tad_linear_fwd_qkv", "prescaled", [P("x", "op16", (M, K)), P("w", "op16", (N, K), data=lambda t, g: t.randn(N, K, generator=g) * 0.05),
                                                     P("q_bias", "f32", (N // 3,)), P("v_bias", "f32", (N // 3,)), P("y", "op16", (M, N), "output"), OP_CODE[fmt], 0.18,
                                                     M, N, K, None])]


def linear_bwd_input(fmt):
    M, Kout, Nred = 70, 408, 128  # dx [M, K] = dy [M, N] wT[K, N]^T: the reduction runs over N
    return [Case("tad_linear_bwd_input", "gelu", [P("dy", "op16", (M, Nred)), P("wT", "op16", (Kout, Nred), data=lambda t, g: t.randn(Kout, Nred, generator=g) * 0.05),
                                                  P("dx", "op16", (M, Kout), "output"), OP_CODE[fmt], P("gelu_preact", "op16", (M, Kout)), ws("ws", 8192), 8192, M, Nred, Kout,
                                                  None])]


def _tn(M, N, K):
    return _lib_().tad_linear_bwd_weight_workspace_bytes(M, N, K)


def linear_bwd_weight(fmt):
    M, N, K = LIN_SMALL
    n = _tn(M, N, K)
    return [Case("tad_linear_bwd_weight", "bias", [P("dy", "op16", (M, N)), P("x", "op16", (M, K)), P("dW", "f32", (N, K), "output"), P("db", "f32", (N,), "output"), 0,
                                                   ws("ws", n), n, M, N, K, None])]


def linear_bwd_weight_qkv(fmt):
    M, N, K = LIN_SMALL
    n = _tn(M, N, K)
    return [Case("tad_linear_bwd_weight_qkv", "accumulate", [P("dy", "op16", (M, N)), P("x", "op16", (M, K)), P("dW", "f32", (N, K), "inout"), P("dq_bias", "f32", (N // 3,), "inout"),
                                                             P("dv_bias", "f32", (N // 3,), "inout"), 1, ws("ws", n), n, M, N, K, None])]


def linear_bwd_weight_pair(fmt):
    M, N1, K = LIN_SMALL
    N2 = 136
    n = max(_tn(M, N1, K), _tn(M, N2, K), _tn(M, N1 + N2, K))
    return [Case("tad_linear_bwd_weight_pair", "qkv_proj", [P("dy1", "op16", (M, N1)), P("x1", "op16", (M, K)), P("dW1", "f32", (N1, K), "output"), P("db1", "f32", (N1 // 3,), "output"),
                                                            P("db1b", "f32", (N1 // 3,), "output"), N1, P("dy2", "op16", (M, N2)), P("x2", "op16", (M, K)), P("dW2", "f32", (N2, K), "output"),
                                                            N2, 0, ws("ws", n), n, M, K, None])]


ATT = (2, 9, 2, 64)  # B, N, H, d: a ragged key tail in every clip


def _lse(B, N, H):
    return lambda t, g: t.rand(B, H, N, generator=g) + 2.0


def _scale(B):
    return lambda t, g: t.tensor([1.25, 0.0][:B])


def attn_fwd(fmt):
    B, N, H, d = ATT
    qkv = lambda: P("qkv", "op16", (B * N, 3 * H * d))  # noqa: E731
    return [
        Case("tad_attn_fwd", "skip_16", [qkv(), P("out", "op16", (B * N, H * d), "output"), OP_CODE[fmt], P("out_lo", "op16", (B * N, H * d), "output"),
                                         P("lse", "f32", (B, H, N), "output"), P("clip_scale", "f32", (B,), data=_scale(B)), B, N, H, d, d ** -0.5, 1, 0.0, 0, None]),
        Case("tad_attn_fwd", "plain_f32", [qkv(), P("out", "f32", (B * N, H * d), "output"), _lib.TAD_F32, None, P("lse", "f32", (B, H, N), "output"), None,
                                           B, N, H, d, d ** -0.5, 0, 0.0, 0, None]),
    ]


def attn_bwd(fmt):
    B, N, H, d = ATT
    small = lambda t, g: t.randn(B * N, H * d, generator=g) * 0.01  # noqa: E731
    return [Case("tad_attn_bwd", "skip", [P("qkv", "op16", (B * N, 3 * H * d)), P("out", "op16", (B * N, H * d)), P("out_lo", "op16", (B * N, H * d), data=small),
                                          P("dout", "op16", (B * N, H * d)), P("lse", "f32", (B, H, N), data=_lse(B, N, H)), P("clip_scale", "f32", (B,), data=_scale(B)),
                                          P("dqkv", "op16", (B * N, 3 * H * d), "output"), P("delta", "f32", (2 * B * H * N,), "workspace"), B, N, H, d, d ** -0.5, 1, 0.0, 0,
                                          None])]


def attn_colsum(fmt):
    B, N, H, d = ATT
    return [Case("tad_attn_colsum", f, [P("qkv", "u16", (B * N, 3 * H * d), data=_op16_bits((B * N, 3 * H * d), dt)), OP_CODE[f],
                                        P("lse", "f32", (B, H, N), data=_lse(B, N, H)), P("w", "f32", (B, N)), P("out", "f32", (B, H, N), "output"), B, N, H, d, d ** -0.5, 0,
                                        None]) for f, dt in (("bf16", "bfloat16"), ("f16", "float16"))]


def attn_fwd_f32(fmt):
    B, N, H, d = ATT
    return [Case("tad_attn_fwd_f32", "lse", [P("qkv", "f32", (B * N, 3 * H * d)), P("out", "f32", (B * N, H * d), "output"), P("lse", "f32", (B, H, N), "output"),
                                             B, N, H, d, d ** -0.5, 0.0, 0, None])]


def attn_bwd_f32(fmt):
    B, N, H, d = ATT
    return [Case("tad_attn_bwd_f32", "plain", [P("qkv", "f32", (B * N, 3 * H * d)), P("out", "f32", (B * N, H * d)), P("dout", "f32", (B * N, H * d)),
                                               P("lse", "f32", (B, H, N), data=_lse(B, N, H)), P("dqkv", "f32", (B * N, 3 * H * d), "output"),
                                               P("delta", "f32", (B * H * N,), "workspace"), B, N, H, d, d ** -0.5, 0.0, 0, None])]


POOL = (2, 5, 12)  # B, N, D


def meanpool_fwd(fmt):
    B, N, D = POOL
    return [Case("tad_meanpool_fwd", "small", [P("x", "f32", (B, N, D)), P("y", "f32", (B, D), "output"), P("ws", "f32", (B * _lib.POOL_SPLIT * D,), "workspace"), B, N, D, None])]


def meanpool_bwd(fmt):
    B, N, D = POOL
    return [Case("tad_meanpool_bwd", "both", [P("dy", "f32", (B, D)), P("dx", "f32", (B, N, D), "output"), P("dx_bf16", "op16", (B, N, D), "output"), B, N, D, None])]


def _pooled_ops():
    return [("bf16", "bfloat16"), ("f16", "float16")]


def _op16_bits(shape, dt, scale=1.0):
    return lambda t, g: (t.randn(*shape, generator=g) * scale).to(getattr(t, dt)).view(t.int16)


def colsum_segments(fmt):
    B, N, K = 2, 5, 16
    n = B * _lib.POOL_SPLIT * K * 4
    return [Case("tad_colsum_segments", f, [P("a", "u16", (B * N, K), data=_op16_bits((B * N, K), dt)), OP_CODE[f], P("S", "f32", (B, K), "output"), ws("ws", n), n, B, N, K, None])
            for f, dt in _pooled_ops()]


def pooled_linear(fmt):
    B, N, D, K = 2, 5, 6, 16
    return [Case("tad_pooled_linear", f, [P("S", "f32", (B, K)), P("w", "u16", (D, K), data=_op16_bits((D, K), dt, 0.1)), OP_CODE[f], P("bias", "f32", (D,)),
                                          P("rowscale", "f32", (B,), data=_scale(B)), P("xbar", "f32", (B, D)), P("out", "f32", (B, D), "output"), B, N, D, K, None])
            for f, dt in _pooled_ops()]


def gelu_grad_bcast(fmt):
    B, N, K = 2, 5, 16
    return [Case("tad_gelu_grad_bcast", f, [P("t", "f32", (B, K)), P("h", "u16", (B * N, K), data=_op16_bits((B * N, K), dt)), P("dh", "u16", (B * N, K), "output"), OP_CODE[f],
                                            B, N, K, None]) for f, dt in _pooled_ops()]


def colsum_16(fmt):
    M, N = 5, 16
    n = _lib_().tad_colsum_workspace_bytes(M, N)
    return [Case("tad_colsum_bf16", "accumulate", [P("a", "op16", (M, N)), P("out", "f32", (N,), "inout"), 1, ws("ws", n), n, M, N, None])]


def colsum_window(fmt):
    B, R, N, r0, rc = 2, 5, 12, 1, 3
    n = _lib_().tad_colsum_workspace_bytes(B * rc, N)
    return [Case("tad_colsum_window_f32", "window", [P("a", "f32", (B, R, N)), P("out", "f32", (N,), "output"), 0, ws("ws", n), n, B, R, N, r0, rc, None])]


def colsum_f32(fmt):
    return [Case("tad_colsum_f32", "wide", [P("a", "f32", (5, 8)), P("out", "f32", (8,), "output"), 5, 8, None]),
            Case("tad_colsum_f32", "any_n", [P("a", "f32", (5, 6)), P("out", "f32", (6,), "output"), 5, 6, None], {"a": 4})]


def scale_cast(fmt):
    M, N = 5, 12
    return [Case("tad_scale_cast_bf16", "all", [P("x", "f32", (M, N)), P("y", "op16", (M, N), "output"), P("gamma", "f32", (N,)),
                                                P("rowscale", "f32", (3,), data=const(1.5, 0.0, 0.75)), 2, M, N, None])]


def split3(fmt):
    M, K = 3, 8
    return [Case("tad_split_bf16x3", "concat", [P("x", "f32", (M, K)), P("out", "op16", (M, 3 * K), "output"), M, K, 0, 0, None])]


def gelu_f32(fmt):
    return [Case("tad_gelu_f32", "n7", [P("h", "f32", (7,)), P("a", "f32", (7,), "output"), 7, None])]


def gelu_bwd_f32(fmt):
    return [Case("tad_gelu_bwd_f32", "n7", [P("dy", "f32", (7,)), P("h", "f32", (7,)), P("dh", "f32", (7,), "output"), 7, None])]


def rowscale_transpose_cast(fmt):
    N, K = 5, 7
    return [Case("tad_rowscale_transpose_cast", "5x7", [P("w", "f32", (N, K)), P("gamma", "f32", (N,)), P("out", "op16", (K, N), "output"), N, K, None])]


def layerscale_grads(fmt):
    out = []
    for K, cid in ((1032, "vector_width"), (6, "element_width")):  # K % 4 == 0 with more than one step of the 256 lanes / K % 4 != 0
        N = 3
        out.append(Case("tad_layerscale_grads", cid, [P("T", "f32", (N, K)), P("W", "f32", (N, K)), P("bias", "f32", (N,)), P("cs", "f32", (N,)), P("gamma", "f32", (N,)),
                                                      P("dW", "f32", (N, K), "inout"), P("dbias", "f32", (N,), "inout"), P("dgamma", "f32", (N,), "inout"), 1, N, K, None]))
    return out


def branch_dropout_fwd(fmt):
    out = []
    for D, cid in ((8, "vector_width"), (6, "element_width")):
        M = 5
        out.append(Case("tad_branch_dropout_fwd", cid, [P("u", "f32", (M, D)), P("res", "f32", (M, D)), P("out", "f32", (M, D), "output"), P("gamma", "f32", (D,)),
                                                        P("rowscale", "f32", (3,), data=const(1.5, 0.0, 0.75)), 2, 0.25, 1234, M, D, None]))
    return out


def branch_dropout_cast(fmt):
    out = []
    for D, cid in ((8, "vector_width"), (6, "element_width")):
        M = 5
        out.append(Case("tad_branch_dropout_cast", cid, [P("g", "f32", (M, D)), P("y", "op16", (M, D), "output"), P("rowscale", "f32", (3,), data=const(1.5, 0.0, 0.75)),
                                                         2, 0.25, 1234, M, D, None]))
    return out


def _sumsq_ws():
    return _lib_().tad_sumsq_workspace_bytes()


def sumsq(fmt):
    n = _sumsq_ws()
    return [Case("tad_sumsq_f32", "n1027", [P("x", "f32", (1027,)), 1027, P("out", "f32", (1,), "inout", data=const(0.0)), ws("ws", n), n, None])]


def grad_norm_coef(fmt):
    n = _sumsq_ws()
    return [Case("tad_grad_norm_coef", f"n{k}", [P("x", "f32", (k,)), k, 0.5, 1.0, P("out3", "f32", (3,), "output"), ws("ws", n), n, None]) for k in (1, 2, 3, 1027, 1028)]


def grad_segnorm(fmt):
    n, nws = 100, _lib_().tad_grad_segnorm_workspace_bytes(1)

    def table(t, g):
        import numpy as np
        return t.from_numpy(np.array([(0, n, 0, 0)], dtype=[("o", "<i8"), ("l", "<i8"), ("s", "<i4"), ("f", "<i4")]).view(np.uint8).copy())

    def work(t, g):
        import numpy as np
        return t.from_numpy(np.array([0, n], dtype="<i8").view(np.uint8).copy())
    return [Case("tad_grad_segnorm", "one_segment", [P("grad", "f32", (n,)), n, P("table", "u8", (24,), data=table), 1, P("work", "u8", (16,), data=work), 1,
                                                     P("coef", "f32", (1,), data=const(0.5)), P("acc", "f64", (1,), "inout", data=lambda t, g: t.zeros(1, dtype=t.float64)),
                                                     P("last", "f32", (1,), "inout", data=const(0.0)),
                                                     P("counters", "i32", (3,), "inout", data=lambda t, g: t.zeros(3, dtype=t.int32), index_range=1), 1, ws("ws", nws), nws, None])]


def adamw(fmt):
    n = _lib.ADAMW_CHUNK
    lr, wd, st = (C.c_float * 1)(1e-3), (C.c_float * 1)(0.05), (C.c_int32 * 1)(1)
    pos = lambda t, g: t.rand(n, generator=g) * 1e-3  # noqa: E731
    return [Case("tad_adamw_step", "one_chunk", [P("param", "f32", (n,), "inout"), P("grad", "f32", (n,)), P("exp_avg", "f32", (n,), "inout"),
                                                 P("exp_avg_sq", "f32", (n,), "inout", data=pos), P("param_bf16", "op16", (n,), "output"),
                                                 P("chunk_group", "u8", (1,), data=lambda t, g: t.zeros(1, dtype=t.uint8)), n, lr, wd, 1, st, 0.9, 0.999, 1e-8,
                                                 P("grad_scale", "f32", (1,), data=const(0.5)), P("sumsq_partials", "f32", (1,), "output"), None])]


def ema(fmt):
    return [Case("tad_ema_update", "tables", [P("tensors", "i64", (1, 4)), 1, P("chunks", "i32", (1, 2)), 1, 0.999, 0.001, None], gpu=False)]


def _table_bytes(table):
    """an int32 CPU table as the bytes of a workspace"""
    return lambda t, g: table.contiguous().view(t.uint8).clone()


def randaug(fmt):
    from simple_tad_amd import kernels as K
    B, T, H, W = 2, 2, 5, 7  # 105 bytes per frame: the statistics kernel peels a head of up to 15 bytes, whole 16-byte pieces and a tail
    fill = (128, 128, 128)
    layers = [[(0, _lib.RA_AUTOCONTRAST, 0, 0.0, None, fill, 0), (1, _lib.RA_EQUALIZE, 0, 0.0, None, fill, 0)],    # per-frame statistics
              [(1, _lib.RA_CONTRAST, 0, 1.3, None, fill, 0), (0, _lib.RA_INVERT, 0, 0.0, None, fill, 0)],          # statistics / lookup table
              [(0, _lib.RA_SOLARIZE, 100, 0.0, None, fill, 0), (1, _lib.RA_BRIGHTNESS, 0, 1.3, None, fill, 0)]]
    table, stats = K.randaug_table(layers, B, T)
    assert stats == 0b011, "the first two layers launch the statistics kernel"
    n = _lib_().tad_randaug_workspace_bytes(3, B, T, H, W)
    return [Case("tad_randaug_apply", "three_layers", [P("x", "u8", (B, T, H, W, 3), data=lambda t, g: _frames(t, g, (B, T, H, W, 3))), P("out", "u8", (B, T, H, W, 3), "output"),
                                                       P("table", "i32", tuple(table.shape), data=lambda t, g: table.clone(), index_range=1), 3, stats, ws("workspace", n), n, B, T,
                                                       H, W, None])]


def multiscale_crop(fmt):
    from simple_tad_amd import kernels as K, transforms as TF
    B, T, Hs, Ws, S_h, S_w = 2, 2, 9, 11, 4, 6
    rows = [(0, 1, 1, 8, 6, 0, 0), (1, 0, 0, 11, 9, 1, 1)]  # (sample, x0, y0, w, h, hset, vset): a crop inside the frame, the whole frame
    table = K.multiscale_crop_table(rows, [TF.resample_coefficients(w, S_w) for w in (8, 11)], [TF.resample_coefficients(h, S_h) for h in (6, 9)],
                                    B, Hs, Ws, S_h, S_w)
    n = _lib_().tad_multiscale_crop_workspace_bytes(B, 2, 2, S_h, S_w)
    assert table.numel() * 4 == n
    x = lambda: P("x", "u8", (B, T, Hs, Ws, 3), data=lambda t, g: _frames(t, g, (B, T, Hs, Ws, 3)))  # noqa: E731
    tab = lambda: P("workspace", "u8", (n,), data=_table_bytes(table))  # noqa: E731
    return [Case("tad_multiscale_crop", "u8_out", [x(), P("out", "u8", (B, T, S_h, S_w, 3), "output"), 0, None, None, tab(), n, B, T, Hs, Ws, S_h, S_w, 2, 2, None]),
            Case("tad_multiscale_crop", "f32_out", [x(), P("out", "f32", (B, 3, T, S_h, S_w), "output"), 1, MEAN3, STD3, tab(), n, B, T, Hs, Ws, S_h, S_w, 2, 2, None])]


def frame_resize(fmt):
    from simple_tad_amd import frame_resize as FR
    B, T, H, W, S = 2, 2, 9, 11, 6
    table, nv = FR.pad_table([FR.NO_PAD] * B, B, H, W, S, S)
    n = _lib_().tad_frame_resize_workspace_bytes(B, nv, S, S)
    assert table.numel() * 4 == n
    x = lambda: P("x", "u8", (B, T, H, W, 3), data=lambda t, g: _frames(t, g, (B, T, H, W, 3)))  # noqa: E731
    tab = lambda: P("workspace", "u8", (n,), data=_table_bytes(table))  # noqa: E731
    return [Case("tad_frame_resize", "u8_out", [x(), P("out", "u8", (B, T, S, S, 3), "output"), 0, None, None, tab(), n, B, T, H, W, S, S, nv, None]),
            Case("tad_frame_resize", "f32_out", [x(), P("out", "f32", (B, 3, T, S, S), "output"), 1, MEAN3, STD3, tab(), n, B, T, H, W, S, S, nv, None])]


def spatial_sample(fmt):
    from simple_tad_amd import kernels as K
    B, T, H, W, S = 1, 2, 8, 8, 4
    table = K.spatial_sample_table([(0, 1, 1, 6, 6, 4, 4, 0, 0, 0), (1, 0, 0, 8, 8, 5, 6, 1, 1, 1)], B, T, H, W, S)  # crop + resize; resize + crop, flipped
    n = _lib_().tad_spatial_sample_workspace_bytes(B, T)
    assert table.numel() * 4 == n
    tab = lambda: P("workspace", "u8", (n,), data=_table_bytes(table))  # noqa: E731
    return [Case("tad_spatial_sample", "f32_in", [P("x", "f32", (B, 3, T, H, W)), 0, P("out", "f32", (B, 3, T, S, S), "output"), None, None, tab(), n, B, T, H, W, S, None]),
            Case("tad_spatial_sample", "u8_in", [P("x", "u8", (B, T, H, W, 3), data=lambda t, g: _frames(t, g, (B, T, H, W, 3))), 1, P("out", "f32", (B, 3, T, S, S), "output"),
                                                 MEAN3, STD3, tab(), n, B, T, H, W, S, None])]


def gather_rows(fmt):
    return [Case("tad_gather_rows_f32", "small", [P("src", "f32", (7, 12)), P("idx", "i32", (5,), data=idx(5, 7), index_range=7), P("out", "f32", (5, 12), "output"), 5, 12, None])]


def scatter_rows(fmt):
    return [Case("tad_scatter_rows_f32", "small", [P("src", "f32", (5, 12)), P("idx", "i32", (5,), data=idx(5, 7), index_range=7),
                                                   P("out", "f32", (7, 12), "inout", data=lambda t, g: t.zeros(7, 12)), 5, 12, None])]


def mae_assemble(fmt):
    B, nv, nm, D = 2, 3, 2, 12
    return [Case("tad_mae_assemble", "small", [P("x_vis", "f32", (B * nv, D)), P("mask_token", "f32", (D,)), P("pos", "f32", (nv + nm, D)),
                                               P("vis_idx", "i32", (B * nv,), data=lambda t, g: t.tensor([0, 2, 4, 1, 2, 3], dtype=t.int32), index_range=5),
                                               P("mask_idx", "i32", (B * nm,), data=lambda t, g: t.tensor([1, 3, 0, 4], dtype=t.int32), index_range=5),
                                               P("out", "f32", (B, nv + nm, D), "output"), B, nv, nm, D, None])]


def mae_target(fmt):
    B, nm, T, HW, tub, p = 2, 2, 2, 4, 2, 2  # 4 tokens per clip, 8 pixels per (patch, channel)
    return [Case("tad_mae_target", "normalized", [P("videos", "f32", (B, 3, T, HW, HW)), P("mask_idx", "i32", (B * nm,), data=lambda t, g: t.tensor([1, 3, 0, 2], dtype=t.int32), index_range=4),
                                                  P("labels", "f32", (B * nm, tub * p * p * 3), "output"), B, nm, T, HW, HW, tub, p, MEAN3, STD3, 1, None])]


def mse_loss(fmt):
    n = 1028
    return [Case("tad_mse_loss", "grad", [P("pred", "f32", (n,)), P("target", "f32", (n,)), n, P("partials", "f32", (_lib_().tad_mse_loss_blocks(n),), "output"),
                                          P("grad", "f32", (n,), "output"), None])]


def _thr(t, g):
    return t.arange(0, 1.001, 0.25, dtype=t.float32)


def _labels01(n):
    return lambda t, g: t.randint(0, 2, (n,), generator=g, dtype=t.int32)


def _members(n):
    return lambda t, g: t.randint(0, 8, (n,), generator=g, dtype=t.int64)


def threshold_histogram(fmt):
    n, T = 37, 5
    return [Case("tad_threshold_histogram", "small", [P("probs", "f32", (n,), data=lambda t, g: t.rand(n, generator=g)), P("labels", "i32", (n,), data=_labels01(n), index_range=2),
                                                      P("thresholds", "f32", (T,), data=_thr), T, n, P("hist", "i64", (2, T + 1), "output"), None])]


def group_threshold_histogram(fmt):
    n, T, G = 37, 5, 3
    return [Case("tad_group_threshold_histogram", "small", [P("probs", "f32", (n,), data=lambda t, g: t.rand(n, generator=g)), P("labels", "i32", (n,), data=_labels01(n), index_range=2),
                                                            P("member", "i64", (n,), data=_members(n), index_range=8), G, P("thresholds", "f32", (T,), data=_thr), T, n,
                                                            P("hist", "i64", (G, 2, T + 1), "output"), None])]


def group_rank_stats(fmt):
    n, G = 37, 3
    return [Case("tad_group_rank_stats", "small", [P("labels_sorted", "i32", (n,), data=_labels01(n), index_range=2), P("member_sorted", "i64", (n,), data=_members(n), index_range=8),
                                                   P("run_end", "u8", (n,), data=lambda t, g: t.cat([t.randint(0, 2, (n - 1,), generator=g, dtype=t.uint8), t.ones(1, dtype=t.uint8)])),
                                                   G, n, P("out_int", "i64", (G, 3), "output"), P("out_ap", "f64", (G,), "output"), None])]


def fbits(v):
    """the int32 that holds the bit pattern of the f32 value v (plan tables carry their coefficients that way)"""
    import struct
    return struct.unpack("<i", struct.pack("<f", v))[0]


def _i32(rows):
    return lambda t, g: t.tensor(rows, dtype=t.int32)


def _i64(vals):
    return lambda t, g: t.tensor(vals, dtype=t.int64)


def _mix_plan(T, H, W):
    """sample 0 blends with its partner, sample 1 takes a box of it (include/tad_mi355x.h: TAD_MIXUP_PLAN_WORDS)"""
    return [[_lib.MIX_BLEND, fbits(0.7), fbits(0.3), 0, 0, 0, 0, 0, 0, fbits(0.7), fbits(0.3), 0],
            [_lib.MIX_PASTE, fbits(1.0), fbits(0.0), 0, min(T, 1), 1, min(H, 3), 1, min(W, 4), fbits(0.8), fbits(0.2), 0]]


def mixup_clips(fmt):
    out = []
    for W, cid in ((8, "vector_width"), (6, "element_width")):  # the float4 path needs W % 4 == 0 besides a 16-byte aligned x
        B, C_, T, H = 2, 3, 2, 4
        out.append(Case("tad_mixup_clips", cid, [P("x", "f32", (B, C_, T, H, W), "inout"), P("plan", "i32", (B, _lib.MIXUP_PLAN_WORDS), data=_i32(_mix_plan(T, H, W)), index_range=1),
                                                 B, C_, T, H, W, None]))
    return out


def mixup_target(fmt):
    B, ncls = 2, 5
    return [Case("tad_mixup_target", "small", [P("plan", "i32", (B, _lib.MIXUP_PLAN_WORDS), data=_i32(_mix_plan(2, 4, 8)), index_range=1),
                                               P("labels", "i64", (B,), data=_i64([3, 0]), index_range=ncls), P("out", "f32", (B, ncls), "output"), B, ncls, 0.92, 0.02, None])]


def soft_target_ce(fmt):
    B, ncls = 3, 5
    soft = lambda t, g: t.softmax(t.randn(B, ncls, generator=g), 1)  # noqa: E731
    mk = lambda target, labels, sm: [P("logits", "f32", (B, ncls)), target, labels, sm, P("loss", "f32", (1,), "output"), P("dlogits", "f32", (B, ncls), "output"), B, ncls, None]  # noqa: E731
    return [Case("tad_soft_target_ce", "target", mk(P("target", "f32", (B, ncls), data=soft), None, 0.0)),
            Case("tad_soft_target_ce", "labels", mk(None, P("labels", "i64", (B,), data=_i64([4, 0, 2]), index_range=ncls), 0.1))]


def frame_loss(fmt):
    B = 5
    K = _lib.FRAME_LOSS_KINDS
    labels = lambda n: P("labels", "i64", (B,), data=_i64([1, 0, 1, 0, 0] if n == 2 else [2, 0, 1, 2, 1]), index_range=n)  # noqa: E731

    def mk(kind, ncls, lab=None, soft=None, ttc=None, ca=None):
        return [K[kind], P("logits", "f32", (B, ncls)), lab, soft, ttc, ca, 0.25, 2.0, 1.0, 0.1, 0.5, 0.01, P("loss", "f32", (1,), "output"),
                P("dlogits", "f32", (B, ncls), "output"), B, ncls, None]
    return [Case("tad_frame_loss", "focal", mk("focal", 3, labels(3))),
            Case("tad_frame_loss", "focal2", mk("focal2", 3, labels(3), ca=P("class_alpha", "f32", (3,), data=const(0.2, 0.5, 0.3)))),
            Case("tad_frame_loss", "exponential", mk("exponential", 3, labels(3), ttc=P("ttc", "f32", (B,), data=const(-1.5, 0.0, 2.0, 0.5, -0.25)))),
            Case("tad_frame_loss", "2bce", mk("2bce", 2, soft=P("soft", "f32", (B, 2), data=lambda t, g: t.rand(B, 2, generator=g)))),
            Case("tad_frame_loss", "smoothap", mk("smoothap", 2, labels(2)))]


def erase_clips(fmt):
    B, C_, T, H, W = 2, 3, 2, 4, 6
    boxes = [[0, _lib.ERASE_PIXEL, 0, 2, 1, 3, 1, 5], [1, _lib.ERASE_RAND, 0, 1, 0, 4, 2, 6], [1, _lib.ERASE_CONST, 1, 2, 2, 4, 0, 3]]
    return [Case("tad_erase_clips", "three_boxes", [P("x", "f32", (B, C_, T, H, W), "inout"), P("boxes", "i32", (3, _lib.ERASE_BOX_WORDS), data=_i32(boxes), index_range=1),
                                                    3, 77, B, C_, T, H, W, None])]


def frames_to_clip(fmt):
    out = []
    for (H, W), cid in (((4, 4), "vector_width"), ((3, 5), "element_width")):  # 16-byte stores need whole planes of 4 floats
        B, T = 2, 2
        out.append(Case("tad_frames_to_clip", cid, [P("x", "u8", (B, T, H, W, 3), data=lambda t, g, sh=(B, T, H, W, 3): _frames(t, g, sh)),
                                                    P("out", "f32", (B, 3, T, H, W), "output"), MEAN3, STD3, B, T, H, W, None]))
    return out


BUILDERS = {
    "tad_cast_f32_bf16": cast, "tad_transpose_cast_f32_bf16": transpose_cast, "tad_transpose_bf16_batched": transpose_batched,
    "tad_im2col_tubelets": im2col, "tad_im2col_tubelets_f32": im2col_f32, "tad_im2col_tubelets_16": im2col_16, "tad_im2col_tubelets_u8": im2col_u8,
    "tad_im2col_frame_windows": frame_windows, "tad_patch_embed_fwd": patch_embed_fwd, "tad_patch_embed_fwd_implicit": patch_embed_implicit,
    "tad_patch_embed_gemm": patch_embed_gemm, "tad_patch_embed_bwd": patch_embed_bwd, "tad_layernorm_fwd": layernorm_fwd, "tad_layernorm_bwd": layernorm_bwd,
    "tad_linear_fwd": linear_fwd, "tad_linear_fwd_qkv": linear_fwd_qkv, "tad_linear_bwd_input": linear_bwd_input, "tad_linear_bwd_weight": linear_bwd_weight,
    "tad_linear_bwd_weight_qkv": linear_bwd_weight_qkv, "tad_linear_bwd_weight_pair": linear_bwd_weight_pair, "tad_attn_fwd": attn_fwd, "tad_attn_bwd": attn_bwd,
    "tad_attn_colsum": attn_colsum, "tad_attn_fwd_f32": attn_fwd_f32, "tad_attn_bwd_f32": attn_bwd_f32, "tad_meanpool_fwd": meanpool_fwd,
    "tad_meanpool_bwd": meanpool_bwd, "tad_colsum_segments": colsum_segments, "tad_pooled_linear": pooled_linear, "tad_gelu_grad_bcast": gelu_grad_bcast,
    "tad_colsum_bf16": colsum_16, "tad_colsum_window_f32": colsum_window, "tad_colsum_f32": colsum_f32, "tad_scale_cast_bf16": scale_cast,
    "tad_split_bf16x3": split3, "tad_gelu_f32": gelu_f32, "tad_gelu_bwd_f32": gelu_bwd_f32, "tad_rowscale_transpose_cast": rowscale_transpose_cast,
    "tad_layerscale_grads": layerscale_grads, "tad_branch_dropout_fwd": branch_dropout_fwd, "tad_branch_dropout_cast": branch_dropout_cast,
    "tad_sumsq_f32": sumsq, "tad_grad_norm_coef": grad_norm_coef, "tad_grad_segnorm": grad_segnorm, "tad_adamw_step": adamw, "tad_ema_update": ema,
    "tad_randaug_apply": randaug, "tad_multiscale_crop": multiscale_crop, "tad_frame_resize": frame_resize, "tad_spatial_sample": spatial_sample,
    "tad_gather_rows_f32": gather_rows, "tad_scatter_rows_f32": scatter_rows, "tad_mae_assemble": mae_assemble, "tad_mae_target": mae_target,
    "tad_mse_loss": mse_loss, "tad_threshold_histogram": threshold_histogram, "tad_group_threshold_histogram": group_threshold_histogram,
    "tad_group_rank_stats": group_rank_stats, "tad_mixup_clips": mixup_clips, "tad_mixup_target": mixup_target, "tad_soft_target_ce": soft_target_ce,
    "tad_frame_loss": frame_loss, "tad_erase_clips": erase_clips, "tad_frames_to_clip": frames_to_clip,
}

# `any` pointers that no case runs on the GPU: the EMA table holds the addresses of the tensors it updates, so its call is built after
# the placements, by tests/test_alignment_gpu.py::test_ema_tables_at_every_offset; the case above gives its refusals only.
NOT_RUN = {"tad_ema_update": ("tensors",)}


def symbols():
    """every symbol with cases, the _f16 twins included"""
    return [s for s in _lib.SIGNATURES if AC.TWIN_OF.get(s, s) in BUILDERS]


def cases(symbol):
    base = AC.TWIN_OF.get(symbol, symbol)
    fmt = "f16" if symbol in AC.TWIN_OF else "bf16"
    out = BUILDERS[base](fmt)
    for c in out:
        c.symbol, c.fmt = symbol, fmt
    return out
