"""Guard-band runs of the HIP kernels (tests/guarded.py): every operand, every output the production wrapper allocates and every
workspace sits between two poisoned guard bands inside one allocation.  Each case asserts
  (a) no byte outside the writable operands changed (arena.verify());
  (b) the outputs meet the tolerance of that kernel's existing test against the same fp64 oracle expression (constants imported from
      tests/test_kernels_gpu.py; others restated with a pointer to where they come from) -- with every output born NaN, an element
      that is never written fails here;
  (c) the outputs are bit-identical to an unguarded run of the same wrapper on the same inputs made just before: a result that
      depends on bytes the kernel does not own differs (or fails (b)).
Shapes come from the launchers' plan boundaries (tests/test_fuzz_gpu.py M_CHOICES / K_CHOICES, +-1): every tail is non-empty.

What this establishes: no result depends on, and no store lands on, bytes outside the operands.  What it does not: an over-read that is
loaded and then discarded changes nothing and is invisible; "no address outside the operands is ever issued" is NOT shown.

Every wrapper of simple_tad_amd/kernels.py that launches a kernel has a case here; tad_patch_embed_bwd and tad_threshold_histogram have no
wrapper in kernels.py and are called through the C ABI on placements.
"""
import math

import pytest
import torch

from attn_util import prescaled_pair
from guarded import GuardedArena, POISON_MODES, same_bits
from oracle import vit_oracle as O
from test_kernels_gpu import ATT_TOL, ATT_TOL_MAX, BF16_ULP, TOL, _attn_ref, check

pytestmark = pytest.mark.gpu

FMTS = {"bf16": torch.bfloat16, "f16": torch.float16}
# one 16-bit ulp of the tensor scale, the bound the existing tests use for 16-bit outputs (test_kernels_gpu.BF16_ULP = 2^-8; IEEE half
# has three more mantissa bits, so the bf16 bound holds for it a fortiori and no second constant is introduced)
ULP16 = BF16_ULP
poison = pytest.mark.parametrize("poison", POISON_MODES)
fmt = pytest.mark.parametrize("fmt", list(FMTS))


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import _lib, kernels
    _lib.load()
    return kernels


@pytest.fixture(scope="module")
def arena():
    return GuardedArena(448 << 20, "cuda")


class InOut:
    """an operand the kernel updates in place"""

    def __init__(self, t):
        self.t = t


class Idx:
    """an index tensor: its guards hold indices in [0, n)"""

    def __init__(self, t, n):
        self.t, self.n = t, n


def _lib():
    from simple_tad_amd import _lib
    return _lib.load()


def rnd(g, shape, scale=1.0, dtype=torch.float32):
    """values exactly representable in ``dtype`` (the oracle sees what the kernel sees), returned as f32"""
    return (torch.randn(shape, generator=g) * scale).to(dtype).float()


def guarded(K, arena, mode, fn, bitwise=True, **ops):
    """fn(**tensors) -> tuple of tensors (None allowed; in-place operands included).  Runs fn on plain device copies, then on arena
    placements with the wrappers' allocations routed into the arena; asserts (a) and (c); returns the guarded outputs for (b)."""
    raw = {k: (v.t if isinstance(v, (InOut, Idx)) else v) for k, v in ops.items()}
    plain = fn(**{k: (v.cuda().clone() if isinstance(v, torch.Tensor) else v) for k, v in raw.items()})
    torch.cuda.synchronize()
    plain = [None if t is None else t.clone() for t in plain]
    arena.reset(mode)
    placed = {}
    for k, v in ops.items():
        if isinstance(v, Idx):
            placed[k] = arena.place(v.t, index_range=v.n, name=k)
        elif isinstance(v, InOut):
            placed[k] = arena.place(v.t, role="inout", name=k)
        elif isinstance(v, torch.Tensor):
            placed[k] = arena.place(v, name=k)
        else:
            placed[k] = v
    with arena.route(K):
        got = fn(**placed)
    arena.verify()
    assert len(got) == len(plain)
    for i, t in enumerate(got):  # (0-dim: a value torch computed from a kernel's partials, e.g. the MSE loss)
        assert t is None or t.dim() == 0 or arena.contains(t), f"output {i} was allocated outside the arena: the wrapper took a path the proxy does not see"
    for i, (a, b) in enumerate(zip(plain, got)):
        assert (a is None) == (b is None)
        if a is not None and bitwise:
            assert same_bits(a, b), f"output {i}: the guarded run differs in bits from the unguarded one (the result depends on bytes outside the operands)"
    return [None if t is None else t.clone() for t in got]  # (copies: the next case reuses the arena)


# =============================================================================================== Linear forward
LIN_FWD = [(65, 36, 200), (257, 100, 192), (2047, 264, 320), (2049, 772, 128)]  # N % 4 only / % 8 only; Kd = 200 goes through _pad_reduction


@poison
@fmt
@pytest.mark.parametrize("M,N,Kd", LIN_FWD)
def test_linear_fwd_epilogues(K, arena, M, N, Kd, fmt, poison):
    op = FMTS[fmt]
    g = torch.Generator().manual_seed(M * 7919 + N * 31 + Kd)
    x, w, b = rnd(g, (M, Kd), dtype=op), rnd(g, (N, Kd), 0.05, op), torch.randn(N, generator=g) * 0.1
    ref = x.double() @ w.double().t() + b.double()
    y, _ = guarded(K, arena, poison, lambda x, w, b: K.linear_fwd(x, w, b, out_dtype=torch.float32), x=x.to(op), w=w.to(op), b=b)
    check(y, ref, what="linear bias f32")
    y16, _ = guarded(K, arena, poison, lambda x, w, b: K.linear_fwd(x, w, b), x=x.to(op), w=w.to(op), b=b)
    check(y16.float(), ref, tol=ULP16, what="linear bias 16-bit")
    yg, pre = guarded(K, arena, poison, lambda x, w, b: K.linear_fwd(x, w, b, out_dtype=torch.float32, epilogue=K.EPI_BIAS_GELU, want_preact=True),
                      x=x.to(op), w=w.to(op), b=b)
    check(yg, O.gelu_erf(ref), what="linear gelu")
    check(pre.float(), ref, tol=ULP16, what="linear preact")
    res, gam = torch.randn(M, N, generator=g), torch.randn(N, generator=g) * 0.3 + 1.0
    for rows_per in (7, 300):  # per-row scale loads / one or two scales per tile
        rs = torch.tensor([0.0 if i % 3 == 0 else 1.25 for i in range((M + rows_per - 1) // rows_per)])
        yr, _ = guarded(K, arena, poison,
                        lambda x, w, b, res, gam, rs: K.linear_fwd(x, w, b, out_dtype=torch.float32, epilogue=K.EPI_BIAS_RESIDUAL, residual=res, gamma=gam,
                                                                   rowscale=rs, rows_per_scale=rows_per),
                        x=x.to(op), w=w.to(op), b=b, res=res, gam=gam, rs=rs)
        check(yr, res.double() + rs.double().repeat_interleave(rows_per)[:M, None] * gam.double() * ref, what=f"linear residual, groups of {rows_per}")


PLANS = {"tile": dict(persistent=0, direct_epilogue=0, split_tail=0, splitk_tail=0, short_k=0),
         "persistent": dict(persistent=1, direct_epilogue=0, split_tail=0, splitk_tail=0, short_k=0, variant=3),
         "splitk_deferred": dict(splitk_tail=2, split_tail=2, splitk_defer=1), "splitk_in_launch": dict(splitk_tail=2, split_tail=2, splitk_defer=0)}


@poison
@pytest.mark.parametrize("mode", ["plain", "res"])
@pytest.mark.parametrize("plan", list(PLANS))
def test_linear_fwd_plans(K, arena, plan, mode, poison):
    """per-tile, persistent (544 tiles of 256 x 128 > 1.5 per CU) and split-K tail plans (32 whole row panels + a ragged tail of 2 x 8
    tiles, both forms of the combine) on a ragged M; the split-K scratch is the wrapper's own exact-size allocation."""
    M, N, Kd = 33 * 256 + 37, 2048, 512
    g = torch.Generator().manual_seed(M + N)
    x, w, b = rnd(g, (M, Kd), dtype=torch.bfloat16), rnd(g, (N, Kd), 0.05, torch.bfloat16), torch.randn(N, generator=g) * 0.1
    res = torch.randn(M, N, generator=g) if mode == "res" else None
    launches = []

    def run(x, w, b, res):
        n0 = K.linear_kernel_launches()
        out = (K.linear_fwd(x, w, b, out_dtype=torch.float32, epilogue=K.EPI_BIAS_RESIDUAL, residual=res) if mode == "res" else K.linear_fwd(x, w, b))
        launches.append(K.linear_kernel_launches() - n0)
        return out

    try:
        K.linear_tuning(**{**K.LINEAR_TUNING_DEFAULTS, **PLANS[plan]})
        y, _ = guarded(K, arena, poison, run, x=x.to(torch.bfloat16), w=w.to(torch.bfloat16), b=b, res=res)
    finally:
        K.linear_tuning(**K.LINEAR_TUNING_DEFAULTS)
    if plan.startswith("splitk"):
        assert launches == [3 if plan == "splitk_deferred" else 2] * 2, f"the split-K tail plan was not taken: {launches}"
    ref = x.double() @ w.double().t() + b.double() + (res.double() if mode == "res" else 0.0)
    check(y.float(), ref, tol=TOL if mode == "res" else ULP16, what=f"linear {plan} {mode}")


@poison
@fmt
@pytest.mark.parametrize("M,D,Kd", [(257, 40, 192), (2049, 200, 320)])
def test_linear_fwd_qkv(K, arena, M, D, Kd, fmt, poison):
    op = FMTS[fmt]
    g = torch.Generator().manual_seed(M + D)
    x, w = rnd(g, (M, Kd), dtype=op), rnd(g, (3 * D, Kd), 0.05, op)
    qb, vb = torch.randn(D, generator=g) * 0.1, torch.randn(D, generator=g) * 0.1
    pre = K.q_prescale_of(D ** -0.5)
    ref = x.double() @ w.double().t() + torch.cat([qb, torch.zeros(D), vb]).double()
    ref[:, :D] *= pre
    for od, tol in ((torch.float32, TOL), (None, ULP16)):
        y = guarded(K, arena, poison, lambda x, w, qb, vb: (K.linear_fwd_qkv(x, w, qb, vb, out_dtype=od, q_prescale=pre),), x=x.to(op), w=w.to(op), qb=qb, vb=vb)[0]
        for i in range(3):  # (per third: the pre-scaled q third has its own scale)
            check(y.float()[:, i * D:(i + 1) * D], ref[:, i * D:(i + 1) * D], tol=tol, what=f"qkv third {i}")


# =============================================================================================== Linear backward
LIN_BWD = [(257, 120, 200), (2049, 264, 392), (5003, 768, 256)]  # N, Kd off 128 (N % 3 == 0 for the qkv split; N = 120, 264 off the 64-deep K-tile of dX)


@poison
@fmt
@pytest.mark.parametrize("w4", [1, 0], ids=["four_wave", "two_wave"])
@pytest.mark.parametrize("M,N,Kd", LIN_BWD)
def test_linear_bwd(K, arena, M, N, Kd, w4, fmt, poison):
    """dx = dy W (also through GELU'), dW = dy^T x, db = colsum(dy): the reduction over a ragged M must stop at M"""
    op = FMTS[fmt]
    g = torch.Generator().manual_seed(M * 104729 + N * 17 + Kd)
    dy, w, x = rnd(g, (M, N), dtype=op), rnd(g, (N, Kd), 0.05, op), rnd(g, (M, Kd), dtype=op)
    h = rnd(g, (M, Kd), 1.5, op)
    wT = w.t().contiguous()
    ref_dx = dy.double() @ w.double()
    ref_dW, ref_db = dy.double().t() @ x.double(), dy.double().sum(0)
    try:
        K.linear_tuning(tn_w4=w4)
        if w4:  # (the input-gradient GEMM does not depend on the tn_w4 knob)
            dx = guarded(K, arena, poison, lambda dy, wT: (K.linear_bwd_input(dy, wT, out_dtype=torch.float32),), dy=dy.to(op), wT=wT.to(op))[0]
            check(dx, ref_dx, what="linear dx")
            hd = h.double().requires_grad_()
            O.gelu_erf(hd).backward(ref_dx)
            dxg = guarded(K, arena, poison, lambda dy, wT, h: (K.linear_bwd_input(dy, wT, out_dtype=torch.float32, gelu_preact=h),), dy=dy.to(op), wT=wT.to(op), h=h.to(op))[0]
            check(dxg, hd.grad, what="linear dx through gelu")
        dW, db = guarded(K, arena, poison, lambda dy, x: K.linear_bwd_weight(dy, x), dy=dy.to(op), x=x.to(op))
        check(dW, ref_dW, what="linear dW")
        check(db, ref_db, what="linear db")
        dW0 = torch.randn(N, Kd, generator=g)
        dWa = guarded(K, arena, poison, lambda dy, x, dW: K.linear_bwd_weight(dy, x, want_bias=False, dW=dW, accumulate=True)[:1], dy=dy.to(op), x=x.to(op), dW=InOut(dW0))[0]
        check(dWa, dW0.double() + ref_dW, what="linear dW accumulate")
        # qkv: bias column sums split into the first / last third, in place
        dq0, dv0 = torch.randn(N // 3, generator=g), torch.randn(N // 3, generator=g)

        def qkv(dy, x, dW, dq, dv):
            K.linear_bwd_weight_qkv(dy, x, dW, dq, dv, True)
            return dW, dq, dv
        dWq, dq, dv = guarded(K, arena, poison, qkv, dy=dy.to(op), x=x.to(op), dW=InOut(dW0), dq=InOut(dq0), dv=InOut(dv0))
        check(dWq, dW0.double() + ref_dW, what="qkv dW")
        check(dq, dq0.double() + ref_db[:N // 3], what="dq_bias")
        check(dv, dv0.double() + ref_db[2 * N // 3:], what="dv_bias")
        # pair: a second problem over the same rows and K
        N2 = 136
        dy2, x2 = rnd(g, (M, N2), dtype=op), rnd(g, (M, Kd), dtype=op)

        def pair(dy1, x1, dW1, db1, dy2, x2, dW2):
            K.linear_bwd_weight_pair(dy1, x1, dW1, db1, None, dy2, x2, dW2, False)
            return dW1, db1, dW2
        dW1, db1, dW2 = guarded(K, arena, poison, pair, dy1=dy.to(op), x1=x.to(op), dW1=InOut(torch.full((N, Kd), float("nan"))), db1=InOut(torch.full((N,), float("nan"))),
                                dy2=dy2.to(op), x2=x2.to(op), dW2=InOut(torch.full((N2, Kd), float("nan"))))
        check(dW1, ref_dW, what="pair dW1")
        check(db1, ref_db, what="pair db1")
        check(dW2, dy2.double().t() @ x2.double(), what="pair dW2")
    finally:
        K.linear_tuning(**K.LINEAR_TUNING_DEFAULTS)


@poison
@pytest.mark.parametrize("M,N", [(1, 4), (255, 16), (1027, 20), (2049, 776)])
def test_colsums(K, arena, M, N, poison):
    g = torch.Generator().manual_seed(M + N)
    a = torch.randn(M, N, generator=g)
    out = guarded(K, arena, poison, lambda a: (K.colsum_f32(a),), a=a)[0]
    check(out, a.double().sum(0), tol=1e-5, what="colsum_f32")  # (tolerances: test_meanpool_colsum_scale_sumsq / test_colsum_f32_shapes)
    if N % 8 == 0:  # (the 16-bit column sums take whole 16-byte chunks)
        for f, op in FMTS.items():
            a16 = a.to(op)
            out = guarded(K, arena, poison, lambda a: (K.colsum_bf16(a),), a=a16)[0]
            check(out, a16.double().sum(0), tol=1e-5, what=f"colsum {f}")
    B, R = 3, max(M // 3, 1)
    a3 = torch.randn(B, R, N, generator=g)
    r0, rc = R // 3, R - R // 3  # the window ends with the last row of the last batch entry
    out = guarded(K, arena, poison, lambda a: (K.colsum_window_f32(a, r0, rc),), a=a3)[0]
    check(out, a3[:, r0:r0 + rc].double().sum((0, 1)), tol=1e-5, what="colsum_window_f32")


# =============================================================================================== attention
ATT = [(2, 1, 3, 64), (3, 8, 1, 64), (1, 129, 1, 64), (2, 393, 3, 80), (1, 1568, 2, 64), (2, 129, 2, 80)]  # B, N, H, d: the last batch entry's key tail ends the tensor


@poison
@fmt
@pytest.mark.parametrize("prescaled", [True, False], ids=["q_prescaled", "plain_q"])
@pytest.mark.parametrize("B,N,H,d", ATT)
def test_attention_16bit(K, arena, B, N, H, d, prescaled, fmt, poison):
    op = FMTS[fmt]
    scale = d ** -0.5
    g = torch.Generator().manual_seed(B * 1000 + N)
    rt = lambda t: t.to(op).float()  # noqa: E731
    qkv, dout = rnd(g, (B * N, 3 * H * d), dtype=op), rnd(g, (B * N, H * d), dtype=op)
    opnd = qkv
    if prescaled:
        opnd, qkv = prescaled_pair(qkv, B, N, H, scale, rt, d=d)
    ref, ref_dqkv = _attn_ref(qkv, B, N, H, scale, dout)
    kw = dict(q_prescaled=prescaled, d=d)
    out32, lse32 = guarded(K, arena, poison, lambda qkv: K.attn_fwd(qkv, B, N, H, scale, out_dtype=torch.float32, **kw), qkv=opnd.to(op))
    check(out32.reshape(B, N, -1), ref, tol=ATT_TOL, tol_max=ATT_TOL_MAX, what="attn fwd f32")
    found = K.attn_tuning_get("fwd_q64")
    for q64 in ((0, 1) if d == 64 else (0,)):
        try:
            K.attn_tuning(fwd_q64=q64)
            out, lse, lo = guarded(K, arena, poison, lambda qkv: K.attn_fwd(qkv, B, N, H, scale, want_lo=True, **kw), qkv=opnd.to(op))
        finally:
            K.attn_tuning(fwd_q64=found)
        # (random inputs: the bound of tests/test_fuzz_gpu.py::test_attention_random_shapes for the 16-bit forward, 4e-3 + half an ulp, on both norms)
        check(out.float().reshape(B, N, -1), ref, tol=4e-3 + ULP16 / 2, what=f"attn fwd 16-bit (fwd_q64={q64})")
        assert same_bits(lse, lse32) and torch.equal(lo.float(), (out32 - out.float()).to(op).float()), "lse / out_lo"
    for use_lo in (False, True):
        dqkv = guarded(K, arena, poison, lambda qkv, out, dout, lse, lo: (K.attn_bwd(qkv, out, dout, lse, B, N, H, scale, out_lo=lo, **kw),),
                       qkv=opnd.to(op), out=out.cpu(), dout=dout.to(op), lse=lse.cpu(), lo=lo.cpu() if use_lo else None)[0]
        # tad_attn_bwd_scratch_bytes: the wrapper's delta is a placement of exactly the declared size (nothing rounds it up)
        assert [p.end - p.start for p in arena.placements if p.name.startswith("wrapper") and p.dtype == torch.float32] == [_lib().tad_attn_bwd_scratch_bytes(B, N, H)]
        gq, r = dqkv.float().cpu().reshape(B, N, 3, H, d), ref_dqkv.reshape(B, N, 3, H, d)
        if N == 1:  # (one key: dq = dk = 0 exactly, no scale of their own -- the whole tensor, as tests/test_fuzz_gpu.py compares it)
            check(gq, r, tol=2 * ULP16, what=f"attn dqkv (out_lo={use_lo})")
            continue
        for i, nm in enumerate("qkv"):
            check(gq[:, :, i], r[:, :, i], tol=2 * ULP16, what=f"attn d{nm} (out_lo={use_lo})")


@poison
@pytest.mark.parametrize("B,N,H,d", [(2, 8, 3, 64), (1, 393, 3, 80), (2, 129, 1, 64)])
def test_attention_f32(K, arena, B, N, H, d, poison):
    scale = d ** -0.5
    g = torch.Generator().manual_seed(N)
    qkv, dout = torch.randn(B * N, 3 * H * d, generator=g), torch.randn(B * N, H * d, generator=g)
    ref, ref_dqkv = _attn_ref(qkv, B, N, H, scale, dout)
    out, lse = guarded(K, arena, poison, lambda qkv: K.attn_fwd_f32(qkv, B, N, H, scale, want_lse=True, d=d), qkv=qkv)
    check(out.reshape(B, N, -1), ref, what="attn_f32 fwd")  # (TOL: test_attention_f32_fwd_bwd)
    dqkv = guarded(K, arena, poison, lambda qkv, out, dout, lse: (K.attn_bwd_f32(qkv, out, dout, lse, B, N, H, scale, d=d),),
                   qkv=qkv, out=out.cpu(), dout=dout, lse=lse.cpu())[0]
    check(dqkv.reshape(B, N, -1), ref_dqkv, what="attn_f32 bwd")


@poison
@fmt
@pytest.mark.parametrize("prescaled", [True, False], ids=["q_prescaled", "plain_q"])
@pytest.mark.parametrize("B,N,H,d", [(2, 129, 2, 64), (1, 393, 1, 80)])
def test_attention_dropout(K, arena, B, N, H, d, prescaled, fmt, poison):
    """p > 0 against the oracle with the kernels' counter-based keep mask injected (O.attention_core(drop_p, seed)); expressions and bounds of
    test_attention_dropout_16bit_kernels_vs_oracle_with_the_injected_mask / test_attention_dropout_f32_vs_oracle_with_the_injected_mask"""
    op = FMTS[fmt]
    scale, p, seed = d ** -0.5, 0.25, 7654321
    g = torch.Generator().manual_seed(N)
    rt = lambda t: t.to(op).float()  # noqa: E731
    qkv, dout = rnd(g, (B * N, 3 * H * d), dtype=op), rnd(g, (B * N, H * d), dtype=op)
    opnd = qkv
    if prescaled:
        opnd, qkv = prescaled_pair(qkv, B, N, H, scale, rt, d=d)
    qd = qkv.double().reshape(B, N, -1).requires_grad_()
    ref = O.attention_core(qd, H, scale, drop_p=p, seed=seed)
    ref.backward(dout.double().reshape(B, N, -1))
    kw = dict(q_prescaled=prescaled, drop_p=p, seed=seed, d=d)
    tol, tol_max = (ATT_TOL, ATT_TOL_MAX) if fmt == "bf16" else (6e-4, 1.2e-3)
    out32, lse = guarded(K, arena, poison, lambda qkv: K.attn_fwd(qkv, B, N, H, scale, out_dtype=torch.float32, **kw), qkv=opnd.to(op))
    check(out32.reshape(B, N, -1), ref, tol=tol, tol_max=tol_max, what="attn dropout fwd")
    q4 = qkv.double().reshape(B, N, 3, H, d)
    sc = torch.einsum("bnhd,bmhd->bhnm", q4[:, :, 0], q4[:, :, 1]) * scale
    assert (lse.cpu().double() - torch.logsumexp(sc, -1)).abs().max().item() < 1e-3  # (the full softmax's, whatever was dropped)
    out16, lse, lo = guarded(K, arena, poison, lambda qkv: K.attn_fwd(qkv, B, N, H, scale, want_lo=True, **kw), qkv=opnd.to(op))
    dqkv = guarded(K, arena, poison, lambda qkv, out, dout, lse, lo: (K.attn_bwd(qkv, out, dout, lse, B, N, H, scale, out_lo=lo, **kw),),
                   qkv=opnd.to(op), out=out16.cpu(), dout=dout.to(op), lse=lse.cpu(), lo=lo.cpu())[0]
    gq, r = dqkv.float().cpu().reshape(B, N, 3, H, d), qd.grad.reshape(B, N, 3, H, d)
    for i, nm in enumerate("qkv"):
        check(gq[:, :, i], r[:, :, i], tol=2 * (BF16_ULP if fmt == "bf16" else 2 * tol), what=f"attn dropout d{nm}")
    if prescaled or fmt == "f16":
        return  # (the f32 family has one contract and one format: once per shape and poison mode)
    q32, do32 = torch.randn(B * N, 3 * H * d, generator=g), torch.randn(B * N, H * d, generator=g)
    q32d = q32.double().reshape(B, N, -1).requires_grad_()
    ref32 = O.attention_core(q32d, H, scale, drop_p=p, seed=seed)
    ref32.backward(do32.double().reshape(B, N, -1))
    o32, l32 = guarded(K, arena, poison, lambda qkv: K.attn_fwd_f32(qkv, B, N, H, scale, want_lse=True, d=d, drop_p=p, seed=seed), qkv=q32)
    check(o32.reshape(B, N, -1), ref32, tol=1e-5, what="attn_f32 dropout fwd")
    dq32 = guarded(K, arena, poison, lambda qkv, out, dout, lse: (K.attn_bwd_f32(qkv, out, dout, lse, B, N, H, scale, d=d, drop_p=p, seed=seed),),
                   qkv=q32, out=o32.cpu(), dout=do32, lse=l32.cpu())[0]
    check(dq32.reshape(B, N, -1), q32d.grad, tol=2e-5, what="attn_f32 dropout bwd")


# =============================================================================================== LayerNorm, pooling
@poison
@fmt
@pytest.mark.parametrize("rows,D", [(5, 4), (33, 252), (201, 1000), (31, 1280), (5, 1792), (1569, 2048)])
def test_layernorm(K, arena, rows, D, fmt, poison):
    op = FMTS[fmt]
    g = torch.Generator().manual_seed(rows + D)
    x = torch.randn(rows, D, generator=g) * 2 + 0.5
    w, b = torch.randn(D, generator=g) * 0.2 + 1, torch.randn(D, generator=g) * 0.1
    dy, dres = rnd(g, (rows, D), dtype=op), torch.randn(rows, D, generator=g)
    xd, wd, bd = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    ref = O.layer_norm(xd, wd, bd, 1e-6)
    ref.backward(dy.double())
    y32, mean, rstd = guarded(K, arena, poison, lambda x, w, b: K.layernorm_fwd(x, w, b, 1e-6, out_dtype=torch.float32), x=x, w=w, b=b)
    check(y32, ref, what="ln fwd f32")
    check(mean, x.double().mean(-1), what="ln mean")
    y16 = guarded(K, arena, poison, lambda x, w, b: K.layernorm_fwd(x, w, b, 1e-6, out_dtype=op, save_stats=False), x=x, w=w, b=b)[0]
    check(y16.float(), ref, tol=ULP16, what="ln fwd 16-bit")
    ref_dx = xd.grad + dres.double()
    dx, dxb, dg, db, cs = guarded(K, arena, poison,
                                  lambda dy, x, w, mean, rstd, dres: K.layernorm_bwd(dy, x, w, mean, rstd, dres=dres, want_bf16=True, want_colsum=True),
                                  dy=dy.to(op), x=x, w=w, mean=mean.cpu(), rstd=rstd.cpu(), dres=dres)
    check(dx, ref_dx, what="ln dx")
    check(dxb.float(), ref_dx, tol=ULP16, what="ln dx 16-bit")
    check(dg, wd.grad, what="ln dgamma")
    check(db, bd.grad, what="ln dbeta")
    check(cs, ref_dx.sum(0), what="ln colsum")
    # f32 dy, per-sample row scale on the 16-bit copy and the column sums, reductions accumulated into existing sinks
    rows_per = 7
    rs = torch.tensor([0.0 if i % 3 == 0 else 1.25 for i in range((rows + rows_per - 1) // rows_per)])
    s0 = [torch.randn(D, generator=g) for _ in range(3)]

    def bwd_into(dy, x, w, mean, rstd, rs, dg, db, cs):
        return K.layernorm_bwd(dy, x, w, mean, rstd, want_bf16=True, want_colsum=True, rowscale=rs, rows_per_scale=rows_per, into=(dg, db, cs))
    dx2, dxb2, dg2, db2, cs2 = guarded(K, arena, poison, bwd_into, dy=dy, x=x, w=w, mean=mean.cpu(), rstd=rstd.cpu(), rs=rs,
                                       dg=InOut(s0[0]), db=InOut(s0[1]), cs=InOut(s0[2]))
    scaled = xd.grad * rs.double().repeat_interleave(rows_per)[:rows, None]
    check(dx2, xd.grad, what="ln dx (f32 dy)")
    check(dxb2.float(), scaled, tol=ULP16, what="ln scaled 16-bit dx")
    check(dg2, s0[0].double() + wd.grad, what="ln dgamma into")
    check(db2, s0[1].double() + bd.grad, what="ln dbeta into")
    check(cs2, s0[2].double() + scaled.sum(0), what="ln colsum into")


@poison
@pytest.mark.parametrize("B,N,D", [(3, 197, 252), (1, 5, 4), (5, 393, 1000)])
def test_meanpool(K, arena, B, N, D, poison):
    g = torch.Generator().manual_seed(N)
    x, dy = torch.randn(B, N, D, generator=g), torch.randn(B, D, generator=g)
    y = guarded(K, arena, poison, lambda x: (K.meanpool_fwd(x),), x=x)[0]
    check(y, x.double().mean(1), tol=1e-5, what="meanpool fwd")  # (tolerances: test_meanpool_colsum_scale_sumsq)
    dx, dxb = guarded(K, arena, poison, lambda dy: K.meanpool_bwd(dy, N, want_bf16=True), dy=dy)
    ref = (dy.double() / N)[:, None, :].expand(B, N, D)
    check(dx, ref, tol=1e-6, what="meanpool bwd")
    check(dxb.float(), ref, tol=ULP16, what="meanpool bwd 16-bit")


# =============================================================================================== patch embedding
@poison
@fmt
@pytest.mark.parametrize("B,T,HW,patch,D", [(3, 4, 28, 14, 200), (1, 2, 32, 16, 200), (5, 2, 48, 16, 64)])
def test_patch_embedding(K, arena, B, T, HW, patch, D, fmt, poison):
    """patch 14: K = 1176 padded to ldk = 1216 -- the padded columns of cols must be written (zero), nothing behind them; the pos table
    has ntok rows (the residual row is taken modulo ntok), not B * ntok"""
    op = FMTS[fmt]
    g = torch.Generator().manual_seed(HW + B)
    x = torch.randn(B, 3, T, HW, HW, generator=g)
    x16 = x.to(op).float()
    Kc = 3 * 2 * patch * patch
    ldk = K.patch_embed_ldk(3, 2, patch)
    ntok = (T // 2) * (HW // patch) ** 2
    ref_cols = O.im2col_tubelets(x16, 2, patch).reshape(B * ntok, Kc)
    cols = guarded(K, arena, poison, lambda x: (K.im2col_tubelets(x, 2, patch, dtype=op),), x=x)[0]
    assert cols.shape == (B * ntok, ldk) and torch.equal(cols[:, :Kc].float().cpu(), ref_cols) and not cols[:, Kc:].float().any()
    c32 = guarded(K, arena, poison, lambda x: (K.im2col_tubelets_f32(x, 2, patch),), x=x)[0]
    assert torch.equal(c32[:, :Kc].cpu(), O.im2col_tubelets(x, 2, patch).reshape(B * ntok, Kc)) and not c32[:, Kc:].any()
    # uint8 frames [B,T,H,W,3], both channel orders (tests/test_input_stage.py: normalised then rounded like the f32 route)
    frames = torch.randint(0, 256, (B, T, HW, HW, 3), generator=g, dtype=torch.uint8)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    for bgr in (False, True):
        cu = guarded(K, arena, poison, lambda f: (K.im2col_tubelets_u8(f, 2, patch, mean, std, bgr=bgr, dtype=op),), f=frames)[0]
        fr = frames.flip(-1) if bgr else frames
        xn = ((fr.double() / 255.0 - torch.tensor(mean).double()) / torch.tensor(std).double()).permute(0, 4, 1, 2, 3)
        check(cu[:, :Kc].float(), O.im2col_tubelets(xn, 2, patch).reshape(B * ntok, Kc), tol=ULP16, what=f"im2col_u8 bgr={bgr}")
        assert not cu[:, Kc:].float().any()
    w, b = rnd(g, (D, Kc), 0.02, op), torch.randn(D, generator=g) * 0.02
    pos = O.sinusoid_table(ntok, D)[0].float()
    out, cols2 = guarded(K, arena, poison, lambda x, w, b, pos: K.patch_embed_fwd(x, K.pad_k(w, ldk), b, pos, 2, patch), x=x, w=w.to(op), b=b, pos=pos)
    ref = O.patch_embed(x16.double(), w.double().reshape(D, 3, 2, patch, patch), b.double(), 2, patch) + pos.double()
    check(out, ref, what="patch_embed_fwd")  # (TOL: test_patch_embed_fwd)
    assert same_bits(cols2, cols)
    # the GEMM alone on a caller-supplied cols with the padded ldk; the pos residual has ntok rows, taken modulo ntok over the B * ntok rows
    wp = torch.nn.functional.pad(w, (0, ldk - Kc)).to(op)
    out_g = guarded(K, arena, poison, lambda cols, w, b, pos: (K.patch_embed_gemm(cols, w, b, pos, ntok),), cols=cols.cpu(), w=wp, b=b, pos=pos)[0]
    check(out_g, ref, what="patch_embed_gemm")
    assert same_bits(out_g, out)
    if patch == 16:  # the forward that reads the clip itself: the bits of the explicit route (test_patch_embed_implicit_gemm_is_bit_identical_...)
        out_i = guarded(K, arena, poison, lambda x, w, b, pos: (K.patch_embed_fwd_implicit(x, w, b, pos, 2, patch),), x=x, w=w.to(op), b=b, pos=pos)[0]
        check(out_i, ref, what="patch_embed_fwd_implicit")
        assert same_bits(out_i, out)
    # tad_patch_embed_bwd (C ABI; the Conv3d weight gradient on the padded patch matrix): dW [D, ldk], db [D], workspace of exactly the declared size
    from simple_tad_amd import _lib as L
    lib = L.load()
    M = B * ntok
    dy = rnd(g, (M, D), 0.1, op)
    fn = getattr(lib, L.F16_TWINS["tad_patch_embed_bwd"] if op == torch.float16 else "tad_patch_embed_bwd")
    nb = lib.tad_patch_embed_bwd_workspace_bytes(M, D, ldk)
    st = torch.cuda.current_stream().cuda_stream
    plain = [dy.to(op).cuda(), cols.clone(), torch.empty(D, ldk, device="cuda"), torch.empty(D, device="cuda"), torch.empty(nb, dtype=torch.uint8, device="cuda")]
    assert fn(*[t.data_ptr() for t in plain], nb, M, D, ldk, st) == 0, lib.tad_last_error_string()
    arena.reset(poison)
    placed = [arena.place(dy.to(op), name="dy"), arena.place(cols.cpu(), name="cols"), arena.place((D, ldk), torch.float32, role="output", name="dW"),
              arena.place((D,), torch.float32, role="output", name="db"), arena.place((nb,), torch.uint8, role="workspace", name="workspace")]
    assert fn(*[t.data_ptr() for t in placed], nb, M, D, ldk, st) == 0, lib.tad_last_error_string()
    arena.verify()
    check(placed[2], dy.double().t() @ cols.float().double().cpu(), what="patch_embed_bwd dW")  # (TOL: test_patch_embed_bwd_entry_point_is_the_weight_gradient_gemm)
    check(placed[3], dy.double().sum(0), what="patch_embed_bwd db")
    assert same_bits(placed[2], plain[2]) and same_bits(placed[3], plain[3])


# =============================================================================================== casts, transposes
@poison
@fmt
@pytest.mark.parametrize("R,Cc", [(1, 4), (33, 12), (65, 132), (257, 68)])
def test_casts(K, arena, R, Cc, fmt, poison):
    op = FMTS[fmt]
    g = torch.Generator().manual_seed(R * Cc)
    x = torch.randn(R, Cc, generator=g) * 3
    y = guarded(K, arena, poison, lambda x: (K.cast_op16(x, dtype=op),), x=x)[0]
    assert same_bits(y.cpu(), x.to(op)), "cast: RNE, bit-exact (test_cast_bit_exact)"
    yt = guarded(K, arena, poison, lambda x: (K.transpose_cast_op16(x, dtype=op),), x=x)[0]
    assert same_bits(yt.cpu(), x.t().contiguous().to(op))
    gam = torch.randn(Cc, generator=g) * 0.1 + 1
    rs = torch.tensor([0.0 if i % 3 == 0 else 1.25 for i in range((R + 9) // 10)])
    sc = guarded(K, arena, poison, lambda x, gam, rs: (K.scale_cast_op16(x, gam, rs, 10, dtype=op),), x=x, gam=gam, rs=rs)[0]
    check(sc.float(), x.double() * gam.double() * rs.double().repeat_interleave(10)[:R, None], tol=ULP16, what="scale_cast")
    for role_b, stack in ((False, False), (True, False), (False, True)):
        sp = guarded(K, arena, poison, lambda x: (K.split_bf16x3(x, role_b, stack=stack, dtype=op),), x=x)[0].cpu()
        hi = x.to(op)
        lo = (x - hi.float()).to(op)
        parts = [hi, lo, hi] if role_b else [hi, hi, lo]
        assert same_bits(sp, torch.cat(parts, 0 if stack else 1)), (role_b, stack)  # [M,3K] side by side, or stacked [3M,K], in this order


@poison
@fmt
def test_transpose_batched(K, arena, fmt, poison):
    """two matrices in one flat buffer, ragged 64 x 64 tiles; the table holds element offsets, so its guards repeat a valid row that reads
    ANOTHER tile's source (a stray table row shows as wrong values, never as a wild address)"""
    op = FMTS[fmt]
    g = torch.Generator().manual_seed(3)
    mats = [(0, 72, 136), (72 * 136, 8, 8)]
    n = 72 * 136 + 64
    src = rnd(g, (n,), dtype=op).to(op)
    table = K.transpose_table(mats)
    decoy = table[0].clone()
    decoy[0] = table[1][0]
    arena.reset(poison)
    sa, da = arena.place(src, name="src"), arena.place((n,), op, role="output", name="dst")
    ta = arena.place(table, guard_pattern=(decoy, decoy), name="table")
    with arena.route(K):
        K.transpose_bf16_batched(sa, da, ta)
    arena.verify()
    for off, R, Cc in mats:
        assert same_bits(da[off:off + R * Cc].reshape(Cc, R), src[off:off + R * Cc].reshape(R, Cc).t().contiguous().cuda()), (off, R, Cc)


@poison
@pytest.mark.parametrize("n", [1, 3, 8191, 8193])
def test_gelu_f32(K, arena, n, poison):
    g = torch.Generator().manual_seed(n)
    h, dy = torch.randn(n, generator=g) * 1.5, torch.randn(n, generator=g)
    hd = h.double().requires_grad_()
    a = O.gelu_erf(hd)
    a.backward(dy.double())
    check(guarded(K, arena, poison, lambda h: (K.gelu_f32(h),), h=h)[0], a.detach(), tol=1e-6, what="gelu f32")  # (bounds: test_split_bf16x3_linear_matches_f32_product's file, :547)
    check(guarded(K, arena, poison, lambda dy, h: (K.gelu_bwd_f32(dy, h),), dy=dy, h=h)[0], hd.grad, tol=1e-6, what="gelu bwd f32")


# =============================================================================================== optimizer side
SIZES = [1, 3, 8191, 8193]


@poison
def test_sumsq_and_grad_norm_coef_next_to_each_other(K, arena, poison):
    g = torch.Generator().manual_seed(5)
    for n in SIZES:
        v = torch.randn(n, generator=g)
        ref = (v.double() ** 2).sum().item()

        def run(v, out):
            K.sumsq(v, out)
            return (out,)
        out = guarded(K, arena, poison, run, v=v, out=InOut(torch.zeros(1)))[0]
        assert abs(out.item() - ref) <= 2e-6 * ref, (n, out.item(), ref)  # (bound: test_sumsq_alignment_tails_and_grad_norm_coef)
        inv, mx = 1.0 / 1024.0, 5.0
        o = guarded(K, arena, poison, lambda v: (K.grad_norm_coef(v, inv, mx),), v=v)[0].cpu()
        n_ref = math.sqrt(ref) * inv
        c_ref = inv * min(mx / (n_ref + 1e-6), 1.0)
        assert abs(o[0].item() - n_ref) <= 2e-6 * n_ref and abs(o[1].item() - c_ref) <= 4e-6 * c_ref and o[2].item() == 0.0, (n, o)


@poison
def test_ema_update_tensors_with_guards_between_them(K, arena, poison):
    """four parameters of 1, 3, 8191, 8193 elements, each pair its own placement: the guards BETWEEN the tensors are the point.  The table
    holds addresses, so its guards repeat a valid row / a valid chunk entry.  Bit-exact against torch (tests/test_ema_gpu.py)."""
    g = torch.Generator().manual_seed(6)
    ema0 = [torch.randn(n, generator=g) for n in SIZES]
    mod0 = [torch.randn(n, generator=g) for n in SIZES]
    decay = 0.999
    arena.reset(poison)
    ema = [arena.place(t, role="inout", name=f"ema{i}") for i, t in enumerate(ema0)]
    mod = [arena.place(t, name=f"model{i}") for i, t in enumerate(mod0)]
    tab, nt, nc = K.ema_table([(e.data_ptr(), m.data_ptr(), e.numel()) for e, m in zip(ema, mod)])
    table = arena.place(tab, guard_pattern=(tab[:4], tab[4 * nt:4 * nt + 1]), name="table")  # (a valid tensor row in front, a valid chunk pair behind)
    with arena.route(K):
        K.ema_update(table, nt, nc, decay, sum(SIZES))
    arena.verify()
    for e, e0, m0 in zip(ema, ema0, mod0):
        assert torch.equal(e.cpu(), e0 * decay + m0 * (1.0 - decay))


@poison
@fmt
@pytest.mark.parametrize("skip", [False, True], ids=["step", "skipped_step"])
def test_adamw_step_flat_buffer(K, arena, skip, fmt, poison):
    """tensors of 1, 3, 8191, 8193 elements in one flat buffer (each on a chunk boundary), the 16-bit mirror, a skipped step"""
    from simple_tad_amd import _lib
    op = FMTS[fmt]
    CH = _lib.ADAMW_CHUNK
    g = torch.Generator().manual_seed(7)
    offs, n = [], 0
    for s in SIZES:
        offs.append(n)
        n += -(-s // CH) * CH
    n = offs[-1] + -(-SIZES[-1] // 4) * 4  # the buffer ends right behind the last tensor (n % 4 == 0 is the ABI's rule): the last chunk is ragged
    chunks = -(-n // CH)
    group_of = torch.zeros(chunks, dtype=torch.uint8)
    for i, (o, s) in enumerate(zip(offs, SIZES)):
        group_of[o // CH:o // CH + -(-s // CH)] = i % 2
    p0, g0, m0, v0 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1, torch.randn(n, generator=g) * 0.01, torch.rand(n, generator=g) * 1e-3
    lr, wd, step = [1e-3, 5e-4], [0.05, 0.0], [3, 3]
    coef = 0.0 if skip else 0.5

    def run(p, gr, m, v, mirror, cg, gs, part):
        K.adamw_step(p, gr, m, v, cg, lr, wd, step, 0.9, 0.999, 1e-8, param_bf16=mirror, grad_scale=gs, sumsq_partials=part)
        return p, m, v, mirror
    mir0 = p0.to(op)
    p, m, v, mirror = guarded(K, arena, poison, run, p=InOut(p0), gr=g0, m=InOut(m0), v=InOut(v0), mirror=InOut(mir0), cg=Idx(group_of, 2),
                              gs=torch.tensor([coef]), part=InOut(torch.zeros(chunks)))
    if skip:
        assert torch.equal(p.cpu(), p0) and torch.equal(m.cpu(), m0) and torch.equal(v.cpu(), v0) and same_bits(mirror.cpu(), mir0)
        return
    grp = group_of.long().repeat_interleave(CH)[:n]
    for gi in range(2):
        sel = grp == gi
        rp, rm, rv = O.adamw_step(p0[sel].double(), g0[sel].double() * coef, m0[sel].double(), v0[sel].double(), step[gi], lr[gi], wd[gi])
        for a, b, nm in ((p, rp, "param"), (m, rm, "exp_avg"), (v, rv, "exp_avg_sq")):
            e = ((a.cpu()[sel].double() - b).norm() / b.norm()).item()
            assert e < 2e-6, (nm, gi, e)  # (bound: tests/test_optim_gpu.py)
    assert same_bits(mirror.cpu(), p.cpu().to(op)), "the 16-bit mirror is the rounded new parameter"


# =============================================================================================== MAE, metrics
# (R, D, n, mse sizes): the first case is the original one; D = 260 / 384 reach the second 64-lane pass of the row movers (D4 = 65: one
# lane of it; 96: the real decoder width); 4 * (262144 + 1) is the first size at which mse_kernel's grid-stride loop makes a second trip
GATHER_MSE = [(37, 52, 13, (4, 1004, 70012)), (37, 260, 13, ()), (37, 384, 13, (4 * (262144 + 1),))]


@poison
@pytest.mark.parametrize("R,D,n,mse_sizes", GATHER_MSE, ids=["D52", "D260", "D384-stride2"])
def test_gather_scatter_mse(K, arena, R, D, n, mse_sizes, poison):
    g = torch.Generator().manual_seed(8)
    src = torch.randn(R, D, generator=g)
    idx = torch.randperm(R, generator=g)[:n].to(torch.int32)
    got = guarded(K, arena, poison, lambda src, idx: (K.gather_rows(src, idx),), src=src, idx=Idx(idx, R))[0]
    assert torch.equal(got.cpu(), src[idx.long()])  # bit-exact row moves (tests/test_pretrain.py)
    rows = torch.randn(n, D, generator=g)
    back = guarded(K, arena, poison, lambda rows, idx: (K.scatter_rows(rows, idx, R),), rows=rows, idx=Idx(idx, R))[0].cpu()
    want = torch.zeros(R, D)
    want[idx.long()] = rows
    assert torch.equal(back, want)
    for cnt in mse_sizes:  # (n % 4 == 0 is the ABI's rule)
        pred, tgt = torch.randn(cnt, generator=g), torch.randn(cnt, generator=g)
        # (partials.sum() / n runs in torch on the kernel's partials: compared through the loss)
        loss, grad = guarded(K, arena, poison, lambda pred, tgt: K.mse_loss(pred, tgt), pred=pred, tgt=tgt)
        # tad_mse_loss_blocks: the wrapper's partials are a placement of exactly the declared number of f32 (nothing rounds it up)
        assert (arena.placements[2].name.startswith("wrapper") and arena.placements[2].end - arena.placements[2].start == 4 * _lib().tad_mse_loss_blocks(cnt))
        pr = pred.double().requires_grad_()
        lr = torch.nn.functional.mse_loss(pr, tgt.double())
        lr.backward()
        assert abs(loss.item() - lr.item()) < 1e-6 * lr.item() and ((grad.cpu().double() - pr.grad).norm() / pr.grad.norm()).item() < 1e-6  # (test_mae_kernels_vs_oracle)


# (D, tubelet, patch): the first case is the original one; D = 260 / 384: second lane pass of mae_assemble; (1, 8): 64 pixels, the NPIX = 4
# instance of mae_target; (3, 16): 768 pixels, the NPIX = 16 instance, its last slots partly filled
ASSEMBLE_TARGET = [(52, 2, 16), (260, 1, 8), (384, 3, 16)]


@poison
@pytest.mark.parametrize("D,tub,p", ASSEMBLE_TARGET, ids=["D52-2x16", "D260-1x8", "D384-3x16"])
def test_mae_assemble_and_target(K, arena, D, tub, p, poison):
    """expressions and bounds of tests/test_pretrain.py::test_mae_kernels_vs_oracle; odd counts; the index tensors sit between in-range indices"""
    g = torch.Generator().manual_seed(12)
    B, N, Nm = 3, 39, 27
    mask = torch.zeros(B, N, dtype=torch.bool)
    for b in range(B):
        mask[b, torch.randperm(N, generator=g)[:Nm]] = True
    vis = torch.stack([(~mask[b]).nonzero().flatten() for b in range(B)]).to(torch.int32)
    msk = torch.stack([mask[b].nonzero().flatten() for b in range(B)]).to(torch.int32)
    tok, pos, xv = torch.randn(D, generator=g), torch.randn(N, D, generator=g), torch.randn(B, N - Nm, D, generator=g)
    full = guarded(K, arena, poison, lambda xv, tok, pos, vis, msk: (K.mae_assemble(xv, tok, pos, vis, msk, B),),
                   xv=xv.reshape(-1, D), tok=tok, pos=pos, vis=Idx(vis.reshape(-1), N), msk=Idx(msk.reshape(-1), N))[0].cpu()
    pe = pos.expand(B, -1, -1)
    assert torch.equal(full, torch.cat([xv + pe[~mask].reshape(B, -1, D), tok + pe[mask].reshape(B, -1, D)], dim=1))
    vids = torch.randn(3, 3, 2 * tub, 2 * p, 3 * p, generator=g)
    m2 = torch.zeros(3, 2 * 2 * 3, dtype=torch.bool)
    m2[:, [1, 2, 5, 7, 8, 10, 11]] = True
    mt = torch.stack([m2[b].nonzero().flatten() for b in range(3)]).to(torch.int32)
    for norm in (True, False):
        lab = guarded(K, arena, poison, lambda v, mt: (K.mae_target(v, mt, tub, p, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), norm),),
                      v=vids, mt=Idx(mt.reshape(-1), 12))[0].cpu()
        ref = O.mae_target(vids.double(), m2, tubelet=tub, patch=p, normalize_target=norm)
        assert lab.shape == ref.shape and ((lab.double() - ref).norm() / ref.norm()).item() < 2e-6, norm


@poison
@pytest.mark.parametrize("n,T", [(1, 101), (1001, 101), (70003, 37)])
def test_threshold_histogram(K, arena, n, T, poison):
    """exact integer counts (simple_tad_amd/metrics.py allocates through its own module: the C ABI is called on placements here)"""
    from simple_tad_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(n)
    p, y = torch.rand(n, generator=g), (torch.rand(n, generator=g) > 0.7).to(torch.int32)
    thr = torch.linspace(0, 1, T)
    arena.reset(poison)
    pa, ya, ta = arena.place(p, name="p"), arena.place(y, index_range=2, name="labels"), arena.place(thr, name="thresholds")
    hist = arena.place((2, T + 1), torch.int64, role="output", index_range=1 << 31, name="hist")  # (counts, never read as indices)
    assert lib.tad_threshold_histogram(pa.data_ptr(), ya.data_ptr(), ta.data_ptr(), T, n, hist.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    arena.verify()
    k = (p[:, None] >= thr[None, :]).sum(1)  # thresholds at or below p
    want = torch.zeros(2, T + 1, dtype=torch.int64)
    for lab in (0, 1):
        want[lab] = torch.bincount(k[y == lab], minlength=T + 1)
    assert torch.equal(hist.cpu(), want)


# =============================================================================================== workspace contracts (C ABI, exact sizes)
@poison
@pytest.mark.parametrize("query", ['linear_bwd_weight', 'linear_splitk', 'layernorm_bwd', 'colsum', 'colsum_window', 'sumsq'])
def test_workspace_contract_holds_at_exactly_the_declared_size(K, arena, query, poison):
    """a C host allocates exactly what the *_bytes query returns; the Python wrapper never allocates less than 1 MiB, so the entry points are
    called directly here with a workspace placement of exactly the declared size: result right, nothing behind it written.
    tad_attn_bwd_scratch_bytes and tad_mse_loss_blocks: kernels.attn_bwd / kernels.mse_loss allocate exactly the declared size themselves, and
    test_attention_16bit / test_gather_scatter_mse assert that their routed placement has exactly that size"""
    from simple_tad_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(9)
    bfl = torch.bfloat16

    def ws_of(nbytes, name):
        assert nbytes > 0, name
        return arena.place((nbytes,), torch.uint8, role="workspace", name=f"{name} workspace of {nbytes} bytes")

    def ok(rc):
        assert rc == 0, lib.tad_last_error_string()

    if query == "linear_bwd_weight":
        # tad_linear_bwd_weight_workspace_bytes / tad_patch_embed_bwd_workspace_bytes (split reduction: slabs in the workspace)
        M, N, Kd = 5003, 264, 392
        dy, x = rnd(g, (M, N), dtype=bfl), rnd(g, (M, Kd), dtype=bfl)
        for fn, query in ((lib.tad_linear_bwd_weight, lib.tad_linear_bwd_weight_workspace_bytes), (None, lib.tad_patch_embed_bwd_workspace_bytes)):
            arena.reset(poison)
            dya, xa = arena.place(dy.to(bfl), name="dy"), arena.place(x.to(bfl), name="x")
            dW, db = arena.place((N, Kd), torch.float32, role="output", name="dW"), arena.place((N,), torch.float32, role="output", name="db")
            nb = query(M, N, Kd)
            ws = ws_of(nb, "gemm_tn")
            if fn is None:
                ok(lib.tad_patch_embed_bwd(dya.data_ptr(), xa.data_ptr(), dW.data_ptr(), db.data_ptr(), ws.data_ptr(), nb, M, N, Kd, st))
            else:
                ok(fn(dya.data_ptr(), xa.data_ptr(), dW.data_ptr(), db.data_ptr(), 0, ws.data_ptr(), nb, M, N, Kd, st))
            arena.verify()
            check(dW, dy.double().t() @ x.double(), what="dW (exact workspace)")
            check(db, dy.double().sum(0), what="db (exact workspace)")

    if query == "linear_splitk":
        # tad_linear_workspace_bytes: the split-K tail's partial tiles
        M, N, Kd = 33 * 256 + 37, 2048, 512
        xl, wl, bl = rnd(g, (M, Kd), dtype=bfl), rnd(g, (N, Kd), 0.05, bfl), torch.randn(N, generator=g) * 0.1
        try:
            K.linear_tuning(**{**K.LINEAR_TUNING_DEFAULTS, "splitk_tail": 2, "split_tail": 2})
            arena.reset(poison)
            xa, wa, ba = arena.place(xl.to(bfl), name="x"), arena.place(wl.to(bfl), name="w"), arena.place(bl, name="bias")
            y = arena.place((M, N), bfl, role="output", name="y")
            nb = lib.tad_linear_workspace_bytes(M, N, Kd)
            ws = ws_of(nb, "split-K")
            n0 = lib.tad_linear_kernel_launches()
            ok(lib.tad_linear_fwd(xa.data_ptr(), wa.data_ptr(), ba.data_ptr(), y.data_ptr(), _lib.TAD_BF16, _lib.EPI_BIAS, None, None, None, None, 1, ws.data_ptr(), nb, M, N, Kd, st))
            assert lib.tad_linear_kernel_launches() - n0 == 3, "the split-K plan was not taken with the declared workspace"
            arena.verify()
        finally:
            K.linear_tuning(**K.LINEAR_TUNING_DEFAULTS)
        check(y.float(), xl.double() @ wl.double().t() + bl.double(), tol=ULP16, what="linear split-K (exact workspace)")

    if query == "layernorm_bwd":
        # tad_layernorm_bwd_workspace_bytes
        rows, D = 1569, 1000
        xn, wn, dyn = torch.randn(rows, D, generator=g), torch.randn(D, generator=g) * 0.2 + 1, torch.randn(rows, D, generator=g)
        xd, wd, bd = xn.double().requires_grad_(), wn.double().requires_grad_(), torch.zeros(D).double().requires_grad_()
        O.layer_norm(xd, wd, bd, 1e-6).backward(dyn.double())
        arena.reset(poison)
        mean, var = xn.double().mean(-1), xn.double().var(-1, unbiased=False)
        a = {k: arena.place(v, name=k) for k, v in dict(dy=dyn, x=xn, gamma=wn, mean=mean.float(), rstd=(var + 1e-6).rsqrt().float()).items()}
        o = {k: arena.place(s, torch.float32, role="output", name=k) for k, s in dict(dx=(rows, D), dgamma=(D,), dbeta=(D,), colsum=(D,)).items()}  # (colsum_dx too: its partials are the last third of the workspace)
        nb = lib.tad_layernorm_bwd_workspace_bytes(rows, D)
        ws = ws_of(nb, "layernorm_bwd")
        ok(lib.tad_layernorm_bwd(a["dy"].data_ptr(), _lib.TAD_F32, a["x"].data_ptr(), a["gamma"].data_ptr(), a["mean"].data_ptr(), a["rstd"].data_ptr(), None,
                                 o["dx"].data_ptr(), None, o["dgamma"].data_ptr(), o["dbeta"].data_ptr(), o["colsum"].data_ptr(), None, 1, 0, ws.data_ptr(), nb, rows, D, st))
        arena.verify()
        check(o["dx"], xd.grad, what="ln dx (exact workspace)")
        check(o["dgamma"], wd.grad, what="ln dgamma (exact workspace)")
        check(o["dbeta"], bd.grad, what="ln dbeta (exact workspace)")
        check(o["colsum"], xd.grad.sum(0), what="ln colsum (exact workspace)")

    if query == "colsum":
        # tad_colsum_workspace_bytes (bf16 rows and the f32 window) / tad_sumsq_workspace_bytes
        M, N = 5003, 776
        a16 = rnd(g, (M, N), dtype=bfl)
        arena.reset(poison)
        aa, out = arena.place(a16.to(bfl), name="a"), arena.place((N,), torch.float32, role="output", name="colsum")
        nb = lib.tad_colsum_workspace_bytes(M, N)
        ws = ws_of(nb, "colsum")
        ok(lib.tad_colsum_bf16(aa.data_ptr(), out.data_ptr(), 0, ws.data_ptr(), nb, M, N, st))
        arena.verify()
        check(out, a16.double().sum(0), tol=1e-5, what="colsum (exact workspace)")
    if query == "colsum_window":
        N = 776
        B, R, r0, rc = 3, 1667, 555, 1112
        a3 = torch.randn(B, R, N, generator=g)
        arena.reset(poison)
        aa, out = arena.place(a3, name="a"), arena.place((N,), torch.float32, role="output", name="colsum_window")
        nb = lib.tad_colsum_workspace_bytes(B * rc, N)
        ws = ws_of(nb, "colsum_window")
        ok(lib.tad_colsum_window_f32(aa.data_ptr(), out.data_ptr(), 0, ws.data_ptr(), nb, B, R, N, r0, rc, st))
        arena.verify()
        check(out, a3[:, r0:r0 + rc].double().sum((0, 1)), tol=1e-5, what="colsum_window (exact workspace)")
    if query == "sumsq":
        v = torch.randn(3_000_017, generator=g)
        arena.reset(poison)
        va, out = arena.place(v, name="v"), arena.place(torch.zeros(1), role="inout", name="sumsq")
        nb = lib.tad_sumsq_workspace_bytes()
        ws = ws_of(nb, "sumsq")
        ok(lib.tad_sumsq_f32(va.data_ptr(), v.numel(), out.data_ptr(), ws.data_ptr(), nb, st))
        arena.verify()
        ref = (v.double() ** 2).sum().item()
        assert abs(out.item() - ref) <= 2e-6 * ref
