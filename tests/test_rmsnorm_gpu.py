"""The RMSNorm and q / k normalisation kernels (csrc/rmsnorm.hip, include/tad_mi355x_ext.h) against fp64, row by row.

Yardstick (the one tests/test_numeric_edges_gpu.py holds LayerNorm to): an f32 result may err, per row and relative to the row's largest
reference magnitude, by 4x what torch's own f32 expression (forward) or its autograd (backward) errs by on the same row on the same
device -- a wave's summation order differs from torch's, a small constant -- floored at 8 f32 ulps of that magnitude (edge_cases.LN_FLOOR:
on a row where torch happens to be exact, one rounding of ours must not fail).  A 16-bit result may err per element by
1.0625 x (u |ref| + that f32 bound + eta), u = 2^-8 (bf16) / 2^-11 (half), eta = half the smallest subnormal of half (2^-25; 0 for bf16)
and 1/16 standing for the second-order terms (tests/attn_bounds.py: SLACK).

Row classes, interleaved (row r is class r % 4): Gaussian; Gaussian with an offset of 10 .. 1e4; Gaussian with one massive channel; all zero.
"""
import math

import pytest
import torch

import edge_cases as E
import guarded
from attn_bounds import SLACK

pytestmark = pytest.mark.gpu

EPS = 1e-6
DIMS = [4, 128, 384, 768, 1024, 1408, 1792, 2048]  # one lane; a half-idle wave; guarded and exact multiples of 256 (1792 = 7 x 256: the
# one exact multiple whose float4 count per lane, 7, is not also a LayerNorm instance); the register maximum
ROWS = [1, 3, 5, 33, 70]                     # tails of the 4-rows-per-block forward; a backward over 1, 2 and 3 block chunks
QK_SHAPES = [(1, 64), (9, 128), (18, 128), (70, 384), (9, 1408), (5, 1792), (5, 2048)]  # ... the 1B width (guarded, 6 chunks), 7 chunks, and the
# maximum, where the backward asks for exactly 64 KB of LDS
FMT = {"bf16": (torch.bfloat16, 2.0 ** -8, 0.0), "f16": (torch.float16, 2.0 ** -11, 2.0 ** -25)}
FLOOR = E.LN_FLOOR


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import _lib, kernels
    _lib.load()
    return kernels


def dev(t):
    return t.cuda().contiguous()


def hostile_rows(rows, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=g)
    for r in range(rows):
        c = r % 4
        if c == 1:
            x[r] += 10.0 ** (1 + (r // 4) % 4)
        elif c == 2:
            x[r, (7 * r) % D] = 3.0e3
        elif c == 3:
            x[r] = 0.0
    return x


def rms64(x, g, scale=1.0):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * g * scale


def fwd_bwd(x, g, dy, dtype):
    """(y, rrms, dx, dgamma) of the reference expression in ``dtype`` on x's device, backward by autograd"""
    x, g = x.detach().to(dtype).clone().requires_grad_(), g.detach().to(dtype).clone().requires_grad_()
    y = rms64(x, g)
    y.backward(dy.to(dtype))
    return y.detach(), torch.rsqrt(x.detach().pow(2).mean(-1) + EPS), x.grad, g.grad


def row_err(got, ref):
    """max |got - ref| per row relative to the row's largest |ref| (an all-zero reference row: absolute)"""
    ref = ref.double()
    return (got.double() - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-300)


def row_bound(torch32, ref):
    return (4 * row_err(torch32, ref)).clamp_min(FLOOR)


def check16(got16, ref, f32_bound, fmt, what):
    """per element: |got - ref| <= SLACK (u |ref| + f32_bound[row] max|ref row| + eta)"""
    _, u, eta = FMT[fmt]
    ref = ref.double()
    lim = SLACK * (u * ref.abs() + (f32_bound * ref.abs().amax(-1)).unsqueeze(-1) + eta)
    err = (got16.double() - ref).abs()
    worst = (err / lim.clamp_min(1e-300)).max().item()
    print(f"{what} [{fmt}]: worst error / bound {worst:.3f}")
    assert (err <= lim).all(), f"{what} [{fmt}]: {int((err > lim).sum())} elements over the bound, worst ratio {worst:.3f}"


def rel_l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


# ================================================================== RMSNorm
@pytest.mark.parametrize("D", DIMS)
def test_rmsnorm_every_row_count_against_fp64(K, D):
    for rows in ROWS:
        x, gamma = hostile_rows(rows, D, 100 + D + rows), 1.0 + 0.3 * torch.randn(D, generator=torch.Generator().manual_seed(D))
        gd = torch.Generator().manual_seed(7 * D + rows)
        dy, dres = torch.randn(rows, D, generator=gd), torch.randn(rows, D, generator=gd)
        xd, gmd, dyd = dev(x), dev(gamma), dev(dy)
        y64, rr64, dx64, dg64 = fwd_bwd(xd, gmd, dyd, torch.float64)
        y_t, _, dx_t, dg_t = fwd_bwd(xd, gmd, dyd, torch.float32)
        what = f"D {D} rows {rows}"
        # ---- forward, f32
        y, rr = K.rmsnorm_fwd(xd, gmd, EPS, out_dtype=torch.float32)
        b_y = row_bound(y_t, y64)
        e_y = row_err(y, y64)
        print(f"{what}: y worst error / bound {(e_y / b_y).max():.3f}; torch's own worst row error {row_err(y_t, y64).max():.2e}")
        assert (e_y <= b_y).all(), f"{what}: y rows {torch.nonzero(e_y > b_y).flatten().tolist()} over their bound (class = row % 4)"
        assert ((rr.double() - rr64).abs() <= 4 * E.F32_EPS * rr64).all(), f"{what}: rrms"
        zero = torch.arange(rows) % 4 == 3
        if zero.any():
            assert not y[zero.cuda()].any(), "an all-zero row gives y = 0"
            r0 = 1.0 / math.sqrt(float(torch.tensor(EPS, dtype=torch.float32)))
            assert ((rr[zero.cuda()].double() - r0).abs() <= 2 * E.F32_EPS * r0).all(), "rrms of an all-zero row: eps^-1/2"
        y_nostat, none = K.rmsnorm_fwd(xd, gmd, EPS, out_dtype=torch.float32, save_stats=False)
        assert none is None and guarded.same_bits(y_nostat, y)
        # ---- forward, 16-bit: bounded per element, and RNE of the f32 output
        for fmt, (dt, _, _) in FMT.items():
            y16, rr16 = K.rmsnorm_fwd(xd, gmd, EPS, out_dtype=dt)
            check16(y16, y64, b_y, fmt, f"{what}: y16")
            assert guarded.same_bits(y16, y.to(dt)) and torch.equal(rr16, rr), f"{what}: the {fmt} output is not RNE of the f32 output"
        # ---- backward with the forward's own statistics
        dx, none, dg = K.rmsnorm_bwd(dyd, xd, gmd, rr)
        assert none is None
        b_dx = row_bound(dx_t, dx64)
        e_dx = row_err(dx, dx64)
        print(f"{what}: dx worst error / bound {(e_dx / b_dx).max():.3f}")
        assert (e_dx <= b_dx).all(), f"{what}: dx rows {torch.nonzero(e_dx > b_dx).flatten().tolist()} over their bound"
        assert torch.isfinite(dx).all()
        if zero.any():
            zc = zero.cuda()
            want = (rr64[zc].unsqueeze(-1) * dyd[zc].double() * gmd.double())
            assert ((dx[zc].double() - want).abs() <= 4 * E.F32_EPS * want.abs()).all(), "dx of an all-zero row: rrms dy gamma"
        e_dg, t_dg = rel_l2(dg, dg64), rel_l2(dg_t, dg64)
        print(f"{what}: dgamma rel-L2 {e_dg:.2e}, torch's {t_dg:.2e}")
        assert e_dg <= max(4 * t_dg, FLOOR), f"{what}: dgamma rel-L2 {e_dg:.2e} against torch's {t_dg:.2e}"
        # ---- + residual gradient, 16-bit copy of dx, accumulation onto existing content, 16-bit dy
        dresd = dev(dres)
        seed_dg = torch.linspace(-1, 1, D).cuda()
        acc = seed_dg.clone()
        dx2, dx16, dg2 = K.rmsnorm_bwd(dyd, xd, gmd, rr, dres=dresd, want_op16=True, into=acc)
        ref2 = dx64 + dresd.double()
        lim = b_dx * dx64.abs().amax(-1) + E.F32_EPS * ref2.abs().amax(-1)  # dx's own bound + one rounding of the sum
        assert ((dx2.double() - ref2).abs().amax(-1) <= lim).all(), f"{what}: dx + dres"
        assert guarded.same_bits(dx16, dx2.to(dx16.dtype)), "the 16-bit copy of dx is not RNE of the f32 dx"
        assert dg2 is acc and guarded.same_bits(acc, seed_dg + dg), "accumulate = 1 adds the same sum onto the existing content"
        for fmt, (dt, u, eta) in FMT.items():
            dy16 = dyd.to(dt)
            _, _, dx64h, dg64h = fwd_bwd(xd, gmd, dy16.double(), torch.float64)
            _, _, dx_th, dg_th = fwd_bwd(xd, gmd, dy16.float(), torch.float32)
            dxh, dxh16, dgh = K.rmsnorm_bwd(dy16, xd, gmd, rr, want_op16=True)
            bh = row_bound(dx_th, dx64h)
            assert (row_err(dxh, dx64h) <= bh).all(), f"{what}: dx from a {fmt} dy"
            assert dxh16.dtype == dt
            check16(dxh16, dx64h, bh, fmt, f"{what}: dx16")
            assert rel_l2(dgh, dg64h) <= max(4 * rel_l2(dg_th, dg64h), FLOOR)
        # ---- the same bits twice
        again = K.rmsnorm_bwd(dyd, xd, gmd, rr)
        assert guarded.same_bits(again[0], dx) and guarded.same_bits(again[2], dg)
        assert guarded.same_bits(K.rmsnorm_fwd(xd, gmd, EPS, out_dtype=torch.float32)[0], y)


def test_rmsnorm_planted_nan_stays_in_its_row(K):
    rows, D, r = 33, 384, 18
    x, gamma, dy = hostile_rows(rows, D, 5), torch.ones(D) * 0.7, torch.randn(rows, D, generator=torch.Generator().manual_seed(6))
    xd, gd, dyd = dev(x), dev(gamma), dev(dy)
    y, rr = K.rmsnorm_fwd(xd, gd, EPS, out_dtype=torch.float32)
    dx, _, dg = K.rmsnorm_bwd(dyd, xd, gd, rr)
    xp = xd.clone()
    xp[r, 100] = float("nan")
    yp, rrp = K.rmsnorm_fwd(xp, gd, EPS, out_dtype=torch.float32)
    dxp, _, dgp = K.rmsnorm_bwd(dyd, xp, gd, rrp)
    keep = torch.arange(rows).cuda() != r
    assert guarded.same_bits(yp[keep], y[keep]) and guarded.same_bits(dxp[keep], dx[keep]) and guarded.same_bits(rrp[keep], rr[keep])
    assert torch.isnan(yp[r]).all() and torch.isnan(dxp[r]).all() and torch.isnan(dgp).all()
    # a NaN in dy alone: its whole row of dx (the row's mean(t xh) is NaN) and its own column of the gamma gradient, nothing else
    dyp = dyd.clone()
    dyp[r, 3] = float("nan")
    dxq, _, dgq = K.rmsnorm_bwd(dyp, xd, gd, rr)
    assert guarded.same_bits(dxq[keep], dx[keep]) and torch.isnan(dxq[r]).all()
    assert torch.isnan(dgq[3]) and guarded.same_bits(torch.cat((dgq[:3], dgq[4:])), torch.cat((dg[:3], dg[4:])))


# ================================================================== q / k normalisation
def qk_inputs(M, A, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.cat([hostile_rows(M, A, seed + i) for i in range(3)], dim=1) if M >= 4 else torch.randn(M, 3 * A, generator=g)
    gq, gk = 1.0 + 0.3 * torch.randn(A, generator=g), 1.0 + 0.3 * torch.randn(A, generator=g)
    dqkv = torch.randn(M, 3 * A, generator=g)
    return qkv, gq, gk, dqkv


def qk_ref(qkv, gq, gk, d, dtype, A):
    """(q normalised, k normalised, d q_pre, d k_pre, dgq, dgk) of the reference expression in ``dtype``: d is the gradient of the PLAIN
    normalised q and k (what tad_attn_bwd produces under either q contract)"""
    q, k, _ = (t.detach().to(dtype).clone().requires_grad_() for t in qkv.split(A, dim=1))
    gq, gk = gq.detach().to(dtype).clone().requires_grad_(), gk.detach().to(dtype).clone().requires_grad_()
    qn, kn = rms64(q, gq), rms64(k, gk)
    dq, dk, _ = d.to(dtype).split(A, dim=1)
    ((qn * dq).sum() + (kn * dk).sum()).backward()
    return qn.detach(), kn.detach(), q.grad, k.grad, gq.grad, gk.grad


@pytest.mark.parametrize("M,A", QK_SHAPES)
@pytest.mark.parametrize("fmt", list(FMT))
def test_qk_rmsnorm_against_fp64(K, M, A, fmt):
    dt, u, eta = FMT[fmt]
    qkv, gq, gk, dqkv = qk_inputs(M, A, 11 * M + A)
    qkvd, gqd, gkd = dev(qkv), dev(gq), dev(gk)
    d16 = dev(dqkv).to(dt)
    q64, k64, dq64, dk64, dgq64, dgk64 = qk_ref(qkvd, gqd, gkd, d16.double(), torch.float64, A)
    q_t, k_t, dq_t, dk_t, dgq_t, dgk_t = qk_ref(qkvd, gqd, gkd, d16.float(), torch.float32, A)
    what = f"M {M} A {A}"
    for s in (1.0, K.q_prescale_of(64 ** -0.5)):
        out, rr = K.qk_rmsnorm_fwd(qkvd, gqd, gkd, EPS, q_out_scale=s, dtype=dt)
        assert out.dtype == dt and out.shape == (M, 3 * A) and rr.shape == (M, 2)
        # (the f32 bound of q * s: torch's expression with the factor, the error scales with it)
        check16(out[:, :A], q64 * s, row_bound(q_t * s, q64 * s), fmt, f"{what} s {s:.3f}: q third")
        check16(out[:, A:2 * A], k64, row_bound(k_t, k64), fmt, f"{what}: k third")
        assert guarded.same_bits(out[:, 2 * A:], K.cast_op16(qkvd[:, 2 * A:].contiguous(), dtype=dt)), "the v third is the plain cast"
        rr64 = torch.stack([torch.rsqrt(t.double().pow(2).mean(-1) + EPS) for t in qkvd.split(A, dim=1)[:2]], dim=1)
        assert ((rr.double() - rr64).abs() <= 4 * E.F32_EPS * rr64).all()
        assert guarded.same_bits(K.qk_rmsnorm_fwd(qkvd, gqd, gkd, EPS, q_out_scale=s, dtype=dt, save_stats=False)[0], out)
        # ---- backward: the factor does not enter (the incoming dq is the gradient of the plain normalised q)
        pre, dgq, dgk = K.qk_rmsnorm_bwd(d16, qkvd, gqd, gkd, rr, q_out_scale=s)
        check16(pre[:, :A], dq64, row_bound(dq_t, dq64), fmt, f"{what} s {s:.3f}: dq_pre")
        check16(pre[:, A:2 * A], dk64, row_bound(dk_t, dk64), fmt, f"{what}: dk_pre")
        assert guarded.same_bits(pre[:, 2 * A:], d16[:, 2 * A:]), "the v third of the gradient is a copy"
        for got, ref, t32, name in ((dgq, dgq64, dgq_t, "dgq"), (dgk, dgk64, dgk_t, "dgk")):
            e, t = rel_l2(got, ref), rel_l2(t32, ref)
            print(f"{what}: {name} rel-L2 {e:.2e}, torch's {t:.2e}")
            assert e <= max(4 * t, FLOOR), f"{what}: {name} rel-L2 {e:.2e} against torch's {t:.2e}"
        # ---- accumulate, and the same bits twice
        a0, a1 = torch.full((A,), 0.25).cuda(), torch.linspace(0, 1, A).cuda()
        b0, b1 = a0.clone(), a1.clone()
        pre2, r0, r1 = K.qk_rmsnorm_bwd(d16, qkvd, gqd, gkd, rr, q_out_scale=s, into=(b0, b1))
        assert r0 is b0 and guarded.same_bits(b0, a0 + dgq) and guarded.same_bits(b1, a1 + dgk) and guarded.same_bits(pre2, pre)


def test_qk_rmsnorm_planted_nan_stays_in_its_row(K):
    M, A, r = 18, 128, 7
    qkv, gq, gk, dqkv = qk_inputs(M, A, 3)
    qkvd, gqd, gkd, d16 = dev(qkv), dev(gq), dev(gk), dev(dqkv).bfloat16()
    out, rr = K.qk_rmsnorm_fwd(qkvd, gqd, gkd, EPS)
    pre, dgq, dgk = K.qk_rmsnorm_bwd(d16, qkvd, gqd, gkd, rr)
    bad = qkvd.clone()
    bad[r, 5] = float("nan")  # in the q third
    outp, rrp = K.qk_rmsnorm_fwd(bad, gqd, gkd, EPS)
    prep, dgqp, dgkp = K.qk_rmsnorm_bwd(d16, bad, gqd, gkd, rrp)
    keep = torch.arange(M).cuda() != r
    assert guarded.same_bits(outp[keep], out[keep]) and guarded.same_bits(prep[keep], pre[keep])
    assert torch.isnan(outp[r, :A]).all() and guarded.same_bits(outp[r, A:], out[r, A:]), "the k and v thirds of the row are untouched"
    assert torch.isnan(prep[r, :A]).all() and guarded.same_bits(prep[r, A:], pre[r, A:])
    assert torch.isnan(dgqp).all() and guarded.same_bits(dgkp, dgk)


@pytest.mark.parametrize("prescale", [True, False])
def test_q_contract_through_the_attention_kernels(K, prescale):
    """qk_rmsnorm_fwd -> attn_fwd -> attn_bwd -> qk_rmsnorm_bwd against the fp64 chain, under both q contracts.  This is where a wrong use
    of q_out_scale in the backward shows: the factor scale * log2(e) = 0.18 would scale dq_pre and dgq by 0.18 or 5.5.  The tolerance is
    for the 16-bit roundings of the chain (qkv16, P, out, dout, dqkv: a handful of 2^-8 each): 3 % of a tensor's norm."""
    B, N, H, d = 2, 9, 2, 64
    A, scale = H * d, d ** -0.5
    qkv, gq, gk, _ = qk_inputs(B * N, A, 21)
    qkvd, gqd, gkd = dev(qkv * 0.5), dev(gq), dev(gk)
    dout = dev(torch.randn(B * N, A, generator=torch.Generator().manual_seed(22)))
    s = K.q_prescale_of(scale) if prescale else 1.0
    qkv16, rr = K.qk_rmsnorm_fwd(qkvd, gqd, gkd, EPS, q_out_scale=s)
    out, lse = K.attn_fwd(qkv16, B, N, H, scale, q_prescaled=prescale)
    dqkv = K.attn_bwd(qkv16, out, dout.bfloat16(), lse, B, N, H, scale, q_prescaled=prescale)
    pre, dgq, dgk = K.qk_rmsnorm_bwd(dqkv, qkvd, gqd, gkd, rr, q_out_scale=s)
    x = qkvd.double().requires_grad_()
    g0, g1 = gqd.double().requires_grad_(), gkd.double().requires_grad_()
    q, k, v = x.split(A, dim=1)
    heads = lambda t: t.reshape(B, N, H, d).transpose(1, 2)
    att = ((heads(rms64(q, g0)) * scale) @ heads(rms64(k, g1)).transpose(-2, -1)).softmax(-1)
    ref = (att @ heads(v)).transpose(1, 2).reshape(B * N, A)
    (ref * dout.double()).sum().backward()
    assert rel_l2(out, ref) <= 0.03
    for got, want, name in ((pre, x.grad, "dqkv_pre"), (pre[:, :A], x.grad[:, :A], "dq_pre"), (dgq, g0.grad, "dgq"), (dgk, g1.grad, "dgk")):
        e = rel_l2(got, want)
        print(f"prescale {prescale}: {name} rel-L2 {e:.2e}")
        assert e <= 0.03, f"{name}: rel-L2 {e:.2e} (a wrong q factor gives >= 0.8)"


# ================================================================== guard bands
@pytest.mark.parametrize("rows,D", [(5, 132), (5, 1792)])  # (1792: the exact multiple of 256 with seven chunks per lane, unguarded in the backward)
@pytest.mark.parametrize("poison", guarded.POISON_MODES)
def test_every_wrapper_inside_poisoned_guard_bands(K, poison, rows, D):
    M, A = 9, 128
    x, gamma = hostile_rows(rows, D, 1), torch.linspace(0.5, 1.5, D)
    dy = torch.randn(rows, D, generator=torch.Generator().manual_seed(2))
    qkv, gq, gk, dqkv = qk_inputs(M, A, 4)
    # the unguarded results
    y, rr = K.rmsnorm_fwd(dev(x), dev(gamma), EPS, out_dtype=torch.float32)
    y16, _ = K.rmsnorm_fwd(dev(x), dev(gamma), EPS)
    dx, dx16, dg = K.rmsnorm_bwd(dev(dy), dev(x), dev(gamma), rr, dres=dev(dy), want_op16=True)
    out, r2 = K.qk_rmsnorm_fwd(dev(qkv), dev(gq), dev(gk), EPS, q_out_scale=0.18)
    pre, dgq, dgk = K.qk_rmsnorm_bwd(dev(dqkv).bfloat16(), dev(qkv), dev(gq), dev(gk), r2, q_out_scale=0.18)
    arena = guarded.GuardedArena(128 << 20, "cuda", poison=poison)
    place = lambda t: arena.place(dev(t), role="input")
    xa, ga, dya, rra = place(x), place(gamma), place(dy), place(rr)
    qa, gqa, gka, da, r2a = place(qkv), place(gq), place(gk), place(dev(dqkv).bfloat16()), place(r2)
    with arena.route(K):
        g_y, g_rr = K.rmsnorm_fwd(xa, ga, EPS, out_dtype=torch.float32)
        g_y16, _ = K.rmsnorm_fwd(xa, ga, EPS)
        g_dx, g_dx16, g_dg = K.rmsnorm_bwd(dya, xa, ga, rra, dres=dya, want_op16=True)
        g_out, g_r2 = K.qk_rmsnorm_fwd(qa, gqa, gka, EPS, q_out_scale=0.18)
        g_pre, g_dgq, g_dgk = K.qk_rmsnorm_bwd(da, qa, gqa, gka, r2a, q_out_scale=0.18)
    arena.verify()
    for got, want in ((g_y, y), (g_rr, rr), (g_y16, y16), (g_dx, dx), (g_dx16, dx16), (g_dg, dg), (g_out, out), (g_r2, r2), (g_pre, pre),
                      (g_dgq, dgq), (g_dgk, dgk)):
        assert arena.contains(got) and guarded.same_bits(got, want)
