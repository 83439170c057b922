"""tads_residual_rmsnorm_fwd (csrc/iv2_serve.hip): the evaluation tail of an InternVideo2 half block -- x_out = x + y * ls_gamma -- and the
RMSNorm of x_out as the next Linear's 16-bit operand, in one pass.

x_out is held to the bits of torch's ``x + y * gamma`` (the product and the sum each rounded on their own).  xn is held, per element, to
the bound tests/test_rmsnorm_gpu.py applies to rmsnorm_fwd's 16-bit output, restated here (``check16``): with the reference computed in
fp64 from the kernel's OWN x_out,
    |xn - ref| <= 1.0625 x (u |ref| + f32_bound[row] max|ref row| + eta)
u = 2^-8 (bf16) / 2^-11 (half), eta = 2^-25 for half (half the smallest subnormal) and 0 for bf16, 1/16 for the second-order terms, and
f32_bound[row] = 4 x the row error of torch's own f32 expression on the same row on the same device, floored at 8 f32 ulps.

Row classes, interleaved (row r is class r % 4): Gaussian; Gaussian with an offset of 10 .. 1e4; one massive channel; all zero.
Measured on an MI355X: worst error / bound 0.937 (bf16 at D 1792, half at D 2048), 0.897 / 0.790 at D 4.
"""
import pytest
import torch

import guarded
import iv2_serve_ref as S

pytestmark = pytest.mark.gpu

EPS = 1e-6
DIMS = [4, 128, 256, 260, 384, 1024, 1408, 1792, 2048]  # one lane; half a wave; exactly one chunk, and one float4 into the second; the small
# model; 4, 6 (guarded), 7 and 8 chunks per lane
ROWS = [1, 3, 5, 33, 70]  # the tails of four rows per block
FMT = {"bf16": (torch.bfloat16, 2.0 ** -8, 0.0), "f16": (torch.float16, 2.0 ** -11, 2.0 ** -25)}
SLACK = 1.0625
FLOOR = 8 * 2.0 ** -24


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import _lib, kernels
    _lib.load()
    return kernels


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


def operands(rows, D):
    g = torch.Generator().manual_seed(31 * D + rows)
    x = hostile_rows(rows, D, 100 + D + rows)
    y = torch.randn(rows, D, generator=g) * 3.0
    y[torch.arange(rows) % 4 == 3] = 0.0  # the all-zero class stays all zero
    ls = 0.1 + 0.05 * torch.randn(D, generator=g)
    ng = 1.0 + 0.3 * torch.randn(D, generator=g)
    return tuple(t.cuda().contiguous() for t in (x, y, ls, ng))


def row_err(got, ref):
    ref = ref.double()
    return (got.double() - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-300)


def check16(got16, x_out, ng, fmt, what):
    """the bound of the module docstring; returns the worst error / bound"""
    _, u, eta = FMT[fmt]
    ref = S.rms(x_out.double(), ng.double(), EPS)
    f32_bound = (4 * row_err(S.rms(x_out, ng, EPS), ref)).clamp_min(FLOOR)
    lim = SLACK * (u * ref.abs() + (f32_bound * ref.abs().amax(-1)).unsqueeze(-1) + eta)
    err = (got16.double() - ref).abs()
    worst = (err / lim.clamp_min(1e-300)).max().item()
    print(f"{what} [{fmt}]: worst error / bound {worst:.3f}")
    assert (err <= lim).all(), f"{what} [{fmt}]: {int((err > lim).sum())} elements over the bound, worst ratio {worst:.3f}"
    return worst


@pytest.mark.parametrize("fmt", list(FMT))
@pytest.mark.parametrize("D", DIMS)
def test_every_row_count(K, D, fmt):
    dt = FMT[fmt][0]
    worst = 0.0
    for rows in ROWS:
        x, y, ls, ng = operands(rows, D)
        what = f"D {D} rows {rows}"
        want = S.residual(x, y, ls)
        x_out, xn = K.residual_rmsnorm(x, y, ls, ng, EPS, xn_dtype=dt)
        assert xn.dtype == dt and xn.shape == x.shape and x_out.data_ptr() != x.data_ptr()
        assert torch.equal(x_out, want) and guarded.same_bits(x_out, want), f"{what}: x_out is not x + y * gamma"
        worst = max(worst, check16(xn, x_out, ng, fmt, what))
        zero = (torch.arange(rows) % 4 == 3).cuda()
        if zero.any():
            assert not x_out[zero].any() and not xn[zero].any(), "an all-zero row stays zero"
        # a null layer scale: x + y
        x_out0, xn0 = K.residual_rmsnorm(x, y, None, ng, EPS, xn_dtype=dt)
        assert guarded.same_bits(x_out0, S.residual(x, y)), f"{what}: x_out is not x + y"
        check16(xn0, x_out0, ng, fmt, what + " (no layer scale)")
        # the residual alone (behind the last block)
        for gamma in (ls, None):
            only, none = K.residual_rmsnorm(x, y, gamma, None, EPS)
            assert none is None and guarded.same_bits(only, S.residual(x, y, gamma)), f"{what}: the residual-only form"
        # in place, and the same bits twice
        xi = x.clone()
        r_out, r_xn = K.residual_rmsnorm(xi, y, ls, ng, EPS, out=xi, xn_dtype=dt)
        assert r_out is xi and guarded.same_bits(xi, x_out) and guarded.same_bits(r_xn, xn), f"{what}: in place"
        xi = x.clone()
        K.residual_rmsnorm(xi, y, None, None, EPS, out=xi)
        assert guarded.same_bits(xi, S.residual(x, y)), f"{what}: in place, residual only"
    print(f"D {D} [{fmt}]: worst error / bound over every row count {worst:.3f}")


def test_offset_rows_and_the_wrapper_refusals(K):
    """rows around 1e4 (their squares sum to 1e8 D: the mean is formed in f32 without cancellation) and what the wrapper refuses"""
    rows, D = 5, 384
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(rows, D, generator=g) + 1.0e4).cuda()
    y, ls, ng = torch.randn(rows, D, generator=g).cuda(), torch.full((D,), 0.5).cuda(), torch.ones(D).cuda()
    for fmt, (dt, _, _) in FMT.items():
        x_out, xn = K.residual_rmsnorm(x, y, ls, ng, EPS, xn_dtype=dt)
        assert guarded.same_bits(x_out, S.residual(x, y, ls))
        check16(xn, x_out, ng, fmt, "offset 1e4")
        assert ((xn.float() - 1.0).abs() < 2.0 ** -7).all(), "a row of 1e4 + noise normalises to 1"
    from simple_tad_amd._lib import TadError
    with pytest.raises(TadError, match="x_out may be x, it may not be y"):
        K.residual_rmsnorm(x, y, ls, ng, EPS, out=y)
    with pytest.raises(TadError, match="differ"):
        K.residual_rmsnorm(x, y[:4].contiguous(), ls, ng, EPS)
    with pytest.raises(TadError, match="expected torch.float32"):
        K.residual_rmsnorm(x.bfloat16(), y, ls, ng, EPS)


def test_planted_nan_stays_in_its_row(K):
    rows, D, r = 33, 384, 18
    x, y, ls, ng = operands(rows, D)
    x_out, xn = K.residual_rmsnorm(x, y, ls, ng, EPS)
    keep = torch.arange(rows).cuda() != r
    for which in ("x", "y"):
        xp, yp = x.clone(), y.clone()
        (xp if which == "x" else yp)[r, 100] = float("nan")
        p_out, p_xn = K.residual_rmsnorm(xp, yp, ls, ng, EPS)
        assert guarded.same_bits(p_out[keep], x_out[keep]) and guarded.same_bits(p_xn[keep], xn[keep]), which
        # the residual stream carries the NaN in its own element; the norm (a row statistic) spreads it over the row, no further
        nan = torch.isnan(p_out[r])
        assert nan[100] and int(nan.sum()) == 1 and torch.isnan(p_xn[r]).all(), which


@pytest.mark.parametrize("rows,D", [(5, 132), (5, 1792), (70, 2048)])
@pytest.mark.parametrize("poison", guarded.POISON_MODES)
def test_inside_poisoned_guard_bands(K, poison, rows, D):
    x, y, ls, ng = operands(rows, D)
    plain = {}
    for fmt, (dt, _, _) in FMT.items():
        plain[fmt] = K.residual_rmsnorm(x, y, ls, ng, EPS, xn_dtype=dt)
    only = K.residual_rmsnorm(x, y, None, None, EPS)[0]
    arena = guarded.GuardedArena(64 << 20, "cuda", poison=poison)
    xa, ya, la, na = (arena.place(t, role="input") for t in (x, y, ls, ng))
    xio = arena.place(x, role="inout")
    with arena.route(K):
        got = {fmt: K.residual_rmsnorm(xa, ya, la, na, EPS, xn_dtype=dt) for fmt, (dt, _, _) in FMT.items()}
        g_only = K.residual_rmsnorm(xa, ya, None, None, EPS)[0]
        g_in, g_in_xn = K.residual_rmsnorm(xio, ya, la, na, EPS, out=xio)
    arena.verify()
    for fmt in FMT:
        for a, b in zip(got[fmt], plain[fmt]):
            assert arena.contains(a) and guarded.same_bits(a, b)
    assert arena.contains(g_only) and guarded.same_bits(g_only, only)
    assert g_in is xio and guarded.same_bits(xio, plain["bf16"][0]) and guarded.same_bits(g_in_xn, plain["bf16"][1])
