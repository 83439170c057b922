"""Per-element numeric edges of the HIP kernels (the parity files compare whole tensors in two norms on randn-like inputs; an error
confined to a few elements, to small outputs or to inputs outside the bulk of a normal distribution passes them).

  A. fast-mode GELU / GELU' of every Linear plan that owns such an epilogue, and the precise mode's elementwise kernels, per element over
     the whole operand domain (all 65 536 bit patterns of the operand format, f32 sweeps with full mantissas, +-inf, NaN) against
     fp64 x Phi(x) and Phi(x) + x phi(x).  Bound: the polynomial's own error as tests/test_numeric_edges_cpu.py measures it in f32
     (edge_cases.CPU_F32, inside the bounds csrc/common.h states) plus four f32 ulps of the value.
  B. 16-bit stores of the epilogues are round-to-nearest-even bit for bit: the saved pre-activation against torch's cast of the exact f32
     value; 16-bit outputs of the Linear, LayerNorm forward and backward against the cast of their own f32 twins.
  C. LayerNorm forward / backward per row on rows with large common offsets, massive channels, extreme scales, sub-eps variance and
     constant rows, mixed in one launch; bound: 4x torch's own f32 error on the same rows (a one-pass variance is >= 100x outside).
  D. a planted inf / NaN reaches every output the same formula in torch makes non-finite (nothing swallowed), stays inside that blast
     radius (nothing spilled), through the split-K / slab routes too; at the end of the chain grad_norm_coef + adamw_step skip the step.

Run with -s to see the measured figures."""
import math

import pytest
import torch

import edge_cases as E
from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-3  # the parity files' tolerance for f32 outputs (tests/test_kernels_gpu.py), used outside a planted value's blast radius
ULP16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
FMTS = ["bf16", "f16"]


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import kernels
    from simple_tad_amd import _lib
    _lib.load()
    return kernels


def dev(t):
    return t.cuda().contiguous()


def gelu_plans(K):
    """every tile configuration gemm.hip / gemm_w4.hip instantiate with a GELU or GELU' epilogue (launch_nt_variant: 1 = 256 x 256, 3 = 256 x 128,
    7 = the four-wave 256 x 256 kernel, 2 / 4 / 5 = 128 x 128 / 128 x 64 / 64 x 64, 8 / 9 = 192 x 128 with eight / four waves), per tile and
    persistent, with the LDS-transposed and the register-layout epilogue, plus the planner's own choice"""
    base = dict(K.LINEAR_TUNING_DEFAULTS, persistent=0, direct_epilogue=0, split_tail=0, splitk_tail=0, short_k=0)
    plans = [("default", dict(K.LINEAR_TUNING_DEFAULTS))]
    for v, can_persist in ((1, True), (3, True), (7, True), (2, False), (4, False), (5, False), (8, False), (9, False)):
        for direct in ((0,) if v == 7 else (0, 2)):
            for persist in ((0, 1) if can_persist else (0,)):
                plans.append((f"v{v}" + ("_direct" if direct else "") + ("_persist" if persist else ""),
                              dict(base, variant=v, direct_epilogue=direct, persistent=persist)))
    return plans


def same_bits(a, b):
    """equal bit for bit, NaNs compared as NaNs (their payload is not part of any contract)"""
    iv = torch.int16 if a.element_size() == 2 else torch.int32
    an, bn = torch.isnan(a), torch.isnan(b)
    return bool((an == bn).all()) and bool((a.view(iv) == b.view(iv))[~an].all())


def check_fast(got, x, fmt, kind, what, bound=None):
    """got = gelu(x) or gelu'(x) per element (f32 tensors on one device) against fp64; returns the measured figure"""
    x, got = x.flatten(), got.flatten()
    # (beyond 3.39e38, above the largest bf16 value, x Phi~ may overflow where x Phi does not: Phi~ <= 1 + 2.4e-5)
    fin = torch.isfinite(x) & (x.abs() <= 3.39e38)
    xd, g = x[fin].double(), got[fin].double()
    c = E.CPU_F32[(fmt, kind)] if bound is None else bound
    if kind == "gelu":
        ref, scale = E.gelu64(xd), xd.abs().clamp_min(1.0)
        inf = torch.isinf(x)
        assert not torch.isfinite(got[inf]).any(), f"{what}: an infinite pre-activation gave a finite output"
        assert torch.isnan(got[torch.isnan(x)]).all(), f"{what}: a NaN pre-activation must give a NaN output"
    else:
        ref, scale = E.dgelu64(xd), torch.ones_like(xd)
    assert torch.isfinite(g).all(), f"{what}: non-finite output for a finite input"
    err = (g - ref).abs()
    lim = c * scale + (4 * E.ulp32(ref) if bound is None else 0.0)
    fig, i = (err / scale).max(0)
    print(f"{what}: max |error|{' / max(1, |x|)' if kind == 'gelu' else ''} {fig.item():.3e} at x = {xd[i].item():.9g} (bound {c:.3e})")
    over = err > lim
    assert not over.any(), f"{what}: {int(over.sum())} elements over the bound, worst {fig.item():.3e} at x = {xd[i].item():.9g} (bound {c:.3e})"
    return fig.item()


# ================================================================== A + B: forward
@pytest.mark.parametrize("fmt", FMTS)
def test_gelu_forward_bias_sweep_every_plan(K, fmt):
    """x = 0 and the sweep in the f32 bias: the pre-activation IS the bias (+0 accumulator: a -0 bias gives +0).  300 rows cross every row
    tile raggedly; 385+ column tiles of 256 put the persistent kernels on.  Per plan: all rows equal bit for bit; gelu per element against
    fp64 (A); the saved 16-bit pre-activation equals torch's cast of the f32 value and the 16-bit output equals the cast of the f32 output
    of the same plan, as int16 (B).
    Measured on an MI355X, every plan: 2.378e-05 (bf16, bound 2.39e-05) and 3.832e-07 (f16, bound 3.9e-07), times max(1, |x|) -- the CPU evaluation's figures to
    the printed digits."""
    dt = E.OP16[fmt]
    bias = dev(E.bias_sweep(fmt))
    N, M, Kd = bias.numel(), 300, 128
    x, w = torch.zeros(M, Kd, dtype=dt, device="cuda"), torch.zeros(N, Kd, dtype=dt, device="cuda")
    pre32 = bias + 0.0
    pre_ref = pre32.to(dt)
    K.set_operand_dtype(dt)
    first = None
    try:
        for name, cfg in gelu_plans(K):
            K.linear_tuning(**cfg)
            y, pre = K.linear_fwd(x, w, bias, out_dtype=torch.float32, epilogue=K.EPI_BIAS_GELU, want_preact=True)
            y16, _ = K.linear_fwd(x, w, bias, out_dtype=dt, epilogue=K.EPI_BIAS_GELU)
            p16, _ = K.linear_fwd(x, w, bias, out_dtype=dt)
            torch.cuda.synchronize()
            assert same_bits(y, y[:1].expand_as(y)) and same_bits(pre, pre[:1].expand_as(pre)), f"{name}: rows differ"
            assert same_bits(pre[0], pre_ref), f"{name}: saved pre-activation is not RNE of the f32 value"
            assert same_bits(p16[0], pre_ref) and same_bits(p16, p16[:1].expand_as(p16)), f"{name}: 16-bit bias-only output is not RNE of the f32 value"
            assert same_bits(y16, y.to(dt)), f"{name}: 16-bit gelu output is not RNE of the f32 output"
            if first is None:
                first = y[0].clone()
                check_fast(first, pre32, fmt, "gelu", f"gelu fwd {fmt} bias sweep")
            elif not same_bits(y[0], first):  # (a plan with other bits is measured on its own)
                check_fast(y[0], pre32, fmt, "gelu", f"gelu fwd {fmt} bias sweep, {name}")
    finally:
        K.linear_tuning(**K.LINEAR_TUNING_DEFAULTS)
        K.set_operand_dtype(torch.bfloat16)


@pytest.mark.parametrize("fmt", FMTS)
def test_gelu_forward_one_hot_selects_every_16bit_weight(K, fmt):
    """one-hot x rows select one 16-bit weight each, bias 0: the pre-activation is that weight exactly (every finite pattern of the format;
    the non-finite ones are left out -- 0 x inf is NaN in the other rows' sums)"""
    dt = E.OP16[fmt]
    pat = E.op16_patterns(fmt)
    pat = torch.where(torch.isfinite(pat.float()), pat, torch.zeros_like(pat))
    w = dev(pat.reshape(512, 128))
    M = 198
    sel = torch.arange(M) % 128
    x = torch.zeros(M, 128, dtype=dt)
    x[torch.arange(M), sel] = 1.0
    x = dev(x)
    pre32 = w.float().t()[sel.cuda()].contiguous() + 0.0  # [M, 512]
    bias = torch.zeros(512, device="cuda")
    K.set_operand_dtype(dt)
    try:
        for name, cfg in gelu_plans(K):
            K.linear_tuning(**cfg)
            y, pre = K.linear_fwd(x, w, bias, out_dtype=torch.float32, epilogue=K.EPI_BIAS_GELU, want_preact=True)
            torch.cuda.synchronize()
            assert same_bits(pre, pre32.to(dt)), f"{name}: saved pre-activation differs from the selected weight"
            check_fast(y, pre32, fmt, "gelu", f"gelu fwd {fmt} one-hot, {name}")
    finally:
        K.linear_tuning(**K.LINEAR_TUNING_DEFAULTS)
        K.set_operand_dtype(torch.bfloat16)


# ================================================================== A: backward
@pytest.mark.parametrize("fmt", FMTS)
def test_gelu_grad_every_bit_pattern_every_plan(K, fmt):
    """linear_bwd_input with one-hot dy rows against a wT of ones: every product is exactly 1.0, the output is gelu'(h).  h walks all 65 536
    bit patterns of the format over 582 x 33 024 outputs (ragged over every row tile; 3 x 129 tiles of 256 x 256: the persistent kernels
    run), each pattern at ~290 positions: every position must give the bits of the pattern's first one, and those 65 536 values are held to
    fp64 (+-inf: the limits 1 and 0).  A NaN h gives a FINITE gelu' (the clamp drops it: DESIGN.md section 4) -- not asserted either way.
    Measured on an MI355X, every plan (all bit-identical): 1.049e-04 at 4.5 (bf16, bound 1.05e-04), 6.005e-06 at -10.0625 (f16, bound 6.01e-06)."""
    dt = E.OP16[fmt]
    M, Kout, Nred = 582, 33024, 128
    pat = dev(E.op16_patterns(fmt))
    idx = torch.arange(M * Kout, device="cuda") % 65536
    h = pat[idx].reshape(M, Kout).contiguous()
    dy = torch.zeros(M, Nred, dtype=dt)
    dy[torch.arange(M), torch.arange(M) % Nred] = 1.0
    dy = dev(dy)
    wT = torch.ones(Kout, Nred, dtype=dt, device="cuda")
    x = pat.float()
    first = None
    K.set_operand_dtype(dt)
    try:
        for name, cfg in gelu_plans(K):
            K.linear_tuning(**cfg)
            out = K.linear_bwd_input(dy, wT, out_dtype=torch.float32, gelu_preact=h)
            out16 = K.linear_bwd_input(dy, wT, out_dtype=dt, gelu_preact=h)
            torch.cuda.synchronize()
            lut = out.flatten()[:65536].clone()
            assert same_bits(out.flatten(), lut[idx]), f"{name}: gelu' of one bit pattern depends on its position"
            assert same_bits(out16, out.to(dt)), f"{name}: 16-bit output is not RNE of the f32 output"
            if first is None or not same_bits(lut, first):
                fin = torch.isfinite(x)
                check_fast(lut[fin], x[fin], fmt, "dgelu", f"gelu' {fmt}, {name}")
                for v, lim in ((float("inf"), 1.0), (float("-inf"), 0.0)):
                    assert abs(lut[x == v].item() - lim) <= E.CPU_F32[(fmt, "dgelu")], (name, v, lut[x == v].item())
                first = lut if first is None else first
    finally:
        K.linear_tuning(**K.LINEAR_TUNING_DEFAULTS)
        K.set_operand_dtype(torch.bfloat16)


def test_precise_mode_gelu_kernels_per_element(K):
    """gelu_f32 / gelu_bwd_f32 (erff) on the f32 sweeps of both formats: <= 1.5e-7 max(1, |x|) and (our bound, edge_cases.PRECISE_DGELU) 4e-7.
    Measured on an MI355X: 1.048e-07 at 1.205 and 1.340e-07 at 1.375."""
    x = dev(torch.cat([E.f32_sweep("bf16"), E.f32_sweep("f16")]))
    check_fast(K.gelu_f32(x), x, "f32", "gelu", "precise gelu", bound=E.PRECISE_GELU)
    check_fast(K.gelu_bwd_f32(torch.ones_like(x), x), x, "f32", "dgelu", "precise gelu'", bound=E.PRECISE_DGELU)
    nf = torch.tensor([float("inf"), float("-inf"), float("nan")], device="cuda")
    assert not torch.isfinite(K.gelu_f32(nf)[[0, 2]]).any()


# ================================================================== B: a Linear's 16-bit output on real sums
@pytest.mark.parametrize("fmt", FMTS)
def test_linear_16bit_output_is_rne_of_its_f32_twin(K, fmt):
    """random operands, ragged M and N, every epilogue with a 16-bit output: the 16-bit launch stores RNE of what the f32 launch stores (the
    two share the plan and the arithmetic at these shapes; bit for bit)"""
    dt = E.OP16[fmt]
    g = torch.Generator().manual_seed(5)
    for M, N, Kd in ((300, 388, 128), (2500, 768, 256)):
        x, w = dev(torch.randn(M, Kd, generator=g)).to(dt), dev(torch.randn(N, Kd, generator=g) * 0.05).to(dt)
        b = dev(torch.randn(N, generator=g))
        for epi in (K.EPI_BIAS, K.EPI_BIAS_GELU):
            y32, _ = K.linear_fwd(x, w, b, out_dtype=torch.float32, epilogue=epi)
            y16, _ = K.linear_fwd(x, w, b, out_dtype=dt, epilogue=epi)
            assert same_bits(y16, y32.to(dt)), (M, N, Kd, epi)
        dx32, dx16 = K.linear_bwd_input(x, w, out_dtype=torch.float32), K.linear_bwd_input(x, w)  # (x as dy [M, Kd], w as wT [N, Kd])
        assert same_bits(dx16, dx32.to(dt))


# ================================================================== C
@pytest.mark.parametrize("D", E.LN_DIMS)
def test_layernorm_hostile_rows_per_row(K, D):
    """Eight row classes interleaved in one launch of 129 rows (edge_cases.ln_rows), each row against fp64 on its own; bounds per class from
    torch's f32 error on the same rows (edge_cases.ln_bounds; the table: test_numeric_edges_cpu.py -s).
    Measured on an MI355X, D = 768, y error / bound: offset1e3 2.6e-05 / 1.09e-04, offset1e4 3.1e-04 / 1.53e-03, tight1e3 3.1e-03 / 1.11e-02, the other
    classes <= 1.6e-07 / 9.54e-07; dx: 2.8e-06 / 5.1e-05, 7.1e-05 / 8.0e-04, 4.5e-04 / 6.8e-03, <= 2.0e-07 / 9.54e-07; worst ratio over all D: y 0.38 (offset1e3, D 1280)."""
    x, gamma, beta, dy, dres, cls = E.ln_rows(D)
    bnd = E.ln_bounds(D)
    y_ref, mean_ref, rstd_ref, dx_ref, dg_ref, db_ref, dg_abs, db_abs = E.ln_ref(x, gamma, beta, dy)
    xd, gd, bd = dev(x), dev(gamma), dev(beta)
    y32, mean, rstd = K.layernorm_fwd(xd, gd, bd, E.LN_EPS, out_dtype=torch.float32)
    e_y = E.row_relmax(y32.cpu(), y_ref)
    e_rs = (rstd.cpu().double() - rstd_ref).abs() / rstd_ref
    e_mu = (mean.cpu().double() - mean_ref).abs()
    for c, name in enumerate(E.LN_CLASSES):
        print(f"D {D} {name}: y {e_y[cls == c].max():.2e} / {bnd['y'][c]:.2e}, rstd {e_rs[cls == c].max():.2e} / {bnd['rstd'][c]:.2e}")
    assert (e_y <= bnd["y"][cls]).all(), f"y: rows {torch.nonzero(e_y > bnd['y'][cls]).flatten().tolist()} (class = row % 8) over their bound"
    assert (e_rs <= bnd["rstd"][cls]).all(), f"rstd: rows {torch.nonzero(e_rs > bnd['rstd'][cls]).flatten().tolist()} over their bound"
    assert (e_mu <= E.mean_bound(x)).all(), f"mean: rows {torch.nonzero(e_mu > E.mean_bound(x)).flatten().tolist()} over their bound"
    const = cls == E.LN_CLASSES.index("const")
    assert torch.equal(y32.cpu()[const], beta.expand(int(const.sum()), D)), "a constant row must give beta exactly"
    r0 = 1.0 / math.sqrt(float(torch.tensor(E.LN_EPS, dtype=torch.float32)))
    assert ((rstd.cpu()[const].double() - r0).abs() <= 2 * E.ulp32(torch.tensor(r0, dtype=torch.float64))).all(), "rstd of a constant row: eps^-1/2 to 2 ulp"
    for fmt, dt in E.OP16.items():  # B: the 16-bit output is RNE of the f32 output
        y16, m16, r16 = K.layernorm_fwd(xd, gd, bd, E.LN_EPS, out_dtype=dt)
        assert same_bits(y16, y32.to(dt)) and torch.equal(m16, mean) and torch.equal(r16, rstd), fmt
    # backward with the forward's own statistics
    dx, _, dg, db, _ = K.layernorm_bwd(dev(dy), xd, gd, mean, rstd)
    e_dx = E.row_relmax(dx.cpu(), dx_ref)
    for c, name in enumerate(E.LN_CLASSES):
        print(f"D {D} {name}: dx {e_dx[cls == c].max():.2e} / {bnd['dx'][c]:.2e}")
    assert (e_dx <= bnd["dx"][cls]).all(), f"dx: rows {torch.nonzero(e_dx > bnd['dx'][cls]).flatten().tolist()} over their bound"
    e_dg, e_db = (dg.cpu().double() - dg_ref).abs() / dg_abs, (db.cpu().double() - db_ref).abs() / db_abs
    print(f"D {D}: dgamma {e_dg.max():.2e} / {bnd['dgamma']:.2e}, dbeta {e_db.max():.2e} / {bnd['dbeta']:.2e} (per column)")
    assert (e_dg <= bnd["dgamma"]).all() and (e_db <= bnd["dbeta"]).all()
    # + residual gradient, 16-bit copy, column sums
    dx2, dxb, dg2, db2, cs = K.layernorm_bwd(dev(dy), xd, gd, mean, rstd, dres=dev(dres), want_bf16=True, want_colsum=True)
    ref2 = dx_ref + dres.double()
    lim = bnd["dx"][cls] * dx_ref.abs().amax(-1) + E.F32_EPS * ref2.abs().amax(-1)  # dx's own bound + one rounding of the sum
    assert ((dx2.cpu().double() - ref2).abs().amax(-1) <= lim).all(), "dx + dres"
    assert same_bits(dxb, dx2.to(dxb.dtype)), "the 16-bit copy of dx is not RNE of the f32 dx"
    assert ((dg2.cpu().double() - dg_ref).abs() / dg_abs <= bnd["dgamma"]).all() and ((db2.cpu().double() - db_ref).abs() / db_abs <= bnd["dbeta"]).all()
    e_cs = (cs.cpu().double() - ref2.sum(0)).abs() / ref2.abs().sum(0)
    print(f"D {D}: colsum {e_cs.max():.2e} / {bnd['colsum']:.2e}")
    assert (e_cs <= bnd["colsum"]).all()


# ================================================================== D
def check_planted(got, ref, radius, what, tol=TOL):
    """the kernel's non-finite mask contains the reference's (nothing swallowed) and stays inside `radius` (nothing spilled); outside the
    radius the values are the file's tolerance from the reference (max norm over those finite elements)"""
    got, ref, radius = got.detach().double(), ref.to(got.device).double(), radius.to(got.device)
    bad_got, bad_ref = ~torch.isfinite(got), ~torch.isfinite(ref)
    assert bad_ref.any(), f"{what}: the reference has no non-finite output -- the case tests nothing"
    assert not (bad_ref & ~radius).any(), f"{what}: the reference itself leaves the stated radius"
    assert not (bad_ref & ~bad_got).any(), f"{what}: {int((bad_ref & ~bad_got).sum())} non-finite outputs swallowed"
    assert not (bad_got & ~radius).any(), f"{what}: {int((bad_got & ~radius).sum())} non-finite outputs outside the blast radius"
    keep = ~radius
    if keep.any():
        e = ((got[keep] - ref[keep]).abs().max() / ref[keep].abs().max().clamp_min(1e-30)).item()
        assert e <= tol, f"{what}: outside the radius {e:.3e} > {tol}"


def row_mask(shape, i):
    m = torch.zeros(shape, dtype=torch.bool)
    m[i] = True
    return m


def planted_cases(shape):
    """(position, value): the first element and the last element of the (ragged) last row, +inf then NaN"""
    last = tuple(s - 1 for s in shape)
    return [(pos, v) for v in E.NONFINITE for pos in ((0,) * len(shape), last)]


LIN_SMALL = (70, 408, 128)  # M, N, Kd: ragged rows and columns on every tile (N a multiple of 8 and of 3: the weight-gradient GEMM, the qkv bias split)


@pytest.mark.parametrize("M,N,Kd,route,fmt", [LIN_SMALL + ("small", "bf16"), LIN_SMALL + ("small", "f16"), (50176 - 37, 3072, 768, "splitk", "bf16")])
def test_planted_nonfinite_linear_bwd_input(K, M, N, Kd, route, fmt):
    """dx = dy W (x gelu'(h)): a non-finite dy element makes its row of dx non-finite and no other; `splitk`: the last rows run as the
    split-K tail of test_linear_splitk_tail_matches_the_single_launch_plans (partial tiles through a workspace)"""
    dt = E.OP16[fmt]
    g = torch.Generator().manual_seed(M + N)
    dy = dev(torch.randn(M, N, generator=g)).to(dt)
    w = dev(torch.randn(N, Kd, generator=g) * 0.05).to(dt)
    h = dev(torch.randn(M, Kd, generator=g) * 1.5).to(dt)
    wT = w.t().contiguous()
    try:
        if route == "splitk":
            K.linear_tuning(**{**K.LINEAR_TUNING_DEFAULTS, "splitk_tail": 2, "split_tail": 2})
        for pos, v in planted_cases((M, N)):
            dyp = E.plant(dy, pos, v)
            ref = dyp.double() @ w.double()
            n0 = K.linear_kernel_launches()
            check_planted(K.linear_bwd_input(dyp, wT, out_dtype=torch.float32), ref, row_mask((M, Kd), pos[0]), f"dx {route} {pos} {v}")
            if route == "splitk":
                assert K.linear_kernel_launches() - n0 == 3, "the split-K tail did not run"
            check_planted(K.linear_bwd_input(dyp, wT).float(), ref, row_mask((M, Kd), pos[0]), f"dx 16-bit {route} {pos} {v}", tol=ULP16[fmt])
            refg = ref * E.dgelu64(h.double())
            check_planted(K.linear_bwd_input(dyp, wT, out_dtype=torch.float32, gelu_preact=h), refg, row_mask((M, Kd), pos[0]), f"dx gelu' {route} {pos} {v}")
        # a NaN in h alone is clamped away (finite gelu'); together with a non-finite dy the row still carries dy's
        hp = E.plant(h, (0, 0), float("nan"))
        out = K.linear_bwd_input(E.plant(dy, (0, 0), float("inf")), wT, out_dtype=torch.float32, gelu_preact=hp)
        assert not torch.isfinite(out[0]).any() and torch.isfinite(out[1:]).all()
    finally:
        K.linear_tuning(**K.LINEAR_TUNING_DEFAULTS)


@pytest.mark.parametrize("M,N,Kd,route,fmt", [LIN_SMALL + ("small", "bf16"), LIN_SMALL + ("small", "f16"), (25088 + 70, 2304, 768, "slabs", "bf16")])
def test_planted_nonfinite_linear_bwd_weight(K, M, N, Kd, route, fmt):
    """dW = dy^T x, db = colsum(dy): a non-finite dy[i, j] makes row j of dW and db[j] non-finite and nothing else -- plain, accumulate, the qkv
    entry point with its split bias, the pair launch; `slabs`: the rows are reduced in slabs through the workspace (the shape of
    test_weight_gradient_four_wave_kernel_is_bit_identical), eight- and four-wave kernels"""
    dt = E.OP16[fmt]
    g = torch.Generator().manual_seed(M + N + 1)
    dy = dev(torch.randn(M, N, generator=g)).to(dt)
    x = dev(torch.randn(M, Kd, generator=g)).to(dt)
    N2 = 256 if route == "small" else 768
    dy2 = dev(torch.randn(M, N2, generator=g)).to(dt)
    ref2 = dy2.double().t() @ x.double()
    third = N // 3 if N % 3 == 0 else None
    try:
        for tn_w4 in ((1,) if route == "small" else (1, 0)):
            K.linear_tuning(**{**K.LINEAR_TUNING_DEFAULTS, "tn_w4": tn_w4})
            for pos, v in planted_cases((M, N)):
                what = f"{route} w4={tn_w4} {pos} {v}"
                dyp = E.plant(dy, pos, v)
                ref, refb = dyp.double().t() @ x.double(), dyp.double().sum(0)
                rW, rb = row_mask((N, Kd), pos[1]), row_mask((N,), pos[1])
                dW, db = K.linear_bwd_weight(dyp, x)
                check_planted(dW, ref, rW, "dW " + what)
                check_planted(db, refb, rb, "db " + what)
                dW, db = K.linear_bwd_weight(dyp, x, dW=torch.full((N, Kd), 0.5, device="cuda"), db=torch.full((N,), 0.25, device="cuda"), accumulate=True)
                check_planted(dW, ref + 0.5, rW, "dW accumulate " + what)
                check_planted(db, refb + 0.25, rb, "db accumulate " + what)
                if third:
                    for acc in (False, True):
                        dWq, dq, dv = (torch.full(s, 0.5 if acc else 7.0, device="cuda") for s in ((N, Kd), (third,), (third,)))
                        K.linear_bwd_weight_qkv(dyp, x, dWq, dq, dv, accumulate=acc)
                        check_planted(dWq, ref + (0.5 if acc else 0.0), rW, "dW qkv " + what)
                        got_b = torch.cat([dq, torch.zeros(third, device="cuda"), dv])
                        ref_b = refb + (0.5 if acc else 0.0)
                        ref_b[third:2 * third] = 0.0
                        if third <= pos[1] < 2 * third:
                            assert torch.isfinite(got_b).all()  # (the k third has no bias)
                        else:
                            check_planted(got_b, ref_b, rb, "dq / dv bias " + what)
                for acc in (False, True):
                    dW1, db1, dW2 = (torch.full(s, 0.5 if acc else 7.0, device="cuda") for s in ((N, Kd), (N,), (N2, Kd)))
                    K.linear_bwd_weight_pair(dyp, x, dW1, db1, None, dy2, x, dW2, accumulate=acc)
                    check_planted(dW1, ref + (0.5 if acc else 0.0), rW, "dW1 pair " + what)
                    check_planted(db1, refb + (0.5 if acc else 0.0), rb, "db1 pair " + what)
                    assert torch.isfinite(dW2).all(), "the pair's second problem caught the first one's non-finite value"
                    e = ((dW2.double() - ref2 - (0.5 if acc else 0.0)).abs().max() / ref2.abs().max()).item()
                    assert e <= TOL, e
    finally:
        K.linear_tuning(**K.LINEAR_TUNING_DEFAULTS)


@pytest.mark.parametrize("D", [384, 768])
def test_planted_nonfinite_layernorm_bwd(K, D):
    """a non-finite dy[i, j]: row i of dx (both row sums carry it), column j of dgamma / dbeta, all of colsum(dx)"""
    g = torch.Generator().manual_seed(D)
    R = 70
    x, dy, dres = (torch.randn(R, D, generator=g) for _ in range(3))
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    xd, gd = dev(x), dev(gamma)
    _, mean, rstd = K.layernorm_fwd(xd, gd, dev(beta), E.LN_EPS, out_dtype=torch.float32)
    for pos, v in planted_cases((R, D)):
        dyp = E.plant(dy, pos, v)
        _, _, _, dx_ref, dg_ref, db_ref, _, _ = E.ln_ref(x, gamma, beta, dyp)
        for dyk in (dev(dyp), dev(dyp).to(torch.bfloat16)):
            if dyk.dtype != torch.float32:
                _, _, _, dx_ref, dg_ref, db_ref, _, _ = E.ln_ref(x, gamma, beta, dyk.float().cpu())
            dx, dxb, dg, db, cs = K.layernorm_bwd(dyk, xd, gd, mean, rstd, dres=dev(dres), want_bf16=True, want_colsum=True)
            what = f"ln bwd {dyk.dtype} {pos} {v}"
            check_planted(dx, dx_ref + dres.double(), row_mask((R, D), pos[0]), "dx " + what)
            check_planted(dxb.float(), dx_ref + dres.double(), row_mask((R, D), pos[0]), "dx 16-bit " + what, tol=ULP16["bf16"])
            check_planted(dg, dg_ref, row_mask((D,), pos[1]), "dgamma " + what)
            check_planted(db, db_ref, row_mask((D,), pos[1]), "dbeta " + what)
            check_planted(cs, (dx_ref + dres.double()).sum(0), torch.ones(D, dtype=torch.bool), "colsum " + what)


def _attn_radius(B, N, H, d, b, h):
    m = torch.zeros(B, N, 3, H, d, dtype=torch.bool)
    m[b, :, :, h] = True
    return m.reshape(B * N, 3 * H * d)


@pytest.mark.parametrize("d", [64, 80])
@pytest.mark.parametrize("kind", ["bf16", "f16", "f32"])
def test_planted_nonfinite_attention_bwd(K, kind, d):
    """a non-finite dout element: dq of its query row, dk of every key and its own column of dv become non-finite in the fp64 formula; the
    kernels must produce at least those and nothing outside the (clip, head)"""
    B, N, H = 2, 100, 2
    scale = d ** -0.5
    g = torch.Generator().manual_seed(d)
    dt = torch.float32 if kind == "f32" else E.OP16[kind]
    qkv = torch.randn(B * N, 3 * H * d, generator=g).to(dt)
    dout = torch.randn(B * N, H * d, generator=g).to(dt)
    qd = dev(qkv)
    if kind == "f32":
        out, lse = K.attn_fwd_f32(qd, B, N, H, scale, want_lse=True, d=d)
    else:
        out, lse = K.attn_fwd(qd, B, N, H, scale, d=d)
    for (b, n, h, e), v in planted_cases((B, N, H, d)):
        dop = E.plant(dout.reshape(B, N, H, d), (b, n, h, e), v).reshape(B * N, H * d)
        q = qkv.double().reshape(B, N, -1).requires_grad_()
        O.attention_core(q, H, scale).backward(dop.double().reshape(B, N, -1))
        ref = q.grad.reshape(B * N, -1)
        if kind == "f32":
            got = K.attn_bwd_f32(qd, out, dev(dop), lse, B, N, H, scale, d=d)
        else:
            got = K.attn_bwd(qd, out, dev(dop), lse, B, N, H, scale, d=d)
        check_planted(got.float(), ref, _attn_radius(B, N, H, d, b, h), f"attn_bwd {kind} d={d} {(b, n, h, e)} {v}",
                      tol=1e-5 if kind == "f32" else (2 if kind == "bf16" else 4) * ULP16[kind])  # (the parity files' 2 x 2^-8 / 2.4e-3)


def test_planted_nonfinite_reductions_and_losses(K):
    g = torch.Generator().manual_seed(11)
    # meanpool_bwd: the clip
    B, N, D = 3, 197, 384
    dy = torch.randn(B, D, generator=g)
    for pos, v in planted_cases((B, D)):
        dyp = E.plant(dy, pos, v)
        dx, dxb = K.meanpool_bwd(dev(dyp), N, want_bf16=True)
        ref = (dyp.double() / N)[:, None, :].expand(B, N, D)
        rad = torch.zeros(B, N, D, dtype=torch.bool)
        rad[pos[0]] = True
        check_planted(dx, ref, rad, f"meanpool_bwd {pos} {v}", tol=1e-6)
        check_planted(dxb.float(), ref, rad, f"meanpool_bwd 16-bit {pos} {v}", tol=ULP16["bf16"])
    # column sums: the column
    for M, Nc in ((1027, 264), (5000, 776)):  # (16-bit column sums take N in multiples of 8)
        a = torch.randn(M, Nc, generator=g)
        for pos, v in planted_cases((M, Nc)):
            ap = E.plant(a, pos, v)
            rad = row_mask((Nc,), pos[1])
            check_planted(K.colsum_f32(dev(ap)), ap.double().sum(0), rad, f"colsum_f32 {pos} {v}", tol=1e-5)
            for fmt, dt in E.OP16.items():
                a16 = ap.to(dt)
                check_planted(K.colsum_bf16(dev(a16)), a16.double().sum(0), rad, f"colsum {fmt} {pos} {v}", tol=1e-5)
    a = torch.randn(3, 50, 264, generator=g)
    r0, rc = 5, 41
    for pos, v in [((0, r0, 0), float("inf")), ((2, r0 + rc - 1, 263), float("nan")), ((2, r0 + rc - 1, 263), float("inf")), ((0, r0, 0), float("nan"))]:
        ap = E.plant(a, pos, v)
        check_planted(K.colsum_window_f32(dev(ap), r0, rc), ap[:, r0:r0 + rc].double().sum((0, 1)), row_mask((264,), pos[2]), f"colsum_window {pos} {v}", tol=1e-5)
    # a value outside the window is not read
    assert torch.isfinite(K.colsum_window_f32(dev(E.plant(a, (1, r0 + rc, 7), float("nan"))), r0, rc)).all()
    # losses: the sample (and the batch-mean loss)
    Bn, C = 7, 400
    z = torch.randn(Bn, C, generator=g)
    t = torch.softmax(torch.randn(Bn, C, generator=g), -1)
    for pos, v in planted_cases((Bn, C)):
        zp = E.plant(z, pos, v).double().requires_grad_()
        loss_ref = (-t.double() * torch.log_softmax(zp, -1)).sum(-1).mean()
        loss_ref.backward()
        loss, dz = K.soft_target_ce(dev(zp.detach().float()), target=dev(t))
        assert not math.isfinite(loss.item()) and not math.isfinite(loss_ref.item())
        check_planted(dz, zp.grad, row_mask((Bn, C), pos[0]), f"soft_target_ce {pos} {v}", tol=1e-5)
    p, tg = torch.randn(Bn, 1536, generator=g), torch.randn(Bn, 1536, generator=g)
    for pos, v in planted_cases((Bn, 1536)):
        pp = E.plant(p, pos, v)
        loss, grad = K.mse_loss(dev(pp), dev(tg))
        assert not math.isfinite(loss.item())
        check_planted(grad, 2 * (pp.double() - tg.double()) / p.numel(), row_mask((Bn, 1536), pos[0]), f"mse_loss {pos} {v}", tol=1e-6)


@pytest.mark.parametrize("mirror", FMTS)
def test_planted_nonfinite_gradient_skips_the_adamw_step(K, mirror):
    """end of the chain: a weight gradient that carries a planted value (through linear_bwd_weight) goes through grad_norm_coef and a one-group
    adamw_step -- the coefficient is zero or non-finite and p, m, v and the 16-bit mirror keep their bits; the same step with the
    finite gradient does move them (the check is not vacuous)"""
    M, N, Kd = LIN_SMALL
    g = torch.Generator().manual_seed(3)
    dy, x = dev(torch.randn(M, N, generator=g)).to(torch.bfloat16), dev(torch.randn(M, Kd, generator=g)).to(torch.bfloat16)
    n = N * Kd
    chunks = -(-n // 4096)
    cg = torch.zeros(chunks, dtype=torch.uint8, device="cuda")
    p0, m0, v0 = dev(torch.randn(n, generator=g)), dev(torch.randn(n, generator=g) * 0.01), dev(torch.rand(n, generator=g) * 1e-4)

    def step(grad):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        p16 = p.to(E.OP16[mirror])
        before = [t.clone() for t in (p, m, v, p16)]
        coef = K.grad_norm_coef(grad, 1.0 / 65536.0, 1.0)
        K.adamw_step(p, grad, m, v, cg, [1e-3], [0.05], [1], 0.9, 0.999, 1e-8, param_bf16=p16, grad_scale=coef[1:2])
        torch.cuda.synchronize()
        return coef.cpu(), [same_bits(a, b) for a, b in zip((p, m, v, p16), before)]

    for pos, v in planted_cases((M, N)):
        dW, _ = K.linear_bwd_weight(E.plant(dy, pos, v), x)
        coef, kept = step(dW.flatten().contiguous())
        assert coef[1].item() == 0.0 or not math.isfinite(coef[1].item()), (pos, v, coef)
        assert coef[2].item() == 1.0 and all(kept), (pos, v, coef, kept)
    dW, _ = K.linear_bwd_weight(dy, x)
    coef, kept = step(dW.flatten().contiguous())
    assert math.isfinite(coef[1].item()) and coef[1].item() > 0 and coef[2].item() == 0.0 and not any(kept)
