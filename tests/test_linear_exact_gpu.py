"""The Linear GEMMs held to the truth bit for bit (helper and case table: tests/linear_exact.py; the conditions on the inputs and the reach of
the table: tests/test_linear_exact_cpu.py).

Operands are small integers, exact in bf16 and in half, with sum |x||w| + |bias| + |residual| < 2^24: every partial sum in ANY order is an
integer below 2^24, exact in f32, so every output of gemm_nt / gemm_tn -- every tile configuration, the persistent walk, the split-K tail in
its three modes, the slab reduction at any share count, the pair launch, accumulate mode -- must equal the integer reference bit for bit over
the WHOLE tensor (16-bit outputs: the reference rounded once).  A dropped, doubled or misplaced term, a partial sum that went through 16 bits,
a bias or residual added behind a rounding, a combine in the wrong type: each is a wrong integer.  The references are fp64 products of the
same integers on the device (any order of them is exact below 2^53).  The GELU epilogues and the non-power-of-two gamma / rowscale are held
to derived per-element bounds on top of an exact accumulator.

A mismatch is reported as the first failing (row, column) and its difference from the reference (linear_exact.first_mismatch)."""
import contextlib

import pytest
import torch

import edge_cases as E
import linear_exact as X

pytestmark = pytest.mark.gpu
FMTS = ["bf16", "f16"]


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import _lib, kernels
    _lib.load()
    return kernels


@pytest.fixture(autouse=True)
def knobs_stay_put(K):
    yield
    moved = {k: K.linear_tuning_get(k) for k, v in K.LINEAR_TUNING_DEFAULTS.items() if K.linear_tuning_get(k) != v}
    assert not moved, f"a test left knobs moved: {moved}"


@contextlib.contextmanager
def tuned(K, cfg):
    try:
        K.linear_tuning(**{**K.LINEAR_TUNING_DEFAULTS, **cfg})
        yield
    finally:
        K.linear_tuning(**K.LINEAR_TUNING_DEFAULTS)


def cases(pred):
    sel = [c for c in X.CASES if pred(c)]
    return pytest.mark.parametrize("case", sel, ids=[c["id"] for c in sel])


def ints(t):
    """an int64 tensor of small integers on the device (as int32: a quarter of the transfer)"""
    return t.to(torch.int32).cuda()


def op16(ti, dt, scale=1.0):
    """device integers -> the operand format, times a power of two (both steps exact: test_linear_exact_cpu.py)"""
    t = ti.to(dt)
    return t if scale == 1.0 else t * scale


def f32(t, scale=1.0):
    """an integer tensor (times a power of two) as f32 on the device"""
    return None if t is None else (t.double() * scale).float().cuda()


def exact_f32(ref):
    """the fp64 reference as f32, which must hold it exactly"""
    r = ref.float()
    assert torch.equal(r.double(), ref), "the reference is not exact in f32 (the case is not admissible)"
    return r


def expect_of(ref, case, dt):
    r = exact_f32(ref)
    return r.to(dt) if case["out"] == "16" else r  # the exact value rounded once, to nearest even


def out_dtype(case, dt):
    return dt if case["out"] == "16" else torch.float32


def same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape, exp.dtype, exp.shape)
    assert torch.equal(got, exp), f"{what}: {X.first_mismatch(got.double(), exp.double())}"


# ================================================================== a, b: linear_fwd, plain and residual epilogue, f32 and 16-bit output
@pytest.mark.parametrize("fmt", FMTS)
@cases(lambda c: c["entry"] == "fwd" and c["epi"] in ("plain", "res"))
def test_linear_fwd_equals_the_integer_reference(K, case, fmt):
    dt = X.OP16[fmt]
    o = X.operands(case)
    xi, wi = ints(o["x"]), ints(o["w"])
    x, w, bias = op16(xi, dt), op16(wi, dt), f32(o["bias"])
    kw, ref = {}, X.ref_linear(xi.double(), wi.double(), None if bias is None else bias.double())
    if case["epi"] == "res":
        res, gamma, rowscale = f32(o["res"]), o["gamma"].cuda(), o["rowscale"].cuda()
        kw = dict(epilogue=K.EPI_BIAS_RESIDUAL, residual=res, gamma=gamma, rowscale=rowscale, rows_per_scale=case["rows_per_scale"])
        ref, _ = X.ref_residual(xi.double(), wi.double(), bias.double(), res.double(), gamma, rowscale, case["rows_per_scale"])
    exp = expect_of(ref, case, dt)
    del ref
    for name, cfg in case["knobs"]:
        with tuned(K, cfg):
            y, _ = K.linear_fwd(x, w, bias, out_dtype=out_dtype(case, dt), **kw)
        same(y, exp, f"{case['id']} {fmt} {name}")
    if case["epi"] == "res":  # a row group with scale 0 returns the residual
        dropped = (rowscale.repeat_interleave(case["rows_per_scale"])[:case["M"]] == 0)
        assert dropped[0] and torch.equal(y[dropped].float(), res[dropped].to(y.dtype).float())


# ================================================================== c: the GELU epilogue on a real K-long accumulation
def gelu_limit(x64, ref64, fmt):
    """the bound of test_gelu_forward_bias_sweep_every_plan: edge_cases.CPU_F32 times max(1, |x|) plus four f32 ulps of the value"""
    return E.CPU_F32[(fmt, "gelu")] * x64.abs().clamp_min(1.0) + 4 * E.ulp32(ref64)


@pytest.mark.parametrize("fmt", FMTS)
@cases(lambda c: c["epi"] == "gelu")
def test_gelu_epilogue_on_an_exact_accumulator(K, case, fmt):
    """the saved pre-activation is the 16-bit rounding of the exact value, bit for bit; the GELU output per element against
    edge_cases.fast_gelu_cpu of the exact f32 pre-activation on sampled rows, and against fp64 x Phi(x) over the whole tensor"""
    dt = X.OP16[fmt]
    o = X.operands(case)
    s = 2.0 ** -case["scale_log2"]
    xi, wi = ints(o["x"]), ints(o["w"])
    x, w, bias = op16(xi, dt, s), op16(wi, dt), f32(o["bias"], s)
    pre32 = exact_f32(X.ref_linear(xi.double(), wi.double(), ints(o["bias"]).double()) * s)
    pre16 = pre32.to(dt)
    x64 = pre32.double()
    ref64 = E.gelu64(x64)
    lim = gelu_limit(x64, ref64, fmt)
    rows = X.sample_rows(case, 24).cuda()
    cpu = torch.as_tensor(E.fast_gelu_cpu(pre32[rows].cpu().numpy(), fmt)).cuda()
    lim_cpu = gelu_limit(x64[rows], cpu, fmt)
    active = float(((x64.abs() < 4.5) & (x64 != 0)).double().mean())
    for name, cfg in case["knobs"]:
        with tuned(K, cfg):
            y, pre = K.linear_fwd(x, w, bias, out_dtype=torch.float32, epilogue=K.EPI_BIAS_GELU, want_preact=True)
        same(pre, pre16, f"{case['id']} {fmt} {name}: saved pre-activation")
        err, err_cpu = (y.double() - ref64).abs(), (y[rows].double() - cpu).abs()
        print(f"{case['id']} {fmt} {name}: {active:.1%} of the pre-activations inside +-4.5; worst error / bound {float((err / lim).max()):.3f} (fp64), "
              f"{float((err_cpu / lim_cpu).max()):.3f} (fast_gelu_cpu)")
        assert not (err_cpu > lim_cpu).any(), f"{name}: {int((err_cpu > lim_cpu).sum())} sampled elements over the bound against fast_gelu_cpu"
        assert not (err > lim).any(), f"{name}: {int((err > lim).sum())} elements over the bound against fp64"
    if case["family"] == "signed":
        assert active > 0.2, "the pre-activations do not span the polynomial's active range"


# ================================================================== d: linear_bwd_input
@pytest.mark.parametrize("fmt", FMTS)
@cases(lambda c: c["entry"] == "bwd_input" and c["epi"] == "plain")
def test_linear_bwd_input_equals_the_integer_reference(K, case, fmt):
    dt = X.OP16[fmt]
    o = X.operands(case)
    dyi, wTi = ints(o["dy"]), ints(o["wT"])
    dy, wT = op16(dyi, dt), op16(wTi, dt)
    exp = expect_of(X.ref_bwd_input(dyi.double(), wTi.double()), case, dt)
    for name, cfg in case["knobs"]:
        with tuned(K, cfg):
            dx = K.linear_bwd_input(dy, wT, out_dtype=out_dtype(case, dt))
        same(dx, exp, f"{case['id']} {fmt} {name}")


@pytest.mark.parametrize("fmt", FMTS)
@cases(lambda c: c["epi"] == "dgelu")
def test_gelu_backward_epilogue_on_an_exact_accumulator(K, case, fmt):
    """dx = gelu'(h) (dy w) with dy w an exact integer: against fp64 gelu'(h) of the operand-format h times the exact product, per element
    within (the gelu' bound of edge_cases: CPU_F32 + 4 f32 ulps of gelu') |dy w| plus the rounding of the product to f32 (half an ulp) and,
    for a 16-bit output, of that to the format (half an ulp of it)"""
    dt = X.OP16[fmt]
    o = X.operands(case)
    dyi, wTi = ints(o["dy"]), ints(o["wT"])
    dy, wT, h = op16(dyi, dt), op16(wTi, dt), o["h"].to(dt).cuda()
    dx = X.ref_bwd_input(dyi.double(), wTi.double())
    exact_f32(dx)
    g = E.dgelu64(h.double())
    ref = g * dx
    for name, cfg in case["knobs"]:
        with tuned(K, cfg):
            got = K.linear_bwd_input(dy, wT, out_dtype=out_dtype(case, dt), gelu_preact=h).double()
        at = torch.maximum(ref.abs(), got.abs())
        lim = (E.CPU_F32[(fmt, "dgelu")] + 4 * E.ulp32(g)) * dx.abs() + 0.5 * E.ulp32(at)
        if case["out"] == "16":
            lim = lim + 0.5 * X.ulp16(at, fmt)
        err = (got - ref).abs()
        print(f"{case['id']} {fmt} {name}: worst error / bound {float((err / lim.clamp_min(1e-300)).max()):.3f}")
        assert torch.isfinite(got).all() and not (err > lim).any(), f"{name}: {int((err > lim).sum())} elements over the bound"


# ================================================================== e: linear_fwd_qkv
@pytest.mark.parametrize("fmt", FMTS)
@cases(lambda c: c["entry"] == "qkv")
def test_linear_fwd_qkv_equals_the_integer_reference(K, case, fmt):
    """q_prescale = 1/8 moves the binary point: bit for bit.  q_prescale = q_prescale_of(1/8), no power of two: the k and v thirds bit for bit,
    the q third ONE f32 multiply of the exact integer s + b (the product of an exact value is unambiguous: no contraction can change it),
    rounded to the format for a 16-bit output"""
    dt = X.OP16[fmt]
    o = X.operands(case)
    D = case["N"] // 3
    xi, wi = ints(o["x"]), ints(o["w"])
    x, w = op16(xi, dt), op16(wi, dt)
    qb, vb = f32(o["bias"][:D]), f32(o["bias"][2 * D:])
    ref = exact_f32(X.ref_linear(xi.double(), wi.double(), ints(o["bias"]).double()))
    cs = K.q_prescale_of(0.125)
    exps = {}
    for c in (1.0, 0.125, cs):
        e = ref.clone()
        e[:, :D] = e[:, :D] * torch.tensor(c, dtype=torch.float32, device="cuda")  # (python float -> f32, as the C ABI takes it)
        exps[c] = e.to(dt) if case["out"] == "16" else e
    for name, cfg in case["knobs"]:
        for c in (1.0, 0.125, cs):
            with tuned(K, cfg):
                y = K.linear_fwd_qkv(x, w, qb, vb, out_dtype=out_dtype(case, dt), q_prescale=c)
            same(y[:, D:], exps[c][:, D:], f"{case['id']} {fmt} {name} q_prescale {c}: k / v thirds")
            same(y[:, :D], exps[c][:, :D], f"{case['id']} {fmt} {name} q_prescale {c}: q third")


# ================================================================== f: weight gradients
def _weight_inputs(case, dt):
    o = X.operands(case)
    t = {k: ints(v) for k, v in o.items()}
    acc = case["accumulate"]
    dW, db = X.ref_bwd_weight(t["dy"].double(), t["x"].double(), t["dW0"].double() if acc else None, t["db0"].double() if acc else None)
    r = dict(dy=op16(t["dy"], dt), x=op16(t["x"], dt), dW=exact_f32(dW), db=exact_f32(db), acc=acc, dW0=t["dW0"].float(), db0=t["db0"].float())
    if "dy2" in t:
        r.update(dy2=op16(t["dy2"], dt), x2=op16(t["x2"], dt), dW02=t["dW02"].float(),
                 dW2=exact_f32(X.ref_bwd_weight(t["dy2"].double(), t["x2"].double(), t["dW02"].double() if acc else None)[0]))
    return r


def _start(t0, acc):
    """the tensor a weight gradient lands in: the integers to accumulate onto, or a fill that must be overwritten"""
    return t0.clone() if acc else torch.full_like(t0, 7.0)


@pytest.mark.parametrize("fmt", FMTS)
@cases(lambda c: c["entry"] in ("bwd_weight", "bwd_weight_qkv"))
def test_linear_bwd_weight_equals_the_integer_reference(K, case, fmt):
    r = _weight_inputs(case, X.OP16[fmt])
    for name, cfg in case["knobs"]:
        dW, db = _start(r["dW0"], r["acc"]), _start(r["db0"], r["acc"])
        with tuned(K, cfg):
            if case["entry"] == "bwd_weight":
                K.linear_bwd_weight(r["dy"], r["x"], want_bias=True, dW=dW, db=db, accumulate=r["acc"])
                same(db, r["db"], f"{case['id']} {fmt} {name}: db")
            else:
                dq, dv = (t.clone() for t in X.qv_split(db))
                K.linear_bwd_weight_qkv(r["dy"], r["x"], dW, dq, dv, accumulate=r["acc"])
                for got, exp, what in zip((dq, dv), X.qv_split(r["db"]), ("dq_bias", "dv_bias")):
                    same(got, exp, f"{case['id']} {fmt} {name}: {what}")
        same(dW, r["dW"], f"{case['id']} {fmt} {name}: dW")
    if not r["acc"]:  # the entry point that allocates its outputs
        dW, db = K.linear_bwd_weight(r["dy"], r["x"], want_bias=True)
        same(dW, r["dW"], f"{case['id']} {fmt}: dW (fresh)")
        if case["entry"] == "bwd_weight":
            same(db, r["db"], f"{case['id']} {fmt}: db (fresh)")


@pytest.mark.parametrize("fmt", FMTS)
@cases(lambda c: c["entry"] == "bwd_weight_pair")
def test_linear_bwd_weight_pair_equals_the_integer_reference_and_the_single_calls(K, case, fmt):
    """the pair in one launch and as two (another share count, another order over the rows: here that must not matter), and the two single
    calls: all equal the reference, so each other, bit for bit"""
    r = _weight_inputs(case, X.OP16[fmt])
    acc, qkv = r["acc"], case["qkv"]
    for name, cfg in case["knobs"] + [("single_calls", None)]:
        dW1, dW2, db = _start(r["dW0"], acc), _start(r["dW02"], acc), _start(r["db0"], acc)
        dq, dv = (t.clone() for t in X.qv_split(db))
        with tuned(K, cfg or {}):
            if cfg is None:
                if qkv:
                    K.linear_bwd_weight_qkv(r["dy"], r["x"], dW1, dq, dv, accumulate=acc)
                else:
                    K.linear_bwd_weight(r["dy"], r["x"], want_bias=True, dW=dW1, db=db, accumulate=acc)
                K.linear_bwd_weight(r["dy2"], r["x2"], want_bias=False, dW=dW2, accumulate=acc)
            elif qkv:
                K.linear_bwd_weight_pair(r["dy"], r["x"], dW1, dq, dv, r["dy2"], r["x2"], dW2, accumulate=acc)
            else:
                K.linear_bwd_weight_pair(r["dy"], r["x"], dW1, db, None, r["dy2"], r["x2"], dW2, accumulate=acc)
        what = f"{case['id']} {fmt} {name}"
        same(dW1, r["dW"], what + ": dW1")
        same(dW2, r["dW2"], what + ": dW2")
        if qkv:
            for got, exp, nm in zip((dq, dv), X.qv_split(r["db"]), ("dq_bias", "dv_bias")):
                same(got, exp, f"{what}: {nm}")
        else:
            same(db, r["db"], what + ": db1")


# ================================================================== g: gamma / rowscale that are no powers of two
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case", X.NONPOW2_CASES, ids=[c["id"] for c in X.NONPOW2_CASES])
def test_residual_epilogue_bound_on_an_exact_accumulator(K, case, fmt):
    """gamma = 1 + 0.3 z, rowscale 1.25 or 0.  The accumulator s + b is exact, so the epilogue is three roundings at most -- gamma rs, times the
    sum, plus the residual:  |y - ref| <= 1.0625 (2^-23 |gamma rs (s + b)| + 2^-24 |ref|)  with ref in fp64 (1.0625 takes the second-order
    terms; the bound and not the bits, because the compiler may fuse the multiply with the add).  Rows with scale 0: the residual, bit for bit"""
    dt = X.OP16[fmt]
    o = X.operands(case, nonpow2=True)
    xi, wi = ints(o["x"]), ints(o["w"])
    x, w, bias, res, gamma, rowscale = op16(xi, dt), op16(wi, dt), f32(o["bias"]), f32(o["res"]), o["gamma"].cuda(), o["rowscale"].cuda()
    ref, t = X.ref_residual(xi.double(), wi.double(), bias.double(), res.double(), gamma, rowscale, case["rows_per_scale"])
    lim = 1.0625 * (2.0 ** -23 * t.abs() + 2.0 ** -24 * ref.abs())
    dropped = rowscale.repeat_interleave(case["rows_per_scale"])[:case["M"]] == 0
    assert dropped[0] and not dropped.all()
    for name, cfg in case["knobs"]:
        with tuned(K, cfg):
            y, _ = K.linear_fwd(x, w, bias, out_dtype=torch.float32, epilogue=K.EPI_BIAS_RESIDUAL, residual=res, gamma=gamma, rowscale=rowscale,
                                rows_per_scale=case["rows_per_scale"])
        err = (y.double() - ref).abs()
        print(f"{case['id']} {fmt} {name}: worst error / bound {float((err / lim.clamp_min(1e-300)).max()):.3f}")
        assert not (err > lim).any(), f"{name}: {int((err > lim).sum())} elements over the bound, first {X.first_mismatch(torch.where(err > lim, y.double(), ref), ref)}"
        same(y[dropped], res[dropped], f"{case['id']} {fmt} {name}: rows with scale 0")


# ================================================================== h: the patch embedding (the RESMOD epilogue)
@pytest.mark.parametrize("fmt", FMTS)
@cases(lambda c: c["entry"] == "patch_embed")
def test_patch_embedding_equals_the_integer_reference(K, case, fmt):
    """patch_embed_fwd, patch_embed_fwd_implicit, and the uint8 route (im2col_tubelets_u8 with mean 0 and std 1, then the GEMM).  The uint8
    route maps level u to u / 255, an integer only for u = 0 and 255: its clip holds those two levels"""
    dt = X.OP16[fmt]
    P = X.PATCH_EMBED
    ntok = case["res_mod"]
    for binary in (False, True):
        o = X.patch_embed_operands(case, binary=binary)
        clip, w, bias, pos = o["clip"].float().cuda(), op16(ints(o["w"]), dt), f32(o["bias"]), f32(o["pos"])
        levels = o["clip"] // 255 if binary else o["clip"]
        exp = exact_f32(X.ref_patch_embed(levels, o["w"], o["bias"], o["pos"]).double()).cuda()
        cols_ref = X.im2col(levels, P["tubelet"], P["patch"]).reshape(-1, case["K"]).to(dt).cuda()
        if not binary:
            out, cols = K.patch_embed_fwd(clip, w, bias, pos, P["tubelet"], P["patch"])
            same(cols, cols_ref, f"{case['id']} {fmt}: patch matrix")
            same(out, exp, f"{case['id']} {fmt}: patch_embed_fwd")
            out = K.patch_embed_fwd_implicit(clip, w, bias, pos, P["tubelet"], P["patch"])
            assert out is not None, "the implicit kernel must take this case"
            same(out, exp, f"{case['id']} {fmt}: patch_embed_fwd_implicit")
            same(K.patch_embed_gemm(cols, w, bias, None, ntok), exact_f32(exp.double() - pos.double()), f"{case['id']} {fmt}: patch_embed_gemm without pos_embed")
        else:
            frames = o["clip"].permute(0, 2, 3, 4, 1).contiguous().to(torch.uint8).cuda()  # [B, T, H, W, 3]
            cols = K.im2col_tubelets_u8(frames, P["tubelet"], P["patch"], (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), dtype=dt)
            same(cols, cols_ref, f"{case['id']} {fmt}: uint8 patch matrix")
            same(K.patch_embed_gemm(cols, w, bias, pos, ntok), exp, f"{case['id']} {fmt}: uint8 route")


# ================================================================== i: precise mode (split_bf16x3 operands through the same kernels)
def _wide(g, shape):
    return torch.randint(-2047, 2048, shape, generator=g).float()


def test_precise_mode_split_operands_are_exact(K):
    """x = hi + lo in bf16 three times over ([hi | hi | lo] against [hi | lo | hi]: hi hi + hi lo + lo hi).  One operand holds integers up to
    +-2047, which need the lo part; the other -7 ... 7 with lo = 0: the dropped lo lo term is zero and 768 x 2047 x 7 < 2^24, so the forward with
    x wide reaches the lo hi third alone, with w wide the hi lo third alone, and the stacked weight-gradient form both -- all bit for bit"""
    g = torch.Generator().manual_seed(20)
    M, N, Kd = 300, 264, 768
    for wide in ("x", "w"):
        x = _wide(g, (M, Kd)) if wide == "x" else torch.randint(-7, 8, (M, Kd), generator=g).float()
        w = _wide(g, (N, Kd)) if wide == "w" else torch.randint(-7, 8, (N, Kd), generator=g).float()
        big = x if wide == "x" else w
        lo = big - big.to(torch.bfloat16).float()
        assert float((lo != 0).float().mean()) > 0.6
        assert float((x.abs().double() @ w.abs().double().t()).max()) < X.LIMIT
        xs, ws = K.split_bf16x3(x.cuda(), role_b=False), K.split_bf16x3(w.cuda(), role_b=True)
        ref = exact_f32((x.double() @ w.double().t()).cuda())
        for name, cfg in X.SMALL_TILES:
            with tuned(K, cfg):
                y, _ = K.linear_fwd(xs, ws, None, out_dtype=torch.float32)
            same(y, ref, f"precise forward, {wide} wide, {name}")
        # the thirds, separately: without the lo part the result is wrong by exactly the lo term
        hi_only = (x.to(torch.bfloat16).double() @ w.to(torch.bfloat16).double().t()).cuda()
        assert not torch.equal(hi_only, ref.double())
    for wide in ("dy", "x"):
        dy = _wide(g, (M, N)) if wide == "dy" else torch.randint(-7, 8, (M, N), generator=g).float()
        x = _wide(g, (M, Kd)) if wide == "x" else torch.randint(-7, 8, (M, Kd), generator=g).float()
        assert float((dy.abs().double().t() @ x.abs().double()).max()) < X.LIMIT
        ref = exact_f32((dy.double().t() @ x.double()).cuda())
        for name, cfg in X.TN_KERNELS:
            with tuned(K, cfg):
                dW, _ = K.linear_bwd_weight(K.split_bf16x3(dy.cuda(), role_b=False, stack=True), K.split_bf16x3(x.cuda(), role_b=True, stack=True), want_bias=False)
            same(dW, ref, f"precise weight gradient, {wide} wide, {name}")


# ================================================================== j: the integer reductions that ride along
def _dev_ints(lo, hi, shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, device="cuda", dtype=torch.int32)


@pytest.mark.parametrize("M,N", [(1, 4), (255, 16), (1027, 20), (5000, 772), (50176, 3072), (300, 37), (2049, 1)])
def test_colsum_f32_of_integers(K, M, N):
    """the shapes of test_colsum_f32_shapes with levels 0 ... 255: 50 176 x 255 < 2^24"""
    a = _dev_ints(0, 255, (M, N), M + N)
    same(K.colsum_f32(a.float()), exact_f32(a.double().sum(0)), f"colsum_f32 {M} x {N}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M,N", [(1000, 264), (37, 8), (50176, 768)])
def test_colsum_16bit_of_integers(K, M, N, fmt):
    a = _dev_ints(0, 127, (M, N), M + N)
    same(K.colsum_bf16(a.to(X.OP16[fmt])), exact_f32(a.double().sum(0)), f"colsum {fmt} {M} x {N}")


@pytest.mark.parametrize("B,R,N,r0,rc", [(3, 197, 384, 1, 196), (2, 1568, 772, 392, 1176), (5, 50, 36, 0, 50), (16, 1568, 384, 1567, 1)])
def test_colsum_window_f32_of_integers(K, B, R, N, r0, rc):
    a = _dev_ints(-1000, 1000, (B, R, N), B + R + N)
    same(K.colsum_window_f32(a.float(), r0, rc), exact_f32(a[:, r0:r0 + rc].double().sum((0, 1))), f"colsum_window {B} x {R} x {N} [{r0}, {r0 + rc})")


def test_sumsq_and_meanpool_of_integers(K):
    base = _dev_ints(-7, 7, (300011,), 5).float()  # 300 011 x 49 < 2^24
    for off in (0, 1, 2, 3, 5):
        for n in (1, 2, 3, 4, 7, 1023, 4096 * 3 + off, 100003, 300011 - 8):
            v = base[off:off + n]
            out = torch.zeros(1, device="cuda")
            K.sumsq(v, out)
            same(out, exact_f32((v.double() ** 2).sum().reshape(1)), f"sumsq offset {off} n {n}")
    for B, N, D in ((3, 256, 384), (2, 1024, 772), (5, 64, 36)):  # a token count that is a power of two: the mean is exact
        x = _dev_ints(-1000, 1000, (B, N, D), B + N + D)
        same(K.meanpool_fwd(x.float()), exact_f32(x.double().mean(1)), f"meanpool {B} x {N} x {D}")
