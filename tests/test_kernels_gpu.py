"""Per-kernel parity of the HIP path (through the C ABI) against the fp64 oracle evaluated on the
SAME bf16-rounded inputs.  Tolerance (stated by BASELINE.json north_star): 1e-3 relative for
floating point with f32 outputs; bit-exact for index bookkeeping and casts; bf16 outputs are
checked to one bf16 ulp of the tensor scale (2^-8).  Run with `pytest -m gpu` on an MI355X."""
import math

import numpy as np
import pytest
import torch

import golden_recipe as R
from attn_util import prescaled_pair
from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-3
BF16_ULP = 2.0 ** -8
# Inside the fused attention kernels the softmax probabilities P (and dS in backward) are rounded to bf16 before they
# enter the second MFMA (exactly what flash-attn, the reference's own attention backend, does: flash_attention_class.py
# requires fp16/bf16).  That rounding alone is 2^-9 relative per element and does not average out relative to the
# output (measured rel-L2 ~1.5e-3; the max over ~10^5 outputs of a long sequence reaches ~1.7e-3), so the fast kernels are
# held to 2.5e-3 in rel-L2 and 4.5e-3 in the max norm (1.5x what was measured: 1.7e-3 / 3.1e-3; the IEEE-half twins:
# tests/test_half_gpu.py, 6e-4).
ATT_TOL = 2.5e-3
ATT_TOL_MAX = 4.5e-3
ATT_TOL_F16, ATT_TOL_MAX_F16 = 6e-4, 1.2e-3


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import kernels
    from simple_tad_amd import _lib
    _lib.load()
    return kernels


def dev(t):
    return t.cuda().contiguous()


def bf(t):  # round to bf16 and back (exactly representable inputs)
    return t.to(torch.bfloat16).to(torch.float32)


def relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def rell2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def check(a, b, tol=TOL, what="", tol_max=None):
    """tol bounds the rel-L2 error; the max-norm error is held to tol_max (default: the same tol)"""
    e1, e2 = relmax(a, b), rell2(a, b)
    assert e1 <= (tol if tol_max is None else tol_max) and e2 <= tol, f"{what}: max-rel {e1:.3e} l2-rel {e2:.3e} > {tol} (max: {tol_max})"


# ------------------------------------------------------------------ casts (bit-exact RNE)
def test_cast_bit_exact(K):
    x = R.tensor_for("cast.x", (1237, 77), scale=3.0)
    x[0, :4] = torch.tensor([0.0, -0.0, 1e-40, 65504.0])
    y = K.cast_bf16(dev(x))
    assert torch.equal(y.cpu().view(torch.int16), x.to(torch.bfloat16).view(torch.int16))
    w = R.tensor_for("cast.w", (300, 130))
    wt = K.transpose_cast_bf16(dev(w))
    assert torch.equal(wt.cpu().view(torch.int16), w.t().contiguous().to(torch.bfloat16).view(torch.int16))


# ------------------------------------------------------------------ patch index bookkeeping (bit-exact)
def test_im2col_index_bookkeeping_bit_exact(K, golden):
    g = golden("g1_bookkeeping")
    code = torch.arange(2 * 3 * 4 * 32 * 32, dtype=torch.int64).reshape(2, 3, 4, 32, 32)
    rec = torch.zeros(2 * 8, 1536, dtype=torch.int64)
    for digit in range(3):  # base-256 digits are exact in bf16
        x = ((code >> (8 * digit)) & 255).float()
        cols = K.im2col_tubelets(dev(x), 2, 16).cpu().float()
        rec += cols.to(torch.int64) << (8 * digit)
    assert torch.equal(rec.reshape(2, 8, 1536).to(torch.int32), torch.from_numpy(g["patch_codes"]))
    # second geometry against the oracle's im2col
    x = torch.randint(0, 256, (3, 3, 4, 16, 16)).float()
    cols = K.im2col_tubelets(dev(x), 2, 8).cpu().float()
    assert torch.equal(cols.reshape(3, 8, 384), O.im2col_tubelets(x, 2, 8))


# The im2col kernels launch at most 2048 blocks of 256 threads and walk further items in a grid-stride loop: the smallest shape at which each
# instance makes a second trip, whole tensor against the CPU oracle, bit for bit.  (The 8-pixel uint8 kernels: tests/test_frame_store_gpu.py.)
IM2COL_ONE_TRIP = 2048 * 256
_BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}


def _assert_patch_matrix(cols, want, what):
    """cols [B*N, ldk] (device) == want [B, N, K] (oracle, already in cols' dtype) bit for bit, padding columns exactly zero"""
    Kd = want.shape[-1]
    bits = cols.cpu().view(_BITS[cols.dtype])
    assert cols.dtype == want.dtype and bits.shape[0] == want.shape[0] * want.shape[1] and bits.shape[1] >= Kd, what
    assert torch.equal(bits[:, :Kd], want.reshape(-1, Kd).contiguous().view(_BITS[cols.dtype])), what
    assert not bits[:, Kd:].any(), what + ": padding"


@pytest.mark.parametrize("shape,patch,per,dtype", [
    ((3, 3, 8, 256, 256), 16, 8, torch.bfloat16), ((3, 3, 8, 256, 256), 16, 8, torch.float16), ((3, 3, 4, 256, 256), 16, 4, torch.float32),
    ((1, 3, 10, 196, 196), 14, 2, torch.bfloat16), ((1, 3, 10, 196, 196), 14, 2, torch.float16), ((1, 3, 10, 196, 196), 14, 2, torch.float32)],
    ids=["wide-bf16", "wide-f16", "wide-f32", "pairs-bf16", "pairs-f16", "pairs-f32"])
def test_im2col_f32_source_second_grid_stride_trip(K, shape, patch, per, dtype):
    assert math.prod(shape) // per > IM2COL_ONE_TRIP
    x = torch.randn(shape, generator=torch.Generator().manual_seed(11))
    cols = K.im2col_tubelets_f32(dev(x), 2, patch) if dtype == torch.float32 else K.im2col_tubelets(dev(x), 2, patch, dtype=dtype)
    assert (cols.shape[1] > 3 * 2 * patch * patch) == (patch == 14)
    _assert_patch_matrix(cols, O.im2col_tubelets(x.to(dtype), 2, patch), f"{shape} /{patch} {dtype}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("policy", ["ring", "table"])
def test_im2col_u8_pairs_second_grid_stride_trip(K, policy, dtype):
    B, T, HW, mean, std = 7, 4, 196, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    assert B * T * HW * HW // 2 > IM2COL_ONE_TRIP
    frames = torch.randint(0, 256, (B, T, HW, HW, 3), generator=torch.Generator().manual_seed(12), dtype=torch.uint8)
    want = O.im2col_tubelets(O.tensor_normalize(frames, mean, std).permute(0, 4, 1, 2, 3), 2, 14).to(dtype)
    if policy == "ring":  # slot (t + 1) % T of a clip holds its frame t
        cols = K.im2col_tubelets_u8(dev(torch.roll(frames, shifts=1, dims=1)), 2, 14, mean, std, t_offset=1, dtype=dtype)
    else:                 # identity slots over the same frames
        idx = torch.arange(B * T, dtype=torch.int32).reshape(B, T)
        cols = K.im2col_frame_windows(dev(frames.reshape(B * T, HW, HW, 3)), dev(idx), 2, 14, mean, std, dtype=dtype)
    assert cols.shape[1] == 1216
    _assert_patch_matrix(cols, want, f"u8 {policy} {dtype}")


def test_patch_embed_fwd(K):
    x = R.tensor_for("pe.x", (1, 3, 4, 32, 32))
    w = R.tensor_for("pe.w", (64, 3, 2, 16, 16), scale=0.02)
    b = R.tensor_for("pe.b", (64,), scale=0.02)
    pos = O.sinusoid_table(8, 64)[0]
    out, cols = K.patch_embed_fwd(dev(x), dev(w.reshape(64, -1)).to(torch.bfloat16), dev(b), dev(pos), 2, 16)
    ref = O.patch_embed(bf(x).double(), bf(w).double(), b.double(), 2, 16) + pos.double()
    check(out, ref, what="patch_embed_fwd")
    assert torch.equal(cols.cpu().float().reshape(1, 8, 1536), O.im2col_tubelets(bf(x), 2, 16))


@pytest.mark.parametrize("B,T,HW,D,bias,pos", [(1, 4, 32, 64, True, True), (2, 8, 224, 384, True, True), (3, 16, 224, 768, True, False), (5, 2, 48, 200, False, True),
                                               (2, 16, 224, 1024, False, False)])
@pytest.mark.parametrize("fmt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_patch_embed_implicit_gemm_is_bit_identical_to_the_explicit_route(K, B, T, HW, D, bias, pos, fmt):
    """the forward that reads the clip itself (tad_patch_embed_fwd_implicit: no patch matrix) gives the bits of im2col + gemm_nt --
    same rounding of x, same matrix instruction and k order, bias first, position row last -- at ragged row / column tiles (M = 5 * 9 tokens,
    D = 200), the real ViT-S / ViT-B / ViT-L widths, with and without bias / pos_embed, in both operand formats; and it is what a no_grad
    forward of the module runs"""
    g = torch.Generator().manual_seed(B * 1000 + D)
    x = torch.randn(B, 3, T, HW, HW, generator=g)
    w = (torch.randn(D, 3 * 2 * 256, generator=g) * 0.02).to(fmt)
    ntok = (T // 2) * (HW // 16) ** 2
    bv = torch.randn(D, generator=g) if bias else None
    pv = torch.randn(ntok, D, generator=g) if pos else None
    K.set_operand_dtype(fmt)
    try:
        ref, _ = K.patch_embed_fwd(dev(x), dev(w), None if bv is None else dev(bv), None if pv is None else dev(pv), 2, 16)
        got = K.patch_embed_fwd_implicit(dev(x), dev(w), None if bv is None else dev(bv), None if pv is None else dev(pv), 2, 16)
    finally:
        K.set_operand_dtype(torch.bfloat16)
    assert got is not None and got.shape == ref.shape and torch.equal(got, ref)
    # patch sizes the implicit kernel is not written for fall back (None), and the C entry point refuses them
    assert K.patch_embed_fwd_implicit(dev(torch.randn(1, 3, 2, 28, 28)), dev(torch.zeros(8, 1216)).to(torch.bfloat16), None, None, 2, 14) is None


def test_no_grad_forward_takes_the_implicit_patch_embedding():
    import simple_tad_amd as T
    from simple_tad_amd import kernels as KK
    torch.manual_seed(0)
    m = T.VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=1, num_heads=2, all_frames=4, tubelet_size=2, num_classes=2, mlp_ratio=4,
                            qkv_bias=True, init_scale=1.0).cuda()
    x = torch.randn(2, 3, 4, 32, 32).cuda()
    from simple_tad_amd import ops as OPS
    calls = {"implicit": 0, "explicit": 0}
    imp, exp, min_tiles = KK.patch_embed_fwd_implicit, KK.patch_embed_fwd, OPS.IMPLICIT_PATCH_EMBED_MIN_TILES
    OPS.IMPLICIT_PATCH_EMBED_MIN_TILES = 0  # (this tiny model is far below the size from which the implicit route is the faster one)
    KK.patch_embed_fwd_implicit = lambda *a, **k: (calls.__setitem__("implicit", calls["implicit"] + 1), imp(*a, **k))[1]
    KK.patch_embed_fwd = lambda *a, **k: (calls.__setitem__("explicit", calls["explicit"] + 1), exp(*a, **k))[1]
    try:
        m.eval()
        with torch.no_grad():
            y0 = m(x)
        assert calls == {"implicit": 1, "explicit": 0}
        m.train()
        y1 = m(x)
        y1.sum().backward()
        assert calls == {"implicit": 1, "explicit": 1} and m.patch_embed.proj.weight.grad is not None
    finally:
        KK.patch_embed_fwd_implicit, KK.patch_embed_fwd = imp, exp
        OPS.IMPLICIT_PATCH_EMBED_MIN_TILES = min_tiles
    torch.testing.assert_close(y0, y1.detach(), rtol=1e-6, atol=1e-6)  # (the patch embedding's bits are equal: test above; no dropout / drop-path in this model)


# ------------------------------------------------------------------ layernorm
@pytest.mark.parametrize("rows,D", [(150, 128), (37, 384), (1030, 768), (5, 1024), (9, 1280), (9, 1792), (3, 1540)])
def test_layernorm_fwd_bwd(K, rows, D):
    x = R.tensor_for(f"ln.x{D}", (rows, D), scale=2.0, shift=0.5)
    w = R.tensor_for(f"ln.w{D}", (D,), scale=0.1, shift=1.0)
    b = R.tensor_for(f"ln.b{D}", (D,), scale=0.1)
    xd = x.double().requires_grad_()
    wd, bd = w.double().requires_grad_(), b.double().requires_grad_()
    ref = O.layer_norm(xd, wd, bd, 1e-6)
    y32, mean, rstd = K.layernorm_fwd(dev(x), dev(w), dev(b), 1e-6, out_dtype=torch.float32)
    check(y32, ref, what="ln fwd f32")
    check(mean, x.double().mean(-1), what="ln mean")
    y16, _, _ = K.layernorm_fwd(dev(x), dev(w), dev(b), 1e-6, out_dtype=torch.bfloat16)
    check(y16.float(), ref, tol=BF16_ULP, what="ln fwd bf16")
    # backward (dy given in bf16 -> oracle sees the same rounded values), with residual-grad add, bf16 copy, colsum
    dy = bf(R.tensor_for(f"ln.dy{D}", (rows, D)))
    dres = R.tensor_for(f"ln.dres{D}", (rows, D))
    ref.backward(dy.double())
    dx, dxb, dg, db, cs = K.layernorm_bwd(dev(dy).to(torch.bfloat16), dev(x), dev(w), mean, rstd, dres=dev(dres), want_bf16=True,
                                          want_colsum=True)
    ref_dx = xd.grad + dres.double()
    check(dx, ref_dx, what="ln dx")
    check(dxb.float(), ref_dx, tol=BF16_ULP, what="ln dx bf16")
    check(dg, wd.grad, what="ln dgamma")
    check(db, bd.grad, what="ln dbeta")
    check(cs, ref_dx.sum(0), what="ln colsum")
    # f32 dy, no residual
    dx2, _, dg2, _, _ = K.layernorm_bwd(dev(dy), dev(x), dev(w), mean, rstd)
    check(dx2, xd.grad, what="ln dx (f32 dy)")
    check(dg2, wd.grad, what="ln dgamma (f32 dy)")


# ------------------------------------------------------------------ linear
LIN_SHAPES = [(300, 384, 128), (2500, 768, 256), (16, 128, 1536), (2304, 100, 64), (3000, 1152, 384), (4100, 2304, 768), (1568, 768, 3072)]


@pytest.mark.parametrize("M,N,Kd", LIN_SHAPES)
def test_linear_fwd_epilogues(K, M, N, Kd):
    x = bf(R.tensor_for(f"lin.x{M}", (M, Kd)))
    w = bf(R.tensor_for(f"lin.w{N}", (N, Kd), scale=0.05))
    b = R.tensor_for(f"lin.b{N}", (N,), scale=0.1)
    xd, wd = dev(x).to(torch.bfloat16), dev(w).to(torch.bfloat16)
    ref = x.double() @ w.double().t() + b.double()
    y, _ = K.linear_fwd(xd, wd, dev(b), out_dtype=torch.float32)
    check(y, ref, what="linear bias f32")
    y16, _ = K.linear_fwd(xd, wd, dev(b), out_dtype=torch.bfloat16)
    check(y16.float(), ref, tol=BF16_ULP, what="linear bias bf16")
    y0, _ = K.linear_fwd(xd, wd, None, out_dtype=torch.float32)
    check(y0, x.double() @ w.double().t(), what="linear nobias")
    # GELU + saved pre-activation
    yg, pre = K.linear_fwd(xd, wd, dev(b), out_dtype=torch.float32, epilogue=1, want_preact=True)
    check(yg, O.gelu_erf(ref), what="linear gelu")
    check(pre.float(), ref, tol=BF16_ULP, what="linear preact")
    # residual + layer-scale + per-sample drop-path scale
    res = R.tensor_for(f"lin.r{M}", (M, N))
    gam = R.tensor_for(f"lin.g{N}", (N,), scale=0.3, shift=1.0)
    rows_per = 7
    rs = torch.tensor([0.0 if i % 3 == 0 else 1.25 for i in range((M + rows_per - 1) // rows_per)])
    yr, _ = K.linear_fwd(xd, wd, dev(b), out_dtype=torch.float32, epilogue=2, residual=dev(res), gamma=dev(gam), rowscale=dev(rs),
                         rows_per_scale=rows_per)
    ref_r = res.double() + rs.double().repeat_interleave(rows_per)[:M, None] * gam.double() * ref
    check(yr, ref_r, what="linear residual")
    yr2, _ = K.linear_fwd(xd, wd, dev(b), out_dtype=torch.float32, epilogue=2, residual=dev(res))
    check(yr2, res.double() + ref, what="linear residual plain")
    # groups at least as long as a tile (clips of 1568 tokens in the model): the epilogue takes one or two scales per tile instead of
    # one load per row; group boundaries fall inside tiles, a zero scale (dropped sample) must give exactly the residual
    for rows_per in (130, 300, 1568):
        ng = (M + rows_per - 1) // rows_per
        rs = torch.tensor([0.0 if i % 3 == 1 else 1.0 + 0.25 * i for i in range(ng)])
        yr3, _ = K.linear_fwd(xd, wd, dev(b), out_dtype=torch.float32, epilogue=2, residual=dev(res), gamma=dev(gam), rowscale=dev(rs),
                              rows_per_scale=rows_per)
        ref3 = res.double() + rs.double().repeat_interleave(rows_per)[:M, None] * gam.double() * ref
        check(yr3, ref3, what=f"linear residual, groups of {rows_per}")
        dropped = (rs.repeat_interleave(rows_per)[:M] == 0)
        if dropped.any():
            assert torch.equal(yr3.cpu()[dropped], res[dropped]), "a dropped sample must pass the residual through unchanged"


@pytest.mark.parametrize("M,N,Kd", [(300, 384, 128), (2500, 768, 3072), (1570, 3072, 768), (100, 64, 128)])
def test_linear_bwd(K, M, N, Kd):
    """y = x W^T: dx = dy W (optionally through GELU'), dW = dy^T x, db = colsum(dy)"""
    dy = bf(R.tensor_for(f"lb.dy{M}", (M, N)))
    w = bf(R.tensor_for(f"lb.w{N}", (N, Kd), scale=0.05))
    x = bf(R.tensor_for(f"lb.x{M}", (M, Kd)))
    wT = K.transpose_cast_bf16(dev(w))
    dyd = dev(dy).to(torch.bfloat16)
    ref_dx = dy.double() @ w.double()
    dx = K.linear_bwd_input(dyd, wT, out_dtype=torch.float32)
    check(dx, ref_dx, what="linear dx")
    h = bf(R.tensor_for(f"lb.h{M}", (M, Kd), scale=1.5))
    hd = h.double().requires_grad_()
    O.gelu_erf(hd).backward(ref_dx)
    dxg = K.linear_bwd_input(dyd, wT, out_dtype=torch.float32, gelu_preact=dev(h).to(torch.bfloat16))
    check(dxg, hd.grad, what="linear dx through gelu")
    dW, db = K.linear_bwd_weight(dyd, dev(x).to(torch.bfloat16))
    check(dW, dy.double().t() @ x.double(), what="linear dW")
    check(db, dy.double().sum(0), what="linear db")
    # accumulate into existing grads
    dW0 = R.tensor_for("lb.dw0", (N, Kd))
    dWa, _ = K.linear_bwd_weight(dyd, dev(x).to(torch.bfloat16), want_bias=False, dW=dev(dW0), accumulate=True)
    check(dWa, dW0.double() + dy.double().t() @ x.double(), what="linear dW accumulate")


# ------------------------------------------------------------------ attention
ATT_SHAPES = [(2, 100, 2), (1, 1568, 2), (3, 64, 1), (2, 8, 3), (1, 784, 6), (1, 129, 1), (4, 600, 12)]


def _attn_ref(qkv, B, N, H, scale, dout=None):
    q = qkv.double().reshape(B, N, -1).requires_grad_()
    y = O.attention_core(q, H, scale)
    if dout is None:
        return y, None
    y.backward(dout.double().reshape(B, N, -1))
    return y, q.grad


@pytest.mark.parametrize("prescaled", [True, False], ids=["q_prescaled", "plain_q"])
@pytest.mark.parametrize("B,N,H", ATT_SHAPES)
def test_attention_fwd_bwd(K, B, N, H, prescaled):
    """prescaled: the production contract (the qkv Linear writes q * scale * log2e); plain: flash-attn's contract (the kernels apply the
    factor to the f32 scores)"""
    scale = 64 ** -0.5
    qkv = bf(R.tensor_for(f"att.qkv{N}", (B * N, 3 * H * 64), scale=1.0))
    dout = bf(R.tensor_for(f"att.do{N}", (B * N, H * 64)))
    opnd = qkv
    if prescaled:
        opnd, qkv = prescaled_pair(qkv, B, N, H, scale, bf)
    ref, ref_dqkv = _attn_ref(qkv, B, N, H, scale, dout)
    qd = dev(opnd).to(torch.bfloat16)
    kw = {"q_prescaled": prescaled}
    out32, lse = K.attn_fwd(qd, B, N, H, scale, out_dtype=torch.float32, **kw)
    check(out32.reshape(B, N, -1), ref, tol=ATT_TOL, tol_max=ATT_TOL_MAX, what="attn fwd f32")
    # lse = log sum exp(scale q.k)
    q4 = qkv.double().reshape(B, N, 3, H, 64)
    s = torch.einsum("bnhd,bmhd->bhnm", q4[:, :, 0], q4[:, :, 1]) * scale
    # (the kernel's row sum is taken of the bf16-rounded P the second product uses: 2^-9 per term, averaging out with the key count)
    assert (lse.cpu().double() - torch.logsumexp(s, -1)).abs().max().item() < (1e-3 if N >= 64 else 2e-3)
    out16, _ = K.attn_fwd(qd, B, N, H, scale, out_dtype=torch.bfloat16, **kw)
    check(out16.float().reshape(B, N, -1), ref, tol=BF16_ULP, what="attn fwd bf16")
    # out_lo (both outputs leave through the same per-wave LDS patch, back to back): bit-exactly what the rounding of out dropped
    o16, _, lo = K.attn_fwd(qd, B, N, H, scale, want_lo=True, **kw)
    assert torch.equal(o16, out16) and torch.equal(lo.float(), (out32 - out16.float()).to(torch.bfloat16).float())
    dqkv = K.attn_bwd(qd, out16, dev(dout).to(torch.bfloat16), lse, B, N, H, scale, **kw)
    g = dqkv.float().cpu().reshape(B, N, 3, H, 64)
    r = ref_dqkv.reshape(B, N, 3, H, 64)
    for i, nm in enumerate("qkv"):
        # bf16 outputs; P/dS operands are bf16-rounded inside the kernel -> 2 ulp of the tensor scale
        check(g[:, :, i], r[:, :, i], tol=2 * BF16_ULP, what=f"attn d{nm}")


@pytest.mark.parametrize("B,N,H", [(2, 100, 2), (1, 1568, 2), (3, 64, 1), (2, 8, 3), (1, 129, 1), (4, 600, 12), (1, 200, 1)])
def test_attention_fwd_q64_variant_is_bit_identical(K, B, N, H):
    """the opt-in forward with 64 query rows per wave (tad_attn_tuning("fwd_q64", 1): two 32-row halves share every K / V fragment read) does
    the same arithmetic in the same order per row: out, out_lo and lse are bit-identical to the production kernel's, ragged blocks, a
    rescale-forcing spike and whole dead halves included"""
    scale = 64 ** -0.5
    qkv = bf(R.tensor_for(f"att.qkv{N}", (B * N, 3 * H * 64), scale=1.0))
    if N == 200:  # late maxima (cdna_hip_programming.md rule 26): a key in tile 2 far above everything before it
        q4 = qkv.reshape(B, N, 3, H, 64).clone()
        q4[0, 150, 1, 0] = q4[0, 17, 0, 0] * 6.0
        q4[0, 64, 1, 0] = q4[0, 70, 0, 0] * 5.0
        qkv = bf(q4.reshape(B * N, -1))
    opnd, _ = prescaled_pair(qkv, B, N, H, scale, bf)
    qd = dev(opnd).to(torch.bfloat16)
    from simple_tad_amd._lib import ATTN_FWD, ATTN_FWD_Q64
    plan = lambda lo: K.attn_plan(B, N, H, q_prescaled=True, out_lo=lo)[0]  # noqa: E731
    assert (plan(True)["kernel"], plan(True)["skip"]) == (ATTN_FWD, 0)
    ref = K.attn_fwd(qd, B, N, H, scale, want_lo=True, q_prescaled=True)
    found = K.attn_tuning_get("fwd_q64")
    K.attn_tuning(fwd_q64=1)
    try:
        assert [(plan(lo)["kernel"], plan(lo)["has_lo"], plan(lo)["block"]) for lo in (True, False)] == [(ATTN_FWD_Q64, 1, 128), (ATTN_FWD_Q64, 0, 128)]
        got = K.attn_fwd(qd, B, N, H, scale, want_lo=True, q_prescaled=True)
        got_nolo = K.attn_fwd(qd, B, N, H, scale, q_prescaled=True)
    finally:
        K.attn_tuning(fwd_q64=found)
    for a, b, nm in zip(ref, got, ("out", "lse", "out_lo")):
        assert torch.equal(a, b), nm
    assert torch.equal(got_nolo[0], ref[0]) and torch.equal(got_nolo[1], ref[1])


@pytest.mark.parametrize("prescaled", [True, False], ids=["q_prescaled", "plain_q"])
def test_attention_softmax_spike(K, prescaled):
    """Force every branch of the online softmax's offset handling (cdna_hip_programming.md rule 26: a rare data-dependent branch needs an
    input that takes it).  attn_fwd.hip keeps one running maximum per row, started at -1e30, so the first tile always sets it; in a later
    tile it moves -- for all 32 rows of the wave, each to its own maximum so far, with the accumulators and the row sum rescaled -- only
    when some row of the wave has a tile maximum more than RESCALE_THR = 8 log2 units above its running one, and P may reach 2^8
    meanwhile.  One v_sub per score takes the running maximum off; there is no other offset:
      query 17: late-arriving maxima in tiles 0 and 2 (the move in tile 2 rescales the whole wave);  query 64: one move in tile 2;
      query 40: every score far below 0 (q anti-parallel to all keys' common component): the first tile sets a maximum near -96;
      query 41: far below 0 in tile 0, a key in tile 1 with a positive score far above that (negative) maximum."""
    B, N, H = 1, 200, 1
    scale = 64 ** -0.5
    qkv = bf(R.tensor_for("att.spike", (B * N, 3 * H * 64), scale=1.0))
    q4 = qkv.reshape(B, N, 3, H, 64)
    q4[0, 5, 1, 0] = q4[0, 17, 0, 0] * 6.0    # key 5 aligns with query 17
    q4[0, 190, 1, 0] = q4[0, 17, 0, 0] * 12.0  # later key with an even larger score
    q4[0, 130, 1, 0] = q4[0, 64, 0, 0] * 10.0
    q4[0, :, 1, 0] += 3.0 * torch.ones(64)     # a common component in every key ...
    q4[0, 40, 0, 0] = -4.0 * torch.ones(64)    # ... against which query 40 scores ~ -96 * 1.44 everywhere
    q4[0, 41, 0, 0] = -4.0 * torch.ones(64)
    q4[0, 100, 1, 0] = -2.0 * torch.ones(64)   # ... except query 41 on key 100 (tile 1): +64
    qkv = bf(q4.reshape(B * N, -1))
    opnd = qkv
    if prescaled:
        opnd, qkv = prescaled_pair(qkv, B, N, H, scale, bf)
    ref, _ = _attn_ref(qkv, B, N, H, scale)
    out32, lse = K.attn_fwd(dev(opnd).to(torch.bfloat16), B, N, H, scale, out_dtype=torch.float32, q_prescaled=prescaled)
    assert torch.isfinite(out32).all() and torch.isfinite(lse).all()
    check(out32.reshape(B, N, -1), ref, tol=4e-3, what="attn spike")  # P is bf16 inside the kernel: ulp-level error on O(1) weights
    q4d = qkv.double().reshape(B, N, 3, H, 64)
    s = torch.einsum("bnhd,bmhd->bhnm", q4d[:, :, 0], q4d[:, :, 1]) * scale
    assert (lse.cpu().double() - torch.logsumexp(s, -1)).abs().max().item() < 5e-3  # (|lse| reaches ~100 here)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("prescaled", [True, False], ids=["q_prescaled", "plain_q"])
@pytest.mark.parametrize("B,N,H,p", [(2, 100, 2, 0.0), (1, 1568, 2, 0.0), (2, 8, 3, 0.0), (1, 129, 1, 0.0), (1, 393, 3, 0.0), (2, 200, 2, 0.25),
                                     (2, 129, 2, 0.0), (2, 129, 2, 0.25)])
def test_attention_head_dim_80_fwd_bwd(K, B, N, H, p, prescaled, fmt):
    """head_dim 80 (vit_huge: embed_dim 1280 / 16 heads, modeling_finetune.py:390-398) in the 16-bit MFMA attention kernels (round 4:
    dims 0..63 in the head_dim-64 LDS images, dims 64..79 in 32-byte-row side images, a fifth k-step and a third d tile): forward,
    lse and backward against the oracle, ragged N, both operand formats and q contracts, with and without attention dropout (the
    oracle regenerates the keep mask).  Tolerances are those of the head_dim-64 tests.  Every launch is first asserted (kernels.attn_plan) to be the
    general record of the selector it is meant to be: together the cases visit each head_dim-80 record of the launchers' kernel tables
    (output type x q contract x dropout, forward and backward, both formats), those at B=2, N=129, H=2 with one row in the second query
    block, a clip boundary inside the grid and a head stride -- test_attention_every_general_kernel_of_the_selector does the same for head_dim 64."""
    from simple_tad_amd._lib import ATTN_BWD_DKV, ATTN_BWD_DQ, ATTN_FWD
    d, seed = 80, 424242
    scale = d ** -0.5
    dt = torch.bfloat16 if fmt == "bf16" else torch.float16
    rnd = lambda t: t.to(dt).float()  # noqa: E731
    qkv = rnd(R.tensor_for(f"att80.qkv{N}", (B * N, 3 * H * d), scale=1.0))
    dout = rnd(R.tensor_for(f"att80.do{N}", (B * N, H * d)))
    opnd = qkv
    if prescaled:
        opnd, qkv = prescaled_pair(qkv, B, N, H, scale, rnd, d=d)
    qd = qkv.double().reshape(B, N, -1).requires_grad_()
    ref = O.attention_core(qd, H, scale, drop_p=p, seed=seed) if p else O.attention_core(qd, H, scale)
    ref.backward(dout.double().reshape(B, N, -1))
    kw = dict(q_prescaled=prescaled, drop_p=p, seed=seed, d=d)
    planned = dict(q_prescaled=prescaled, drop_p=p, d=d)
    record = dict(hd=d, qs=int(prescaled), drop=int(p > 0), dma_mode=0, skip=0, has_lo=0, grid=-(-N // 128) * H * B, block=256)
    x = dev(opnd).to(dt)
    assert K.attn_plan(B, N, H, out_16bit=False, **planned) == [dict(kernel=ATTN_FWD, out16=0, **record)]
    out32, lse = K.attn_fwd(x, B, N, H, scale, out_dtype=torch.float32, **kw)
    assert out32.shape == (B * N, H * d)
    tol, tol_max = (ATT_TOL, ATT_TOL_MAX) if fmt == "bf16" else (ATT_TOL_F16, ATT_TOL_MAX_F16)
    check(out32.reshape(B, N, -1), ref.detach(), tol=tol, tol_max=tol_max, what="attn80 fwd f32")
    q4 = qkv.double().reshape(B, N, 3, H, d)
    sc = torch.einsum("bnhd,bmhd->bhnm", q4[:, :, 0], q4[:, :, 1]) * scale
    assert (lse.cpu().double() - torch.logsumexp(sc, -1)).abs().max().item() < (1e-3 if N >= 64 else 2e-3)
    assert K.attn_plan(B, N, H, out_16bit=True, out_lo=True, **planned) == [dict(kernel=ATTN_FWD, out16=1, **record)]
    out16, lse, lo = K.attn_fwd(x, B, N, H, scale, want_lo=True, **kw)
    ulp = BF16_ULP if fmt == "bf16" else 2 * tol
    check(out16.float().reshape(B, N, -1), ref.detach(), tol=ulp, what="attn80 fwd 16-bit")
    # out_lo is exactly what the rounding dropped (bit-exact against the f32 output of the same kernel family)
    assert torch.equal(lo.float(), (out32 - out16.float()).to(dt).float())
    assert K.attn_plan(B, N, H, backward=True, out_lo=True, **planned) == [dict(kernel=k, out16=1, **record) for k in (ATTN_BWD_DQ, ATTN_BWD_DKV)]
    dqkv = K.attn_bwd(x, out16, dev(dout).to(dt), lse, B, N, H, scale, out_lo=lo, **kw)
    g, r = dqkv.float().cpu().reshape(B, N, 3, H, d), qd.grad.reshape(B, N, 3, H, d)
    for i, nm in enumerate("qkv"):
        check(g[:, :, i], r[:, :, i], tol=2 * ulp, what=f"attn80 d{nm}")
    # without out_lo (delta from the rounded output) the gradients stay inside the same band
    dqkv2 = K.attn_bwd(x, out16, dev(dout).to(dt), lse, B, N, H, scale, **kw)
    for i, nm in enumerate("qkv"):
        check(dqkv2.float().cpu().reshape(B, N, 3, H, d)[:, :, i], r[:, :, i], tol=3 * ulp, what=f"attn80 d{nm} (rounded-output delta)")


# ------------------------------------------------------------------ helpers
def test_meanpool_colsum_scale_sumsq(K):
    x = R.tensor_for("mp.x", (3, 197, 384))
    y = K.meanpool_fwd(dev(x))
    check(y, x.double().mean(1), tol=1e-5, what="meanpool fwd")
    dy = R.tensor_for("mp.dy", (3, 384))
    dx, dxb = K.meanpool_bwd(dev(dy), 197, want_bf16=True)
    ref = (dy.double() / 197)[:, None, :].expand(3, 197, 384)
    check(dx, ref, tol=1e-6, what="meanpool bwd")
    check(dxb.float(), ref, tol=BF16_ULP, what="meanpool bwd bf16")
    a = bf(R.tensor_for("cs.a", (1000, 264)))
    check(K.colsum_bf16(dev(a).to(torch.bfloat16)), a.double().sum(0), tol=1e-5, what="colsum")
    xs = R.tensor_for("sc.x", (60, 128))
    gam = R.tensor_for("sc.g", (128,), shift=1.0, scale=0.1)
    rs = torch.tensor([0.0, 1.25, 1.25, 0.0, 1.25, 1.25])
    sc = K.scale_cast_bf16(dev(xs), dev(gam), dev(rs), 10)
    check(sc.float(), xs.double() * gam.double() * rs.double().repeat_interleave(10)[:, None], tol=BF16_ULP, what="scale_cast")
    out = torch.zeros(1, device="cuda")
    v = R.tensor_for("ss.x", (100003,))
    K.sumsq(dev(v), out)
    assert abs(out.item() - (v.double() ** 2).sum().item()) < 1e-4 * (v.double() ** 2).sum().item()


def test_sumsq_alignment_tails_and_grad_norm_coef(K):
    """the vectorised sum of squares for every alignment of the first element and every tail length, its determinism, and
    tad_grad_norm_coef (GradScaler.unscale_ + clip_grad_norm_ + the found-inf decision of utils.py:386-412 on the device) against
    the same arithmetic in torch"""
    from simple_tad_amd import _lib
    base = dev(R.tensor_for("ss2.x", (70001,)))
    for off in (0, 1, 2, 3, 5):
        for n in (1, 2, 3, 4, 7, 1023, 4096 * 3 + off, 70001 - 8):
            v = base[off:off + n]
            out = torch.zeros(1, device="cuda")
            K.sumsq(v, out)
            ref = (v.double() ** 2).sum().item()
            assert abs(out.item() - ref) <= 2e-6 * ref, (off, n, out.item(), ref)
    big = dev(R.tensor_for("ss2.big", (3_000_017,)))
    a, b = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    K.sumsq(big, a)
    K.sumsq(big, b)
    assert torch.equal(a, b), "fixed-order reduction: two runs must agree bit for bit"
    g = dev(R.tensor_for("gnc.g", (123457,), scale=300.0))
    nrm = g.double().norm().item()
    for inv, mx in ((1.0 / 1024.0, 0.0), (1.0 / 1024.0, 5.0), (1.0, 1e9), (0.5, 1e-3)):
        o = K.grad_norm_coef(g, inv, mx).cpu()
        n_ref = nrm * inv
        c_ref = inv * (min(mx / (n_ref + 1e-6), 1.0) if mx > 0 else 1.0)
        assert abs(o[0].item() - n_ref) <= 2e-6 * n_ref and abs(o[1].item() - c_ref) <= 4e-6 * c_ref and o[2].item() == 0.0, (inv, mx, o)
    for poison in (float("inf"), float("nan"), 3e38):  # (3e38 squared overflows f32: the norm is inf, as torch's)
        h = g.clone()
        h[777] = poison
        o = K.grad_norm_coef(h, 1.0 / 65536.0, 1.0).cpu()
        assert not math.isfinite(o[0].item()) and o[1].item() == 0.0 and o[2].item() == 1.0, (poison, o)
    with pytest.raises(_lib.TadError):
        K.grad_norm_coef(torch.zeros(8), 1.0)


def test_patch_embed_bwd_entry_point_is_the_weight_gradient_gemm(K):
    """include/tad_mi355x.h declares tad_patch_embed_bwd (the Conv3d weight gradient, modeling_finetune.py:169-205 backward) beside the
    Linear entry points; the product reaches the same kernels through ops.linear_dw.  Called through the C ABI here: dW, db against
    the oracle on the bf16-rounded operands, and bit for bit what tad_linear_bwd_weight returns (exported, bound, never called)"""
    from simple_tad_amd import _lib
    lib = _lib.load()
    M, D, Kc = 2 * 392, 128, 1536
    dy = bf(R.tensor_for("peb.dy", (M, D), scale=0.1))
    cols = bf(R.tensor_for("peb.cols", (M, Kc)))
    dyd, cd = dev(dy).to(torch.bfloat16), dev(cols).to(torch.bfloat16)
    st = torch.cuda.current_stream().cuda_stream
    nb = lib.tad_patch_embed_bwd_workspace_bytes(M, D, Kc)
    assert nb == lib.tad_linear_bwd_weight_workspace_bytes(M, D, Kc) and nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dW, db = torch.full((D, Kc), 7.0, device="cuda"), torch.full((D,), 7.0, device="cuda")  # (overwritten, not accumulated)
    assert lib.tad_patch_embed_bwd(dyd.data_ptr(), cd.data_ptr(), dW.data_ptr(), db.data_ptr(), ws.data_ptr(), nb, M, D, Kc, st) == 0, lib.tad_last_error_string()
    check(dW, dy.double().t() @ cols.double(), what="patch_embed_bwd dW")
    check(db, dy.double().sum(0), what="patch_embed_bwd db")
    dW2, db2 = torch.empty(D, Kc, device="cuda"), torch.empty(D, device="cuda")
    assert lib.tad_linear_bwd_weight(dyd.data_ptr(), cd.data_ptr(), dW2.data_ptr(), db2.data_ptr(), 0, ws.data_ptr(), nb, M, D, Kc, st) == 0
    assert torch.equal(dW, dW2) and torch.equal(db, db2)
    rc = lib.tad_patch_embed_bwd(dyd.data_ptr(), cd.data_ptr(), dW.data_ptr(), db.data_ptr(), ws.data_ptr(), 16, M, D, Kc, st)
    assert rc != 0 and b"workspace" in lib.tad_last_error_string()


def test_errors_are_loud(K):
    from simple_tad_amd._lib import TadError
    with pytest.raises(TadError):
        K.cast_bf16(torch.zeros(8))  # CPU tensor: no fallback
    with pytest.raises(TadError, match="K=64 vs w K=128"):
        K.linear_fwd(torch.zeros(4, 64, dtype=torch.bfloat16, device="cuda"), torch.zeros(8, 128, dtype=torch.bfloat16, device="cuda"))
    from simple_tad_amd import _lib
    a, b, y = (torch.zeros(n, dtype=torch.bfloat16, device="cuda") for n in (4 * 60, 8 * 60, 4 * 8))
    rc = _lib.load().tad_linear_fwd(a.data_ptr(), b.data_ptr(), None, y.data_ptr(), 1, 0, None, None, None, None, 1, None, 0, 4, 8, 60, None)
    assert rc != 0 and b"multiple of 64" in _lib.load().tad_last_error_string()  # the C ABI itself keeps the K-tile contract; the wrapper pads (next test)
    with pytest.raises(TadError):
        K.attn_fwd(torch.zeros(4, 3 * 64, dtype=torch.bfloat16, device="cuda"), 1, 5, 1, 0.125)  # wrong element count


def test_linear_reduction_off_the_k_tile_is_zero_padded(K):
    """K=60 / K=1176 (MAE decoder head of a /14 model): the wrappers pad the reduction to the 64-deep K-tile, results unchanged"""
    for Kd in (60, 1176):
        x = R.tensor_for(f"padk.x{Kd}", (70, Kd)).to(torch.bfloat16)
        w = R.tensor_for(f"padk.w{Kd}", (136, Kd), scale=0.05).to(torch.bfloat16)
        y, _ = K.linear_fwd(dev(x), dev(w), None, out_dtype=torch.float32)
        check(y, x.double() @ w.double().t(), tol=2e-5, what=f"linear K={Kd}")
        dy = R.tensor_for(f"padk.dy{Kd}", (70, Kd)).to(torch.bfloat16)      # input gradient reduces over the layer's OUTPUT width
        wT = R.tensor_for(f"padk.wT{Kd}", (128, Kd), scale=0.05).to(torch.bfloat16)
        dx = K.linear_bwd_input(dev(dy), dev(wT), out_dtype=torch.float32)
        check(dx, dy.double() @ wT.double().t(), tol=2e-5, what=f"linear dX N={Kd}")


@pytest.mark.parametrize("M,N", [(1, 4), (255, 16), (1027, 20), (5000, 772), (50176, 3072), (300, 37), (2049, 1)])
def test_colsum_f32_shapes(K, M, N):
    """column sums of an f32 matrix (bias gradients of the precise mode): wide kernel for N % 4 == 0, narrow one otherwise; f64 accumulation"""
    g = torch.Generator().manual_seed(M + N)
    a = torch.randn(M, N, generator=g) + 0.25
    got = K.colsum_f32(dev(a))
    check(got, a.double().sum(0), tol=2e-6, what=f"colsum f32 {M}x{N}")
    assert torch.equal(got, K.colsum_f32(dev(a)))  # fixed summation order


# ------------------------------------------------------------------ precise-mode kernels (parity gate): 1e-3 is met with margin
def test_split_bf16x3_linear_matches_f32_product(K):
    M, N, Kd = 300, 256, 128
    x = R.tensor_for("sp.x", (M, Kd))
    w = R.tensor_for("sp.w", (N, Kd), scale=0.05)
    xs, ws = K.split_bf16x3(dev(x), role_b=False), K.split_bf16x3(dev(w), role_b=True)
    assert xs.shape == (M, 3 * Kd) and ws.shape == (N, 3 * Kd)
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    assert torch.equal(xs.cpu().view(torch.int16), torch.cat([hi, hi, lo], 1).view(torch.int16))           # bit-exact split
    y, _ = K.linear_fwd(xs, ws, None, out_dtype=torch.float32)
    check(y, x.double() @ w.double().t(), tol=2e-5, what="split-bf16 linear")                                  # f32-level product
    # stacked form for the weight gradient: dW = dy^T x
    dy = R.tensor_for("sp.dy", (M, N))
    dW, _ = K.linear_bwd_weight(K.split_bf16x3(dev(dy), role_b=False, stack=True), K.split_bf16x3(dev(x), role_b=True, stack=True),
                                want_bias=False)
    check(dW, dy.double().t() @ x.double(), tol=2e-5, what="split-bf16 dW")
    check(K.colsum_f32(dev(dy)), dy.double().sum(0), tol=1e-6, what="colsum f32")
    h = R.tensor_for("sp.h", (M, N), scale=1.5)
    hd = h.double().requires_grad_()
    a = O.gelu_erf(hd)
    a.backward(dy.double())
    check(K.gelu_f32(dev(h)), a.detach(), tol=1e-6, what="gelu f32")
    check(K.gelu_bwd_f32(dev(dy), dev(h)), hd.grad, tol=1e-6, what="gelu bwd f32")


@pytest.mark.parametrize("B,N,H,d", [(2, 100, 2, 64), (1, 1568, 1, 64), (2, 8, 3, 64), (2, 100, 2, 80), (1, 393, 3, 80)])
def test_attention_f32_fwd_bwd(K, B, N, H, d):
    """f32 attention kernels: head_dim 64 (precise mode) and 80 (the "huge" configurations, no MFMA kernel)"""
    scale = d ** -0.5
    qkv = R.tensor_for(f"attf.qkv{N}.{d}", (B * N, 3 * H * d))
    dout = R.tensor_for(f"attf.do{N}.{d}", (B * N, H * d))
    ref, ref_dqkv = _attn_ref(qkv, B, N, H, scale, dout)
    out, lse = K.attn_fwd_f32(dev(qkv), B, N, H, scale, want_lse=True, d=d)
    check(out.reshape(B, N, -1), ref, tol=1e-5, what="attn f32 fwd")
    dqkv = K.attn_bwd_f32(dev(qkv), out, dev(dout), lse, B, N, H, scale, d=d)
    check(dqkv.reshape(B, N, -1), ref_dqkv, tol=1e-5, what="attn f32 bwd")


# ---- persistent (one workgroup per CU walks a tile list) vs one-workgroup-per-tile scheduling of the Linear GEMMs.
# Neither scheduling (incl. running a Linear as two launches over row ranges) nor the epilogue's store path (straight from the MFMA layout / transposed through the LDS) may change a
# single bit: same tiles, same K order, same epilogue arithmetic.  Shapes are large enough
# for the persistent path (>= 2 tiles per CU) and include ragged M / N edges.
@pytest.mark.parametrize("M,N,Kd,mode", [
    (12544 + 77, 3072, 768, "gelu"), (25088 + 130, 768, 768, "res"), (25088, 768, 3072, "res"), (25088 + 5, 2304, 768, "plain"),
    (12544 + 200, 3072, 768, "dgelu"), (25088, 768 + 4, 128, "plain_f32"),
    # the peeled last K-tile of the persistent bias-only bf16 kernel: odd number of K-tiles (falls back), two K-tiles, N off the 8-column store width
    (25088 + 5, 2300, 192, "plain"), (20000 + 3, 1028, 128, "plain"), (30000, 1024, 3072, "plain")])
def test_linear_persistent_schedule_is_bit_identical(K, M, N, Kd, mode):
    from simple_tad_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(M + N)
    x = dev(torch.randn(M, Kd, generator=g)).to(torch.bfloat16)
    w = dev(torch.randn(N, Kd, generator=g) * 0.05).to(torch.bfloat16)
    bias = dev(torch.randn(N, generator=g))
    res = dev(torch.randn(M, N, generator=g)) if mode == "res" else None
    h = dev(torch.randn(M, N, generator=g)).to(torch.bfloat16) if mode == "dgelu" else None

    def run():
        if mode == "gelu":
            return K.linear_fwd(x, w, bias, epilogue=K.EPI_BIAS_GELU, want_preact=True)
        if mode == "res":
            return K.linear_fwd(x, w, bias, out_dtype=torch.float32, epilogue=K.EPI_BIAS_RESIDUAL, residual=res)
        if mode == "dgelu":
            return (K.linear_bwd_input(x, w, gelu_preact=h), None)
        if mode == "plain_f32":
            return K.linear_fwd(x, w, bias, out_dtype=torch.float32)
        return K.linear_fwd(x, w, bias)

    outs = {}
    try:
        # (the split-K tail changes the summation order: its own test; short_k would send the K < 512 cases to 128 x 128 tiles under every configuration)
        base = dict(persistent=0, direct_epilogue=0, split_tail=0, splitk_tail=0, short_k=0)
        for name, cfg in [("tile", {}), ("tile_direct", dict(direct_epilogue=2)), ("persist", dict(persistent=1)),
                          ("persist_direct", dict(persistent=1, direct_epilogue=2)), ("split", dict(persistent=1, split_tail=2)),
                          ("default", {**K.LINEAR_TUNING_DEFAULTS, "splitk_tail": 0}),
                          # the four-wave kernels (csrc/gemm_w4.hip: 128 x 128 outputs per wave, hand-ordered K loop), per tile and persistent
                          ("w4_tile", dict(variant=7)), ("w4_persist", dict(variant=7, persistent=1)),
                          # 192 x 128 tiles (the tail launch of the split plan, tad_linear_tuning("tail_192")), with and without the register-layout stores
                          ("t192", dict(variant=8)), ("t192_direct", dict(variant=8, direct_epilogue=2)),
                          # the short-K plan (K < 512: 128 x 128 tiles, two workgroups per CU) and those tiles for any K
                          ("short_k", dict(short_k=1)), ("t128", dict(variant=2)), ("t192_4w", dict(variant=9)), ("t192_4w_direct", dict(variant=9, direct_epilogue=2))]:
            K.linear_tuning(**{**base, **cfg})
            y, pre = run()
            torch.cuda.synchronize()
            outs[name] = (y.clone(), None if pre is None else pre.clone())
    finally:
        K.linear_tuning(**K.LINEAR_TUNING_DEFAULTS)
    y0, p0 = outs["tile"]
    for name in ("tile_direct", "persist", "persist_direct", "split", "default", "w4_tile", "w4_persist", "t192", "t192_direct", "short_k", "t128", "t192_4w", "t192_4w_direct"):
        y1, p1 = outs[name]
        assert torch.equal(y0, y1), f"{name}: output differs from per-tile scheduling"
        if p0 is not None:
            assert torch.equal(p0, p1), f"{name}: pre-activation differs"
    # and the result is right: sampled rows against an f64 product of the same bf16 operands
    rows = torch.randint(0, M, (64,), generator=g).tolist() + [0, M - 1]
    ref = x[rows].double() @ w.double().t()
    if mode == "dgelu":
        hh = h[rows].double()
        ref = ref * (0.5 * (1 + torch.erf(hh / math.sqrt(2))) + hh * torch.exp(-hh * hh / 2) / math.sqrt(2 * math.pi))
    else:
        ref = ref + bias.double()
        if mode == "gelu":
            ref = torch.nn.functional.gelu(ref)
        if mode == "res":
            ref = ref + res[rows].double()
    got = y0[rows].double()
    tol = TOL if y0.dtype == torch.float32 else 2 * BF16_ULP
    assert float((got - ref).abs().max() / ref.abs().max()) < tol


@pytest.mark.parametrize("M,N,Kd", [(50176, 768, 768), (25088 + 70, 2304, 768), (12544, 768 + 8, 3072 - 8), (1024, 512, 256), (40000, 384, 1536)])
def test_weight_gradient_four_wave_kernel_is_bit_identical(K, M, N, Kd):
    """gemm_tn_w4_kernel (csrc/gemm_w4.hip: four waves of 128 x 128, one per SIMD, the default for 256-wide tiles) against the eight-wave
    gemm_tn_kernel: dW and the bias column sums bit for bit (same instruction, same order over the reduction rows), ragged N / K / M edges,
    the qkv entry point with its split bias, accumulate mode; and dW right against an f64 product of the same operands."""
    g = torch.Generator().manual_seed(M + N + Kd)
    dy = dev(torch.randn(M, N, generator=g)).to(torch.bfloat16)
    x = dev(torch.randn(M, Kd, generator=g)).to(torch.bfloat16)
    outs = {}
    try:
        for v in (0, 1):
            K.linear_tuning(**{**K.LINEAR_TUNING_DEFAULTS, "tn_w4": v})
            dW, db = K.linear_bwd_weight(dy, x, want_bias=True)
            acc = torch.full((N, Kd), 0.5, device="cuda")
            dba = torch.full((N,), 0.25, device="cuda")
            K.linear_bwd_weight(dy, x, want_bias=True, dW=acc, db=dba, accumulate=True)
            extra = None
            if N % 3 == 0:
                dWq, dq, dv = torch.zeros(N, Kd, device="cuda"), torch.zeros(N // 3, device="cuda"), torch.zeros(N // 3, device="cuda")
                K.linear_bwd_weight_qkv(dy, x, dWq, dq, dv, accumulate=False)
                extra = (dWq.clone(), dq.clone(), dv.clone())
            torch.cuda.synchronize()
            outs[v] = (dW.clone(), db.clone(), acc.clone(), dba.clone(), extra)
    finally:
        K.linear_tuning(**K.LINEAR_TUNING_DEFAULTS)
    for a_, b_ in zip(outs[0][:4], outs[1][:4]):
        assert torch.equal(a_, b_)
    if outs[0][4] is not None:
        assert all(torch.equal(a_, b_) for a_, b_ in zip(outs[0][4], outs[1][4]))
    rows = torch.randint(0, N, (16,), generator=g).tolist() + [0, N - 1]
    ref = dy[:, rows].double().t() @ x.double()
    check(outs[1][0][rows], ref, what="dW (four-wave kernel)")
    check(outs[1][1], dy.double().sum(0), what="db (four-wave kernel)")


@pytest.mark.parametrize("M,N1,N2,Kd,qkv", [(50176, 2304, 768, 768, True), (25088 + 70, 768, 768 + 8, 768, False), (12544, 3072, 1024, 1024, True),
                                            (20000, 1152, 384, 384, True), (30000, 2304 + 24, 768, 768, True), (1024, 512, 256, 256, False)])
def test_weight_gradient_pair_launch(K, M, N1, N2, Kd, qkv):
    """tad_linear_bwd_weight_pair: the qkv and proj weight gradients of a Block as ONE launch of the four-wave kernel (output rows >= N1 take the
    second problem's operands) against the two single calls -- the same products summed over the rows in another order (a different share
    count), so equal to f32 summation accuracy, not bit for bit; bit for bit where the pair falls back to two launches (K on 128-wide tiles,
    N1 not a multiple of 256, tn_pair = 0), deterministic, accumulate mode, split (qkv) and plain bias sums, right against f64."""
    g = torch.Generator().manual_seed(M + N1 + N2)
    dy1 = dev(torch.randn(M, N1, generator=g)).to(torch.bfloat16)
    x1 = dev(torch.randn(M, Kd, generator=g)).to(torch.bfloat16)
    dy2 = dev(torch.randn(M, N2, generator=g)).to(torch.bfloat16)
    x2 = dev(torch.randn(M, Kd, generator=g)).to(torch.bfloat16)

    def single(acc):
        dW1 = torch.full((N1, Kd), 0.5 if acc else 0.0, device="cuda")
        dW2 = torch.full((N2, Kd), 0.25 if acc else 0.0, device="cuda")
        if qkv:
            dq, dv = torch.full((N1 // 3,), 1.0 if acc else 0.0, device="cuda"), torch.full((N1 // 3,), 2.0 if acc else 0.0, device="cuda")
            K.linear_bwd_weight_qkv(dy1, x1, dW1, dq, dv, accumulate=acc)
            b = (dq, dv)
        else:
            db = torch.full((N1,), 1.0 if acc else 0.0, device="cuda")
            K.linear_bwd_weight(dy1, x1, want_bias=True, dW=dW1, db=db, accumulate=acc)
            b = (db,)
        K.linear_bwd_weight(dy2, x2, want_bias=False, dW=dW2, accumulate=acc)
        return (dW1, dW2) + b

    def pair(acc):
        dW1 = torch.full((N1, Kd), 0.5 if acc else 0.0, device="cuda")
        dW2 = torch.full((N2, Kd), 0.25 if acc else 0.0, device="cuda")
        if qkv:
            dq, dv = torch.full((N1 // 3,), 1.0 if acc else 0.0, device="cuda"), torch.full((N1 // 3,), 2.0 if acc else 0.0, device="cuda")
            K.linear_bwd_weight_pair(dy1, x1, dW1, dq, dv, dy2, x2, dW2, accumulate=acc)
            b = (dq, dv)
        else:
            db = torch.full((N1,), 1.0 if acc else 0.0, device="cuda")
            K.linear_bwd_weight_pair(dy1, x1, dW1, db, None, dy2, x2, dW2, accumulate=acc)
            b = (db,)
        return (dW1, dW2) + b

    # one launch when N1 is a multiple of 256 and K runs on the 256-wide tiles (tn_variant: unless those would pad K by a third or more)
    one_launch = N1 % 256 == 0 and -(-Kd // 256) * 256 * 3 < -(-Kd // 128) * 128 * 4
    for acc in (False, True):
        s_, p_ = single(acc), pair(acc)
        p2 = pair(acc)
        torch.cuda.synchronize()
        for a_, b_, c_ in zip(s_, p_, p2):
            assert torch.equal(b_, c_), "pair launch is not deterministic"
            if one_launch:
                scale = float(a_.abs().max())
                assert float((a_ - b_).abs().max()) <= 2e-5 * scale + 1e-4, f"pair vs single calls: {float((a_ - b_).abs().max()):.3e} of {scale:.3e}"
            else:
                assert torch.equal(a_, b_), "fallback of the pair differs from the single calls"
    try:
        K.linear_tuning(tn_pair=0)
        for a_, b_ in zip(single(True), pair(True)):
            assert torch.equal(a_, b_), "tn_pair = 0 differs from the single calls"
    finally:
        K.linear_tuning(**K.LINEAR_TUNING_DEFAULTS)
    dW1, dW2 = pair(False)[:2]
    rows = torch.randint(0, min(N1, N2), (12,), generator=g).tolist() + [0, min(N1, N2) - 1]
    check(dW1[rows], dy1[:, rows].double().t() @ x1.double(), what="dW1 (pair)")
    check(dW2[rows], dy2[:, rows].double().t() @ x2.double(), what="dW2 (pair)")
    check(dW1[[N1 - 1]], dy1[:, [N1 - 1]].double().t() @ x1.double(), what="dW1 last row (pair)")
    check(dW2[[N2 - 1]], dy2[:, [N2 - 1]].double().t() @ x2.double(), what="dW2 last row (pair)")


@pytest.mark.parametrize("M,D,Kd", [(25088 + 5, 768, 768), (20000 + 3, 384, 384), (300, 128, 128), (40000, 1024, 256)])
def test_qkv_linear_q_prescale_every_schedule(K, M, D, Kd):
    """tad_linear_fwd_qkv(q_prescale): `q = q * self.scale` (modeling_finetune.py:96) folded into the qkv Linear -- the q third of the
    output is multiplied by the factor before its ONE rounding, k and v thirds and the (q_bias, 0, v_bias) bias are those of the plain
    Linear; identical bits from every scheduling path (per-tile / persistent, LDS / register epilogue, peeled last K-tile); D = 384 puts
    the q | k boundary inside a 256-column tile."""
    g = torch.Generator().manual_seed(M + D)
    x = dev(torch.randn(M, Kd, generator=g)).to(torch.bfloat16)
    w = dev(torch.randn(3 * D, Kd, generator=g) * 0.05).to(torch.bfloat16)
    qb, vb = dev(torch.randn(D, generator=g)), dev(torch.randn(D, generator=g))
    c = K.q_prescale_of(64 ** -0.5)
    outs = {}
    try:
        base = dict(persistent=0, direct_epilogue=0, split_tail=0)
        for name, cfg in [("tile", {}), ("tile_direct", dict(direct_epilogue=2)), ("persist", dict(persistent=1)),
                          ("persist_direct", dict(persistent=1, direct_epilogue=2)), ("default", K.LINEAR_TUNING_DEFAULTS)]:
            K.linear_tuning(**{**base, **cfg})
            outs[name] = (K.linear_fwd_qkv(x, w, qb, vb, q_prescale=c).clone(), K.linear_fwd_qkv(x, w, qb, vb, out_dtype=torch.float32, q_prescale=c).clone())
        plain = K.linear_fwd_qkv(x, w, qb, vb)
    finally:
        K.linear_tuning(**K.LINEAR_TUNING_DEFAULTS)
    y0, y0f = outs["tile"]
    for name in ("tile_direct", "persist", "persist_direct", "default"):
        assert torch.equal(y0, outs[name][0]) and torch.equal(y0f, outs[name][1]), f"{name}: differs from per-tile scheduling"
    assert torch.equal(y0[:, D:], plain[:, D:]), "k / v thirds must be the plain Linear's"
    rows = torch.randint(0, M, (64,), generator=g).tolist() + [0, M - 1]
    ref = x[rows].double() @ w.double().t()
    ref[:, :D] = (ref[:, :D] + qb.double()) * c
    ref[:, 2 * D:] += vb.double()
    assert float((y0f[rows].double() - ref).abs().max() / ref.abs().max()) < TOL
    assert float((y0[rows].double() - ref).abs().max() / ref.abs().max()) < 2 * BF16_ULP


@pytest.mark.parametrize("defer", [1, 0], ids=["deferred_combine", "combine_in_launch"])
@pytest.mark.parametrize("M,N,Kd,mode", [(50176, 768, 3072, "plain"), (50176 - 37, 768, 2304, "plain_f32"), (50176, 768, 3072, "res"),
                                         (50176, 768, 768, "res"), (50176, 1024, 1024, "plain"), (25088 + 5, 768, 1024, "res")])
def test_linear_splitk_tail_matches_the_single_launch_plans(K, M, N, Kd, mode, defer):
    """The under-filled last round of tiles as a split-K launch (tad_linear_fwd's `ws`; csrc/gemm.hip SPLITK): every tile of the tail
    is computed by several workgroups over shares of the K-tiles, their f32 partial tiles are combined inside the launch (arrival
    counter, agent-scope release / acquire).  Against the plan without it the result differs only in the summation order over K
    (tolerance-identical: the f32 accumulators of the shares are added in f32); rows of the main launch are bit-identical; the wait
    never gave up (error word 0); twice in a row gives identical bits (the combine order is fixed: share 0, 1, 2 ...).
    defer = 1 (the default plan): the partial tiles are left by a launch in front of the whole-round launch and combined by a third
    launch behind it -- same arithmetic, same order, so both forms must agree to the bit."""
    g = torch.Generator().manual_seed(M + N + Kd)
    x = dev(torch.randn(M, Kd, generator=g)).to(torch.bfloat16)
    w = dev(torch.randn(N, Kd, generator=g) * 0.05).to(torch.bfloat16)
    bias = dev(torch.randn(N, generator=g))
    res = dev(torch.randn(M, N, generator=g)) if mode == "res" else None
    gamma = dev(torch.rand(N, generator=g) + 0.5) if mode == "res" else None
    rows_per_scale = 1568
    rowscale = dev(torch.rand((M + rows_per_scale - 1) // rows_per_scale, generator=g) + 0.5) if mode == "res" else None

    def run():
        if mode == "res":
            return K.linear_fwd(x, w, bias, out_dtype=torch.float32, epilogue=K.EPI_BIAS_RESIDUAL, residual=res, gamma=gamma, rowscale=rowscale,
                                rows_per_scale=rows_per_scale)[0]
        if mode == "plain_f32":
            return K.linear_fwd(x, w, bias, out_dtype=torch.float32)[0]
        return K.linear_fwd(x, w, bias)[0]

    try:
        K.linear_tuning(**{**K.LINEAR_TUNING_DEFAULTS, "splitk_tail": 0})
        y0 = run().clone()
        K.linear_tuning(**{**K.LINEAR_TUNING_DEFAULTS, "splitk_tail": 2, "split_tail": 2, "splitk_defer": defer})
        launches = K.linear_kernel_launches()
        y1 = run().clone()
        assert K.linear_kernel_launches() - launches == (3 if defer else 2)  # (partial tiles of the tail +) main rounds + the split-K tail
        y2 = run().clone()
        K.linear_tuning(**{**K.LINEAR_TUNING_DEFAULTS, "splitk_tail": 2, "split_tail": 2, "splitk_defer": 1 - defer})
        assert torch.equal(run(), y1)  # the other form of the combine: bit-identical
    finally:
        K.linear_tuning(**K.LINEAR_TUNING_DEFAULTS)
    torch.cuda.synchronize()
    ws = K.linear_workspace(0, x.device)
    assert int(ws[4032:4036].view(torch.int32).item()) == 0, "a split-K wait gave up"
    assert torch.equal(y1, y2)
    # which rows the tail covers: everything behind the whole rounds of 256 x 256 tiles
    tiles_n, tiles_m, cus = (N + 255) // 256, (M + 255) // 256, K.device_info()["cu_count"] & ~7
    main_rows = (tiles_m * tiles_n // cus) * cus // tiles_n * 256
    assert 0 < main_rows < M
    assert torch.equal(y0[:main_rows], y1[:main_rows])
    a, b = y0[main_rows:].double(), y1[main_rows:].double()
    tol = 2e-5 if y0.dtype == torch.float32 else 2 * BF16_ULP  # (bf16 outputs: an f32 difference in the last bits can flip a rounding)
    assert float((a - b).abs().max() / a.abs().max()) < tol
    rows = torch.randint(main_rows, M, (48,), generator=g).tolist() + [main_rows, M - 1]
    ref = x[rows].double() @ w.double().t() + bias.double()
    if mode == "res":
        sc = rowscale[torch.tensor(rows, device=x.device) // rows_per_scale].double()[:, None]
        ref = ref * gamma.double() * sc + res[rows].double()
    assert float((y1[rows].double() - ref).abs().max() / ref.abs().max()) < (TOL if y1.dtype == torch.float32 else 2 * BF16_ULP)


@pytest.mark.parametrize("mode", ["plain", "res"], ids=["plain_bf16", "residual_f32"])
def test_linear_executor_runs_the_plan(K, mode):
    """The launcher executes what kernels.linear_plan (csrc/gemm_plan.hip) says, at the smallest shape at which the split plan exists (32 whole row
    panels + a ragged tail): under the defaults and the four plans of test_guarded_gpu.py the launch counter grows by exactly the number of steps
    of the plan.  Outputs: bit-identical between all plans in every row that no split-K step covers, and between the two forms of the split-K
    combine everywhere; the rows of a split-K tail differ from the unsplit plans only in the summation order over K (the tolerance of
    test_linear_splitk_tail_matches_the_single_launch_plans)."""
    from test_guarded_gpu import PLANS
    M, N, Kd = 33 * 256 + 37, 2048, 512
    g = torch.Generator().manual_seed(M + N)
    x = dev(torch.randn(M, Kd, generator=g)).to(torch.bfloat16)
    w = dev(torch.randn(N, Kd, generator=g) * 0.05).to(torch.bfloat16)
    b = dev(torch.randn(N, generator=g) * 0.1)
    res = dev(torch.randn(M, N, generator=g)) if mode == "res" else None
    from simple_tad_amd import _lib
    outs, split_rows = {}, {}
    try:
        for name, knobs in {"defaults": {}, **PLANS}.items():
            K.linear_tuning(**{**K.LINEAR_TUNING_DEFAULTS, **knobs})
            plan = K.linear_plan(M, N, Kd, epilogue=2 if mode == "res" else 0, out_16bit=mode != "res", residual=mode == "res",
                                 ws_bytes=_lib.load().tad_linear_workspace_bytes(M, N, Kd))
            n0 = K.linear_kernel_launches()
            y = (K.linear_fwd(x, w, b, out_dtype=torch.float32, epilogue=K.EPI_BIAS_RESIDUAL, residual=res) if mode == "res" else K.linear_fwd(x, w, b))[0]
            assert K.linear_kernel_launches() - n0 == len(plan), (name, plan)
            ranges = sorted({(s["r0"], s["rows"]) for s in plan})
            assert ranges[0][0] == 0 and sum(r for _, r in ranges) == M, plan  # the steps cover every row once
            outs[name] = y.clone()
            sk = {(s["r0"], s["rows"]) for s in plan if s["kernel"] == 10}
            assert len(sk) == (1 if name.startswith("splitk") else 0), (name, plan)
            split_rows[name] = next(iter(sk)) if sk else (M, 0)
    finally:
        K.linear_tuning(**K.LINEAR_TUNING_DEFAULTS)
    y0 = outs["defaults"]
    ref = x.double() @ w.double().t() + b.double() + (res.double() if mode == "res" else 0.0)
    check(y0.float(), ref, tol=TOL if mode == "res" else BF16_ULP, what=f"linear defaults {mode}")
    assert torch.equal(outs["splitk_deferred"], outs["splitk_in_launch"]), "the two forms of the split-K combine differ"
    for name, y in outs.items():
        r0, rows = split_rows[name]
        assert torch.equal(y[:r0], y0[:r0]) and torch.equal(y[r0 + rows:], y0[r0 + rows:]), f"{name}: rows outside a split-K step differ from the default plan"
        if rows:
            a, c = y0[r0:r0 + rows].double(), y[r0:r0 + rows].double()
            assert float((a - c).abs().max() / a.abs().max()) < (2e-5 if y0.dtype == torch.float32 else 2 * BF16_ULP), name


@pytest.mark.parametrize("tn_pair", [0, 1])
def test_linear_bwd_weight_runs_the_plan(K, tn_pair):
    """the weight gradient alone and as a pair (one launch with tn_pair = 1, two with 0: linear_bwd_weight_plan says which) against the float64 product"""
    M, N, Kd, N2 = 33 * 256 + 37, 512, 256, 256
    g = torch.Generator().manual_seed(M + N + tn_pair)
    dy, x = bf(torch.randn(M, N, generator=g)), bf(torch.randn(M, Kd, generator=g))
    dy2, x2 = bf(torch.randn(M, N2, generator=g)), bf(torch.randn(M, Kd, generator=g))
    d16 = lambda t: dev(t).to(torch.bfloat16)
    from simple_tad_amd import _lib
    need = max(_lib.load().tad_linear_bwd_weight_workspace_bytes(M, n, Kd) for n in (N, N2, N + N2))
    try:
        K.linear_tuning(**{**K.LINEAR_TUNING_DEFAULTS, "tn_pair": tn_pair})
        single, pair = K.linear_bwd_weight_plan(M, N, Kd), K.linear_bwd_weight_plan(M, N, Kd, N2=N2, ws_bytes=need)
        assert len(single) == 1 and single[0]["pair"] == 0 and single[0]["N"] == N and single[0]["grid"] == single[0]["tiles"] * single[0]["splits"]
        assert [(r["N"], r["pair"]) for r in pair] == ([(N + N2, 1)] if tn_pair else [(N, 0), (N2, 0)]), pair
        dW, db = K.linear_bwd_weight(d16(dy), d16(x))
        dW1, dW2, db1 = (torch.empty(N, Kd, device="cuda"), torch.empty(N2, Kd, device="cuda"), torch.empty(N, device="cuda"))
        K.linear_bwd_weight_pair(d16(dy), d16(x), dW1, db1, None, d16(dy2), d16(x2), dW2, False)
    finally:
        K.linear_tuning(**K.LINEAR_TUNING_DEFAULTS)
    check(dW, dy.double().t() @ x.double(), what="linear dW")
    check(db, dy.double().sum(0), what="linear db")
    check(dW1, dy.double().t() @ x.double(), what="pair dW1")
    check(db1, dy.double().sum(0), what="pair db1")
    check(dW2, dy2.double().t() @ x2.double(), what="pair dW2")


def test_linear_taller_than_the_32bit_epilogue_offsets(K):
    """VERDICT r01 robustness: an f32 output beyond 2 GiB (here 180 000 x 3072 x 4 B = 2.2 GB, ViT-B fc1 at B = 115) used to be refused;
    rows are independent, so the launcher runs row ranges that fit the 32-bit epilogue offsets.  Bit-identical to the same rows
    computed as a small problem of their own (same tile plan per row is not guaranteed, same arithmetic per output element is)."""
    M, N, Kd = 180000, 3072, 64
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, Kd, generator=g).bfloat16().cuda()
    w = (torch.randn(N, Kd, generator=g) * 0.1).bfloat16().cuda()
    b = torch.randn(N, generator=g).cuda()
    y, _ = K.linear_fwd(x, w, b, out_dtype=torch.float32)
    for r0 in (0, 174000, 174100, M - 300):
        ys, _ = K.linear_fwd(x[r0:r0 + 300].contiguous(), w, b, out_dtype=torch.float32)
        assert torch.equal(y[r0:r0 + 300], ys), r0
    ref = x[-300:].double() @ w.double().t() + b.double()
    check(y[-300:], ref, what="tall linear")
    # bf16 output of the same shape stays ONE launch range (1.1 GB < 2 GiB with 2-byte elements): exercised for the cap arithmetic
    yb, _ = K.linear_fwd(x, w, b, out_dtype=torch.bfloat16)
    assert torch.equal(yb[-300:].float(), K.linear_fwd(x[-300:].contiguous(), w, b, out_dtype=torch.bfloat16)[0].float())


# ------------------------------------------------------------------ attention dropout (modeling_finetune.py:99-101; flash_attention_class.py:59-61)
@pytest.mark.parametrize("d,H", [(64, 2), (80, 2)])
def test_attention_dropout_f32_vs_oracle_with_the_injected_mask(K, d, H):
    """attn_drop inside attention: the kernels' counter-based keep mask, regenerated by the oracle (attention_dropout_keep) and injected
    into the reference formula softmax(q k^T) -> dropout -> @ v, forward and backward; ragged N; and the mask's statistics."""
    B, N, p, seed = 2, 200, 0.25, 1234567
    scale = d ** -0.5
    qkv = R.tensor_for(f"attdrop.qkv{d}", (B, N, 3 * H * d), scale=1.0)
    dout = R.tensor_for(f"attdrop.do{d}", (B, N, H * d))
    qd = qkv.double().requires_grad_()
    ref = O.attention_core(qd, H, scale, drop_p=p, seed=seed)
    ref.backward(dout.double())
    out, lse = K.attn_fwd_f32(dev(qkv.reshape(B * N, -1)), B, N, H, scale, want_lse=True, d=d, drop_p=p, seed=seed)
    check(out.reshape(B, N, -1), ref, tol=1e-5, what="attn dropout fwd")
    dqkv = K.attn_bwd_f32(dev(qkv.reshape(B * N, -1)), out, dev(dout.reshape(B * N, -1)), lse, B, N, H, scale, d=d, drop_p=p, seed=seed)
    check(dqkv.reshape(B, N, -1), qd.grad, tol=2e-5, what="attn dropout bwd")
    # p = 0 is the plain kernel; another seed is another mask
    out0, _ = K.attn_fwd_f32(dev(qkv.reshape(B * N, -1)), B, N, H, scale, want_lse=True, d=d)
    check(out0.reshape(B, N, -1), O.attention_core(qkv.double(), H, scale), tol=1e-5, what="attn p=0")
    out2, _ = K.attn_fwd_f32(dev(qkv.reshape(B * N, -1)), B, N, H, scale, want_lse=True, d=d, drop_p=p, seed=seed + 1)
    assert not torch.equal(out, out2)
    keep = O.attention_dropout_keep(4, 3, 512, p, seed).float()
    assert abs(keep.mean().item() - (1 - p)) < 2e-3 and abs(keep.mean(-1).std().item() - (p * (1 - p) / 512) ** 0.5) < 3e-3


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("prescaled", [True, False], ids=["q_prescaled", "plain_q"])
def test_attention_dropout_16bit_kernels_vs_oracle_with_the_injected_mask(K, fmt, prescaled):
    """attn_drop inside the 16-bit MFMA attention kernels (round 4; before, attn_drop > 0 fell to the exact-f32 kernels at 1/16 of the
    matrix rate): same counter-based keep mask as the f32 family, regenerated by the oracle and injected into the reference formula
    softmax(q k^T) -> dropout -> @ v (modeling_finetune.py:96-103), forward and backward, ragged N spanning several tiles, both
    operand formats, both q contracts; lse is that of the FULL softmax; p = 0 and another seed behave."""
    B, N, H, p, seed = 2, 200, 2, 0.25, 7654321
    scale = 64 ** -0.5
    dt = torch.bfloat16 if fmt == "bf16" else torch.float16
    rnd = lambda t: t.to(dt).float()  # noqa: E731
    qkv = rnd(R.tensor_for("attdrop16.qkv", (B * N, 3 * H * 64), scale=1.0))
    dout = rnd(R.tensor_for("attdrop16.do", (B * N, H * 64)))
    opnd = qkv
    if prescaled:
        opnd, qkv = prescaled_pair(qkv, B, N, H, scale, rnd)
    qd = qkv.double().reshape(B, N, -1).requires_grad_()
    ref = O.attention_core(qd, H, scale, drop_p=p, seed=seed)
    ref.backward(dout.double().reshape(B, N, -1))
    kw = dict(q_prescaled=prescaled, drop_p=p, seed=seed)
    x = dev(opnd).to(dt)
    out32, lse = K.attn_fwd(x, B, N, H, scale, out_dtype=torch.float32, **kw)
    tol, tol_max = (ATT_TOL, ATT_TOL_MAX) if fmt == "bf16" else (ATT_TOL_F16, ATT_TOL_MAX_F16)
    check(out32.reshape(B, N, -1), ref, tol=tol, tol_max=tol_max, what="attn dropout fwd")
    q4 = qkv.double().reshape(B, N, 3, H, 64)
    sc = torch.einsum("bnhd,bmhd->bhnm", q4[:, :, 0], q4[:, :, 1]) * scale
    assert (lse.cpu().double() - torch.logsumexp(sc, -1)).abs().max().item() < 1e-3  # (the full softmax's, whatever was dropped)
    out16, lse, lo = K.attn_fwd(x, B, N, H, scale, want_lo=True, **kw)
    dqkv = K.attn_bwd(x, out16, dev(dout).to(dt), lse, B, N, H, scale, out_lo=lo, **kw)
    g, r = dqkv.float().cpu().reshape(B, N, 3, H, 64), qd.grad.reshape(B, N, 3, H, 64)
    for i, nm in enumerate("qkv"):
        check(g[:, :, i], r[:, :, i], tol=2 * (BF16_ULP if fmt == "bf16" else 2 * tol), what=f"attn dropout d{nm}")
    # the mask is applied: the result differs from the undropped one, another seed is another mask, p = 0 is the plain kernel
    out0, _ = K.attn_fwd(x, B, N, H, scale, out_dtype=torch.float32, q_prescaled=prescaled)
    out2, _ = K.attn_fwd(x, B, N, H, scale, out_dtype=torch.float32, q_prescaled=prescaled, drop_p=p, seed=seed + 1)
    assert not torch.equal(out32, out0) and not torch.equal(out32, out2)
    check(out0.reshape(B, N, -1), O.attention_core(qkv.double().reshape(B, N, -1), H, scale), tol=tol, tol_max=tol_max, what="attn p=0")


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("p", [0.0, 0.25], ids=["no_dropout", "dropout"])
@pytest.mark.parametrize("prescaled", [True, False], ids=["q_prescaled", "plain_q"])
def test_attention_every_general_kernel_of_the_selector(K, prescaled, p, fmt):
    """The launchers look their kernel up in a table indexed by the fields of the selector's record (csrc/attn_plan.h): a table wired with two
    fields swapped still passes tests that only visit the production contract.  So every general head_dim-64 record -- forward: output type x q
    contract x dropout, backward: q contract x dropout, both formats -- is planned, asserted to be the record it is meant to be, run once at a
    shape with one row in the second query block, a clip boundary inside the grid and a head stride, and compared with the fp64 oracle (which
    regenerates the keep mask).  The head_dim-80 records are visited the same way, at the same shape, by the cases of
    test_attention_head_dim_80_fwd_bwd, which already ran every one of them.  Tolerances: those of the attention tests above."""
    from simple_tad_amd._lib import ATTN_BWD_DKV, ATTN_BWD_DQ, ATTN_FWD
    B, N, H, d, seed = 2, 129, 2, 64, 97531
    scale = d ** -0.5
    dt = torch.bfloat16 if fmt == "bf16" else torch.float16
    rnd = lambda t: t.to(dt).float()  # noqa: E731
    qkv = rnd(R.tensor_for(f"attsel.qkv{d}", (B * N, 3 * H * d), scale=1.0))
    dout = rnd(R.tensor_for(f"attsel.do{d}", (B * N, H * d)))
    opnd = qkv
    if prescaled:
        opnd, qkv = prescaled_pair(qkv, B, N, H, scale, rnd, d=d)
    qd = qkv.double().reshape(B, N, -1).requires_grad_()
    ref = O.attention_core(qd, H, scale, drop_p=p, seed=seed) if p else O.attention_core(qd, H, scale)
    ref.backward(dout.double().reshape(B, N, -1))
    kw = dict(q_prescaled=prescaled, drop_p=p, d=d)
    record = dict(hd=d, qs=int(prescaled), drop=int(p > 0), dma_mode=0, skip=0, has_lo=0, grid=2 * H * B, block=256)
    x = dev(opnd).to(dt)
    tol, tol_max = (ATT_TOL, ATT_TOL_MAX) if fmt == "bf16" else (ATT_TOL_F16, ATT_TOL_MAX_F16)
    ulp = BF16_ULP if fmt == "bf16" else 2 * tol

    def held(a, b, what, **bound):  # every figure is printed before it is asserted
        print(f"{what}: max-rel {relmax(a, b):.3e} l2-rel {rell2(a, b):.3e} (bound {bound})")
        check(a, b, what=what, **bound)
    assert K.attn_plan(B, N, H, out_16bit=False, **kw) == [dict(kernel=ATTN_FWD, out16=0, **record)]
    out32, lse = K.attn_fwd(x, B, N, H, scale, out_dtype=torch.float32, seed=seed, **kw)
    held(out32.reshape(B, N, -1), ref.detach(), "fwd f32", tol=tol, tol_max=tol_max)
    q4 = qkv.double().reshape(B, N, 3, H, d)
    sc = torch.einsum("bnhd,bmhd->bhnm", q4[:, :, 0], q4[:, :, 1]) * scale
    assert (lse.cpu().double() - torch.logsumexp(sc, -1)).abs().max().item() < 1e-3
    assert K.attn_plan(B, N, H, out_16bit=True, out_lo=True, **kw) == [dict(kernel=ATTN_FWD, out16=1, **record)]
    out16, lse16, lo = K.attn_fwd(x, B, N, H, scale, want_lo=True, seed=seed, **kw)
    held(out16.float().reshape(B, N, -1), ref.detach(), "fwd 16-bit", tol=ulp)
    assert torch.equal(lse16, lse) and torch.equal(lo.float(), (out32 - out16.float()).to(dt).float())
    assert K.attn_plan(B, N, H, backward=True, out_lo=True, **kw) == [dict(kernel=k, out16=1, **record) for k in (ATTN_BWD_DQ, ATTN_BWD_DKV)]
    dqkv = K.attn_bwd(x, out16, dev(dout).to(dt), lse, B, N, H, scale, out_lo=lo, seed=seed, **kw)
    g, r = dqkv.float().cpu().reshape(B, N, 3, H, d), qd.grad.reshape(B, N, 3, H, d)
    for i, nm in enumerate("qkv"):
        held(g[:, :, i], r[:, :, i], f"d{nm}", tol=2 * ulp)


def test_attention_dropout_in_the_model_is_reproducible_and_off_in_eval():
    import simple_tad_amd as T
    torch.manual_seed(0)
    m = T.VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True, all_frames=4,
                            tubelet_size=2, num_classes=2, init_scale=1.0, attn_drop_rate=0.2).cuda()
    x = torch.randn(2, 3, 4, 32, 32).cuda()
    m.train()
    torch.manual_seed(5); a = m(x); a.sum().backward()
    ga = m.blocks[0].attn.qkv.weight.grad.clone()
    m.zero_grad()
    torch.manual_seed(5); b = m(x); b.sum().backward()
    assert torch.equal(a, b) and torch.equal(ga, m.blocks[0].attn.qkv.weight.grad) and bool(torch.isfinite(ga).all())
    torch.manual_seed(6); c = m(x)
    assert not torch.equal(a, c)                     # another seed, another mask
    m.eval()
    with torch.no_grad():
        e1, e2 = m(x), m(x)
    m0 = T.VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True, all_frames=4,
                             tubelet_size=2, num_classes=2, init_scale=1.0, attn_drop_rate=0.0).cuda().eval()
    m0.load_state_dict(m.state_dict())
    with torch.no_grad():
        assert torch.equal(e1, e2) and torch.equal(e1, m0(x))   # no dropout in eval: the fused 16-bit path, same bits as a model without it
