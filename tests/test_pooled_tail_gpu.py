"""The pooled tail: the last block when only the token mean of its output is read (ops.BlockPoolFn, csrc/pooled_tail.hip).

  * tad_colsum_segments against an fp64 sum of the same 16-bit values, within the plain f32 summation bound;
  * tad_gelu_grad_bcast bit for bit against the kernel it replaces (tad_linear_bwd_input with the GELU' epilogue on the broadcast operand);
  * the fused function against BlockFn + MeanPoolFn: everything upstream of the MLP's hidden layer bit for bit; the pooled output, dW2
    and db2 (the same products in another f32 summation order) no further from an fp64 evaluation than twice the general path is;
  * the model's dispatch, and guard bands around every buffer of the two kernels.
"""
import contextlib

import pytest
import torch

import simple_tad_amd as T
from guarded import GuardedArena, POISON_MODES, same_bits
from simple_tad_amd import kernels as K, ops
from simple_tad_amd.modeling_finetune import Block
from test_guarded_gpu import guarded

pytestmark = pytest.mark.gpu

FMTS = {"bf16": (torch.bfloat16, "fast"), "f16": (torch.float16, "half")}
fmt = pytest.mark.parametrize("fmt", list(FMTS))
COLSUM_SHAPES = [(1, 1, 512), (3, 7, 512), (4, 129, 1536), (2, 1568, 3072), (3, 8, 512)]
DGELU_SHAPES = [(3, 8, 128), (4, 129, 128), (2, 1568, 768)]


@contextlib.contextmanager
def precision(mode):
    old = ops.get_precision()
    ops.set_precision(mode)
    try:
        yield
    finally:
        ops.set_precision(old)


def colsum_operand(B, N, Kc, dtype):
    g = torch.Generator().manual_seed(B * 100003 + N * 101 + Kc)
    a = torch.randn(B, N, Kc, generator=g).to(dtype)
    big = torch.finfo(dtype).max
    a[0, N // 2, :] = torch.tensor([big, -big, 0.0, -0.0], dtype=torch.float32).repeat(Kc // 4).to(dtype)  # a row of +-max-finite / 0
    a[B - 1, :, Kc // 2:] = (a[B - 1, :1, Kc // 2:].float().abs() * (1 - 2 * (torch.arange(N) % 2)).float().view(N, 1)).to(dtype)  # alternating signs
    return a


def dgelu_operands(B, N, D, dtype):
    """gb [B, D] (one clip dropped: dp2 = 0), wT [4D, D], h [B*N, 4D] on a grid through [-8, 8] with +-0, the GELU minimum and +-large values"""
    g = torch.Generator().manual_seed(B * 7919 + N * 13 + D)
    dp2 = torch.full((B,), 2.0)
    dp2[1] = 0.0
    grow = torch.randn(B, D, generator=g) * 0.01
    grow[1, ::2] *= -1.0
    gb = (grow * dp2.view(B, 1)).to(dtype)  # (the dropped clip: zeros of either sign)
    wT = (torch.randn(4 * D, D, generator=g) * 0.05).to(dtype)
    n = B * N * 4 * D
    special = torch.tensor([0.0, -0.0, -0.751791524693564457, -0.75, 8.0, -8.0, 4.5, -4.5, 5.0, -5.0, 60000.0, -60000.0, 1e-6, -1e-6])
    grid = torch.cat([torch.linspace(-8.0, 8.0, 4093), special])
    h = grid.repeat(n // grid.numel() + 1)[:n].reshape(B * N, 4 * D).to(dtype)
    return gb, wT, h


# =============================================================================================== tad_colsum_segments
@fmt
@pytest.mark.parametrize("B,N,Kc", COLSUM_SHAPES)
def test_colsum_segments_against_fp64(B, N, Kc, fmt):
    dtype = FMTS[fmt][0]
    a = colsum_operand(B, N, Kc, dtype)
    S = K.colsum_segments(a.cuda().reshape(B * N, Kc), B, N).cpu().double()
    ref = a.double().sum(1)
    bound = N * 2.0 ** -24 * a.double().abs().sum(1)  # the plain f32 summation bound, any order
    err = (S - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"\ncolsum_segments {fmt} {B} x {N} x {Kc}: worst |S - S64| / bound {worst:.3e}")
    assert bool((err <= bound).all()), (worst, int((err > bound).sum()))
    # deterministic: a second call gives the same bits
    assert torch.equal(K.colsum_segments(a.cuda().reshape(B * N, Kc), B, N).cpu().double(), S)


# =============================================================================================== tad_pooled_linear
POOLED_LINEAR_SHAPES = [(1, 1, 1, 8), (3, 7, 129, 512), (5, 129, 128, 1536), (2, 1568, 768, 3072)]  # D odd, B % 4 != 0, K / 8 <, =, > 256


def pooled_linear_operands(B, N, D, Kc, dtype):
    g = torch.Generator().manual_seed(B + 17 * N + 31 * D + Kc)
    S = torch.randn(B, Kc, generator=g) * N
    w = (torch.randn(D, Kc, generator=g) * 0.05).to(dtype)
    bias, xbar = torch.randn(D, generator=g) * 0.1, torch.randn(B, D, generator=g)
    scale = torch.full((B,), 2.0)
    scale[B // 2] = 0.0
    return S, w, bias, scale, xbar


@fmt
@pytest.mark.parametrize("B,N,D,Kc", POOLED_LINEAR_SHAPES)
def test_pooled_linear_against_fp64(B, N, D, Kc, fmt):
    """one rounding to f32 of xbar + scale ((S W^T) / N + bias), evaluated in f64 (products f32 x 16-bit are exact there): half an f32 ulp
    of the result, plus the f64 roundings in front of it: the accumulation bound K 2^-52 sum |s w| of the dot product and a few 2^-53
    relative roundings of u and of the sum (2^-49 (|xbar| + 2 |u|) covers them)"""
    S, w, bias, scale, xbar = pooled_linear_operands(B, N, D, Kc, FMTS[fmt][0])
    for has_bias, has_scale in ((True, True), (False, False)):
        out = K.pooled_linear(S.cuda(), w.cuda(), bias.cuda() if has_bias else None, scale.cuda() if has_scale else None, xbar.cuda(), N).cpu().double()
        u = S.double() @ w.double().t() / N + (bias.double() if has_bias else 0.0)
        sc = scale.double().view(B, 1) if has_scale else 1.0
        ref = xbar.double() + sc * u
        bound = 2.0 ** -24 * ref.abs() + 2.0 ** -49 * (xbar.double().abs() + 2.0 * u.abs()) + Kc * 2.0 ** -52 * (S.double().abs() @ w.double().abs().t()) * (2.0 / N) + 1e-300
        err = (out - ref).abs()
        assert bool((err <= bound).all()), (has_bias, has_scale, (err / bound).max().item())


@pytest.mark.parametrize("poison", POISON_MODES)
@fmt
@pytest.mark.parametrize("B,N,D,Kc", POOLED_LINEAR_SHAPES)
def test_pooled_linear_guard_bands(arena, B, N, D, Kc, fmt, poison):
    S, w, bias, scale, xbar = pooled_linear_operands(B, N, D, Kc, FMTS[fmt][0])
    out = guarded(K, arena, poison, lambda S, w, bias, scale, xbar: (K.pooled_linear(S, w, bias, scale, xbar, N),), S=S, w=w, bias=bias, scale=scale,
                  xbar=xbar)[0]
    assert bool(torch.isfinite(out).all())


# =============================================================================================== tad_gelu_grad_bcast
@fmt
@pytest.mark.parametrize("B,N,D", DGELU_SHAPES)
def test_gelu_grad_bcast_is_the_dgelu_epilogue_bit_for_bit(B, N, D, fmt):
    dtype = FMTS[fmt][0]
    gb, wT, h = (t.cuda() for t in dgelu_operands(B, N, D, dtype))
    gb_rows = gb.view(B, 1, D).expand(B, N, D).reshape(B * N, D).contiguous()
    want = K.linear_bwd_input(gb_rows, wT, gelu_preact=h)
    t = K.linear_bwd_input(gb, wT, out_dtype=torch.float32)
    got = K.gelu_grad_bcast(t, h, N)
    assert got.dtype == want.dtype == dtype and got.shape == want.shape
    w16, g16 = want.view(torch.int16), got.view(torch.int16)
    nbad = int((w16 != g16).sum())
    assert torch.equal(w16, g16), f"{nbad} of {w16.numel()} 16-bit words differ"
    zeros = g16.view(B, N, 4 * D)[1]
    assert bool(((zeros & 0x7FFF) == 0).all()), "the dropped clip's rows are zeros"


# =============================================================================================== BlockPoolFn vs BlockFn + MeanPoolFn
BLOCK_PARAMS = ("norm1.weight", "norm1.bias", "attn.q_bias", "attn.v_bias", "attn.qkv.weight", "attn.proj.weight", "attn.proj.bias",
                "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


def _block(D=128, H=2):
    torch.manual_seed(3)
    blk = Block(dim=D, num_heads=H, mlp_ratio=4, qkv_bias=True, init_values=0., drop_path=0.5,
                norm_layer=__import__("functools").partial(torch.nn.LayerNorm, eps=1e-6))
    with torch.no_grad():
        for k, p in blk.named_parameters():
            if k in ("norm1.weight", "norm2.weight"):
                p.copy_(1.0 + 0.2 * torch.randn_like(p))
            else:
                p.copy_(torch.randn_like(p) * (0.05 if p.dim() > 1 else 0.1))
    return blk.cuda().train()


class _Tap:
    """records operands of kernel calls made by ops (the kernels module is shared: patched for the duration of one run)"""

    def __init__(self):
        self.rec = {}

    @contextlib.contextmanager
    def on(self):
        saved = {n: getattr(K, n) for n in ("linear_fwd", "linear_bwd_input", "colsum_segments", "meanpool_fwd")}
        rec = self.rec

        def linear_fwd(x, w, bias=None, **kw):
            if kw.get("residual") is not None and x.shape[1] == 4 * w.shape[0]:  # fc2: a, x1
                rec["a"], rec["x1"], rec["w2"] = x.clone(), kw["residual"].clone(), w.clone()
            return saved["linear_fwd"](x, w, bias, **kw)

        def linear_bwd_input(dy, wT, out_dtype=None, gelu_preact=None):
            out = saved["linear_bwd_input"](dy, wT, out_dtype=out_dtype, gelu_preact=gelu_preact)
            if gelu_preact is not None:
                rec["gb_rows"], rec["dh"] = dy.clone(), out.clone()
            elif out_dtype == torch.float32:  # the pooled tail's B-row product t = gb W2
                rec["gb"] = dy.clone()
            return out

        def colsum_segments(a, B, N):
            rec["a"], rec["w2"] = a.clone(), None
            return saved["colsum_segments"](a, B, N)

        def meanpool_fwd(x):
            rec["pool_in"] = x.clone()
            return saved["meanpool_fwd"](x)

        for n, f in (("linear_fwd", linear_fwd), ("linear_bwd_input", linear_bwd_input), ("colsum_segments", colsum_segments),
                     ("meanpool_fwd", meanpool_fwd)):
            setattr(K, n, f)
        try:
            yield self
        finally:
            for n, f in saved.items():
                setattr(K, n, f)


def _run_block(blk, x, dy, scales, pooled, sinks):
    """one forward + backward of the block followed by the token mean; returns (pooled output, dx, {param: grad}, tap record)"""
    for p in blk.parameters():
        p.grad = None
    ops._sinks.clear()
    notified = []
    if sinks:
        ps = list(blk.parameters())
        flat = torch.zeros(sum(p.numel() for p in ps), device="cuda")
        o = 0
        for p in ps:
            v = flat[o:o + p.numel()].view_as(p)
            p.grad = v
            ops.register_grad_sink(p, v, notify=lambda prm, _n=notified: _n.append(id(prm)))
            o += p.numel()
    blk.drop_path.presampled = [s.clone() for s in scales]
    xg = x.clone().requires_grad_()
    tap = _Tap()
    with tap.on():
        out = blk.forward_pooled(xg) if pooled else ops.MeanPoolFn.apply(blk(xg))
        if pooled:  # (the pooled tail takes the token mean of x1; the general path's mean-pool reads x2)
            tap.rec["x1"] = tap.rec["pool_in"].reshape(-1, x.shape[-1])
        out.backward(dy)
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in blk.named_parameters()}
    ops._sinks.clear()
    for p in blk.parameters():
        p.grad = None
    return out.detach(), xg.grad.clone(), grads, tap.rec, sorted(notified)


def _dev(got, ref):
    d = got.double().cpu() - ref.cpu()
    return d.abs().max().item(), (d.norm() / ref.cpu().norm().clamp_min(1e-300)).item()


@fmt
@pytest.mark.parametrize("sinks", [False, True], ids=["autograd", "sinks"])
@pytest.mark.parametrize("N", [8, 129])
def test_block_pool_against_block_and_meanpool(N, sinks, fmt):
    dtype, mode = FMTS[fmt]
    B, D = 4, 128
    with precision(mode):
        blk = _block(D, 2)
        g = torch.Generator().manual_seed(N)
        x = torch.randn(B, N, D, generator=g).cuda()
        dy = (torch.randn(B, D, generator=g) * 0.1).cuda()
        keep = 0.5
        scales = [torch.tensor([1.0, 0.0, 1.0, 1.0]).cuda() / keep, torch.tensor([1.0, 1.0, 0.0, 1.0]).cuda() / keep]  # one dropped clip per branch
        ops.set_pooled_tail(True)
        assert blk.pools_fused()
        o_gen, dx_gen, g_gen, r_gen, n_gen = _run_block(blk, x, dy, scales, False, sinks)
        o_new, dx_new, g_new, r_new, n_new = _run_block(blk, x, dy, scales, True, sinks)
    # the same operands reach both tails, and the new path's gb is a row of the general path's operand
    assert same_bits(r_gen["a"], r_new["a"]) and same_bits(r_gen["x1"], r_new["x1"])
    assert same_bits(r_gen["gb_rows"].view(B, N, D)[:, 0].contiguous(), r_new["gb"]) and same_bits(r_gen["gb_rows"].view(B, N, D)[:, N - 1].contiguous(), r_new["gb"])
    if sinks:
        assert n_gen == n_new and len(n_new) > 0, "the same parameters are notified through their gradient sinks"
    # everything upstream of the MLP's hidden layer: bit for bit
    assert torch.equal(dx_gen, dx_new)
    for k in BLOCK_PARAMS:
        if k not in ("mlp.fc2.weight", "mlp.fc2.bias"):
            assert torch.equal(g_gen[k], g_new[k]), k
    # pooled output, dW2, db2: each path's deviation from fp64 on the same 16-bit operands
    a64, x164 = r_gen["a"].double().view(B, N, 4 * D), r_gen["x1"].double().view(B, N, D)
    w2 = r_gen["w2"].double()
    b2 = blk.mlp.fc2.bias.detach().double()
    dp2 = scales[1].double().view(B, 1, 1)
    ref = {"pooled": (x164 + dp2 * (a64 @ w2.t() + b2)).mean(1),
           "dW2": r_gen["gb_rows"].double().t() @ a64.view(B * N, 4 * D),
           "db2": r_gen["gb_rows"].double().sum(0)}
    got = {"pooled": (o_gen, o_new), "dW2": (g_gen["mlp.fc2.weight"], g_new["mlp.fc2.weight"]), "db2": (g_gen["mlp.fc2.bias"], g_new["mlp.fc2.bias"])}
    pairs = {k: (_dev(got[k][0], ref[k]), _dev(got[k][1], ref[k])) for k in ref}
    msg = "; ".join(f"{k}: general max-abs {p[0][0]:.3e} rel-l2 {p[0][1]:.3e}, pooled tail max-abs {p[1][0]:.3e} rel-l2 {p[1][1]:.3e}" for k, p in pairs.items())
    print(f"\nblock + mean-pool {fmt} N={N} {'sinks' if sinks else 'autograd'}: {msg}")
    for k, (gen, new) in pairs.items():
        assert new[0] <= 2.0 * gen[0] and new[1] <= 2.0 * gen[1], msg


# =============================================================================================== dispatch
def _tiny(depth=3, **kw):
    torch.manual_seed(0)
    m = T.VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=depth, num_heads=2, mlp_ratio=4, qkv_bias=True,
                            all_frames=4, tubelet_size=2, num_classes=2, init_scale=1.0, **kw)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.02)
    return m.cuda().train()


def _step(m, x):
    m.zero_grad(set_to_none=True)
    before = ops._PoolStats.calls
    ops._chain.hits = 0
    out = m(x)
    torch.nn.functional.cross_entropy(out, torch.tensor([1, 0], device="cuda")).backward()
    return ops._PoolStats.calls - before, {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def test_dispatch_takes_the_pooled_tail_only_where_it_is_valid():
    x = torch.randn(2, 3, 4, 32, 32).cuda()
    depth = 3
    ops.set_pooled_tail(True)
    try:
        m = _tiny(depth)
        n, g_on = _step(m, x)
        assert n == 1 and ops._chain.hits == depth - 1 and ops._chain.pending == 0
        # switch off: the route of before, bit for bit the composition patch_embed -> blocks -> MeanPoolFn -> fc_norm -> head
        ops.set_pooled_tail(False)
        n, g_off = _step(m, x)
        assert n == 0 and ops._chain.hits == depth - 1 and ops._chain.pending == 0
        m.zero_grad(set_to_none=True)
        t = m.patch_embed(x, pos_embed=m._pos_on(x.device))
        for blk in m.blocks:
            t = blk(t)
        out = m.head(m._ln(m.fc_norm, ops.MeanPoolFn.apply(t)))
        torch.nn.functional.cross_entropy(out, torch.tensor([1, 0], device="cuda")).backward()
        for k, p in m.named_parameters():
            assert torch.equal(p.grad, g_off[k]), k
        ops.set_pooled_tail(True)
        # a forward hook on the last block must see its [B, N, D] output: general route
        seen = []
        hd = m.blocks[-1].register_forward_hook(lambda mod, i, o: seen.append(tuple(o.shape)))
        n, g_hook = _step(m, x)
        hd.remove()
        assert n == 0 and seen == [(2, 8, 128)]
        for k in g_off:
            assert torch.equal(g_hook[k], g_off[k]), k
        # final_reduction="cls": every token row is read by nothing but row 0 -- not a mean
        assert _step(_tiny(depth, final_reduction="cls"), x)[0] == 0
        # precise mode (forward only)
        with precision("precise"), torch.no_grad():
            before = ops._PoolStats.calls
            m.eval()(x)
            assert ops._PoolStats.calls == before
        m.train()
        # eval / no_grad forwards take it too and agree with the general route within f32 re-association of the pooled features
        with torch.no_grad():
            before = ops._PoolStats.calls
            f_on = m.eval().forward_features(x)
            assert ops._PoolStats.calls == before + 1
            ops.set_pooled_tail(False)
            f_off = m.forward_features(x)
            ops.set_pooled_tail(True)
        assert (f_on - f_off).abs().max().item() <= 1e-4 * f_off.abs().max().item()
        m.train()
        # use_checkpoint: the last block + mean-pool is the last checkpointed unit and runs the same function (forward and recompute), so
        # that the checkpointed and the plain model keep giving the same bits (tests/test_variants_gpu.py, tests/test_grad_parity_gpu.py pin that)
        mc = _tiny(depth, use_checkpoint=True)
        mc.load_state_dict(m.state_dict())
        n, g_ck = _step(mc, x)
        assert n == 2
        for k in g_on:
            assert torch.equal(g_ck[k], g_on[k]), k
    finally:
        ops.set_pooled_tail(True)


# =============================================================================================== guard bands
@pytest.fixture(scope="module")
def arena():
    return GuardedArena(160 << 20, "cuda")


@pytest.mark.parametrize("poison", POISON_MODES)
@fmt
@pytest.mark.parametrize("B,N,Kc", COLSUM_SHAPES)
def test_colsum_segments_guard_bands(arena, B, N, Kc, fmt, poison):
    a = colsum_operand(B, N, Kc, FMTS[fmt][0]).reshape(B * N, Kc)
    S = guarded(K, arena, poison, lambda a: (K.colsum_segments(a, B, N),), a=a)[0]
    assert bool(torch.isfinite(S).all())


@pytest.mark.parametrize("poison", POISON_MODES)
@fmt
@pytest.mark.parametrize("B,N,D", DGELU_SHAPES)
def test_gelu_grad_bcast_guard_bands(arena, B, N, D, fmt, poison):
    gb, wT, h = dgelu_operands(B, N, D, FMTS[fmt][0])
    t = K.linear_bwd_input(gb.cuda(), wT.cuda(), out_dtype=torch.float32).cpu()
    dh = guarded(K, arena, poison, lambda t, h: (K.gelu_grad_bcast(t, h, N),), t=t, h=h)[0]
    assert not bool(torch.isnan(dh.float()).any())
