"""The fused Block variants on the GPU: the four kernels of csrc/layerscale.hip one by one (bit-exact where the contract is a single
rounding, a priori rounding bounds elsewhere, guard-band arenas at ragged shapes), then whole layer-scale / dropout blocks through
ops.BlockVariantFn against the fp64 oracle."""
import functools

import pytest
import torch
import torch.utils.checkpoint as checkpoint

import block_variants_recipe as V
import golden_recipe as R
import simple_tad_amd as T
from guarded import GuardedArena, POISON_MODES, same_bits
from simple_tad_amd import ops
from simple_tad_amd.modeling_finetune import DropPath

pytestmark = pytest.mark.gpu

FMTS = {"bf16": torch.bfloat16, "f16": torch.float16}
NK = [(1, 1), (5, 3), (130, 67), (768, 3072)]
MD = [(3, 5), (130, 260), (2 * 197, 128)]
RPS = [1, 7, 197]
fmt = pytest.mark.parametrize("fmt", list(FMTS))


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import _lib, kernels
    _lib.load()
    return kernels


def rnd(seed, *shape, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).cuda()


def rowscale_for(M, rps, seed=0):
    """drop-path scales [ceil(M / rps)]: 0 or 2 (keep_prob 0.5), at least one of each when there is room"""
    n = -(-M // rps)
    g = torch.Generator().manual_seed(100 + seed)
    s = (torch.rand(n, generator=g) < 0.5).float() * 2.0
    s[-1] = 2.0
    if n > 1:
        s[0] = 0.0
    return s.cuda()


def rows_of(s, M, rps):
    return s[torch.arange(M, device=s.device) // rps]


# ----------------------------------------------------------------------------- tad_rowscale_transpose_cast
@fmt
@pytest.mark.parametrize("N,Kd", NK)
def test_rowscale_transpose_cast_is_bit_exact(K, N, Kd, fmt):
    W, gamma = rnd(1, N, Kd), rnd(2, N, shift=0.1)
    out = K.rowscale_transpose_cast(W, gamma, dtype=FMTS[fmt])
    ref = (gamma[:, None] * W).to(FMTS[fmt]).t().contiguous()
    assert out.shape == (Kd, N) and out.dtype == FMTS[fmt] and same_bits(out, ref)


# ----------------------------------------------------------------------------- tad_layerscale_grads
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("N,Kd", NK)
def test_layerscale_grads(K, N, Kd, with_bias):
    Tm, W, gamma = rnd(3, N, Kd), rnd(4, N, Kd, scale=0.02), rnd(5, N, scale=0.05, shift=0.1)
    bias = rnd(6, N, scale=0.02) if with_bias else None
    cs = rnd(7, N) if with_bias else None
    dW, db, dg = K.layerscale_grads(Tm, W, bias, cs, gamma)
    # write mode: dW and dbias are single f32 products
    assert same_bits(dW, gamma[:, None] * Tm)
    assert (db is None) == (not with_bias)
    if with_bias:
        assert same_bits(db, gamma * cs)
    # dgamma: any f32 summation of the K products (+ the bias term) lies within gamma_{K+2} of the exact sum of their magnitudes
    Td, Wd = Tm.double(), W.double()
    ref = (Td * Wd).sum(1) + (bias.double() * cs.double() if with_bias else 0.0)
    mag = (Td * Wd).abs().sum(1) + ((bias.double() * cs.double()).abs() if with_bias else 0.0)
    bound = V.gamma_n(Kd + 2) * mag
    err = (dg.double() - ref).abs()
    print(f"\n[{N},{Kd}] dgamma: worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    # two runs: the same bits
    dW2, db2, dg2 = K.layerscale_grads(Tm, W, bias, cs, gamma)
    assert same_bits(dW, dW2) and same_bits(dg, dg2) and (db is None or same_bits(db, db2))
    # accumulate mode (gradient sinks): old + new, one product and one sum (or one fused multiply-add) per element
    oW, og = rnd(8, N, Kd), rnd(9, N)
    ob = rnd(10, N) if with_bias else None
    aW, ag = oW.clone(), og.clone()
    ab = ob.clone() if with_bias else None
    r = K.layerscale_grads(Tm, W, bias, cs, gamma, dW=aW, dbias=ab, dgamma=ag, accumulate=True)
    assert r[0].data_ptr() == aW.data_ptr() and r[2].data_ptr() == ag.data_ptr()
    newW = gamma.double()[:, None] * Td
    assert bool(((aW.double() - (oW.double() + newW)).abs() <= 2.0 ** -23 * (oW.double().abs() + newW.abs())).all())
    assert bool(((ag.double() - (og.double() + ref)).abs() <= 2.0 ** -23 * (og.double().abs() + ref.abs()) + bound).all())
    if with_bias:
        newb = gamma.double() * cs.double()
        assert bool(((ab.double() - (ob.double() + newb)).abs() <= 2.0 ** -23 * (ob.double().abs() + newb.abs())).all())


# ----------------------------------------------------------------------------- tad_branch_dropout_fwd / _cast
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("M,D", MD)
def test_dropout_mask_pattern_is_the_restated_one(K, M, D, p):
    """u = 1, res = 0: the output is exactly 0 or fl(1 / (1 - p)) in the pattern of the numpy mask"""
    seed = 77 + M
    keep = V.branch_keep(M, D, p, seed).cuda()
    assert 0 < int(keep.sum()) < M * D
    ik = torch.tensor(V.inv_keep_f32(p), dtype=torch.float32, device="cuda")
    out = K.branch_dropout_fwd(torch.ones(M, D, device="cuda"), torch.zeros(M, D, device="cuda"), p=p, seed=seed)
    assert same_bits(out, torch.where(keep, ik, torch.zeros((), device="cuda")).expand(M, D).contiguous())
    for name, dt in FMTS.items():
        c = K.branch_dropout_cast(torch.ones(M, D, device="cuda"), p=p, seed=seed, dtype=dt)
        assert same_bits(c, torch.where(keep, ik, torch.zeros((), device="cuda")).expand(M, D).contiguous().to(dt)), name


@pytest.mark.parametrize("with_gamma", [True, False])
@pytest.mark.parametrize("rps", RPS)
@pytest.mark.parametrize("M,D", MD)
def test_branch_dropout_fwd_general(K, M, D, rps, with_gamma):
    p, seed = 0.3, 2 ** 31 - 5
    u, res = rnd(11, M, D), rnd(12, M, D)
    gamma = rnd(13, D, scale=0.05, shift=0.1) if with_gamma else None
    s = rowscale_for(M, rps)
    sr = rows_of(s, M, rps)
    dead = (sr == 0).nonzero().reshape(-1)
    if s.numel() == 1:  # one scale for every row: the dropped case is the whole tensor
        bad = u.clone()
        bad[0, 0], bad[M - 1, D - 1] = float("inf"), float("nan")
        assert same_bits(K.branch_dropout_fwd(bad, res, gamma, torch.zeros_like(s), rps, p, seed), res)
    else:
        assert 0 < dead.numel() < M
        u[dead[0], 0], u[dead[-1], D - 1] = float("inf"), float("nan")     # must not leak: a select, not a product with 0
    out = K.branch_dropout_fwd(u, res, gamma, s, rps, p, seed)
    keep = V.branch_keep(M, D, p, seed).cuda()
    live = keep & (sr != 0)[:, None]
    assert same_bits(out[~live], res[~live]), "dropped elements and rows of dropped clips must be res bit for bit"
    gm = gamma.double() if with_gamma else torch.ones(D, dtype=torch.float64, device="cuda")
    term = torch.where(live, sr.double()[:, None] * gm * V.inv_keep_f32(p) * torch.where(live, u, torch.zeros_like(u)).double(),
                       torch.zeros((), dtype=torch.float64, device="cuda"))
    err = (out.double() - (res.double() + term)).abs()
    bound = 4 * V.U24 * (res.double().abs() + term.abs())
    print(f"\n[{M},{D}] rps {rps}: worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())


@fmt
@pytest.mark.parametrize("rps", RPS)
@pytest.mark.parametrize("M,D", MD)
def test_branch_dropout_cast_rounds_like_torch(K, M, D, rps, fmt):
    p, seed = 0.3, 123456789
    g = rnd(14, M, D)
    s = rowscale_for(M, rps, seed=1)
    sr = rows_of(s, M, rps)
    dead = (sr == 0).nonzero().reshape(-1)
    if s.numel() == 1:
        bad = g.clone()
        bad[0, D - 1] = float("inf")
        assert same_bits(K.branch_dropout_cast(bad, torch.zeros_like(s), rps, p, seed, dtype=FMTS[fmt]), torch.zeros(M, D, device="cuda", dtype=FMTS[fmt]))
    else:
        g[dead[0], D - 1] = float("inf")
    out = K.branch_dropout_cast(g, s, rps, p, seed, dtype=FMTS[fmt])
    live = V.branch_keep(M, D, p, seed).cuda() & (sr != 0)[:, None]
    f = sr * V.inv_keep_f32(p)                               # one f32 factor per row
    ref = torch.where(live, g * f[:, None], torch.zeros_like(g)).to(FMTS[fmt])
    assert same_bits(out, ref)
    # without a rowscale and with p = 0 it is the plain cast
    assert same_bits(K.branch_dropout_cast(rnd(15, M, D), dtype=FMTS[fmt]), rnd(15, M, D).to(FMTS[fmt]))


# ----------------------------------------------------------------------------- guard-band arenas, ragged shapes
@pytest.fixture(scope="module")
def arena():
    return GuardedArena(96 << 20, "cuda")


def guarded(K, arena, mode, fn, inout=(), **tensors):
    """fn(**tensors) on plain copies and on arena placements (the wrapper's allocations routed into the arena): no byte outside the
    writable operands changes and the guarded results equal the plain ones bit for bit"""
    plain = fn(**{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in tensors.items()})
    torch.cuda.synchronize()
    plain = [None if t is None else t.clone() for t in plain]
    arena.reset(mode)
    placed = {k: (arena.place(v.cpu(), role="inout" if k in inout else "input", name=k) if isinstance(v, torch.Tensor) else v)
              for k, v in tensors.items()}
    with arena.route(K):
        got = fn(**placed)
    arena.verify()
    assert len(got) == len(plain)
    for i, (a, b) in enumerate(zip(plain, got)):
        assert (a is None) == (b is None)
        if a is not None:
            assert arena.contains(b), f"output {i} was allocated outside the arena"
            assert same_bits(a, b), f"output {i}: the guarded run differs in bits (the result depends on bytes outside the operands)"


@pytest.mark.parametrize("poison", POISON_MODES)
def test_new_wrappers_inside_guard_bands(K, arena, poison):
    for N, Kd in ((5, 3), (130, 67), (132, 68)):
        W, Tm, gamma, bias, cs = rnd(20, N, Kd), rnd(21, N, Kd), rnd(22, N), rnd(23, N), rnd(24, N)
        for dt in FMTS.values():
            guarded(K, arena, poison, lambda w, gamma: (K.rowscale_transpose_cast(w, gamma, dtype=dt),), w=W, gamma=gamma)
        guarded(K, arena, poison, lambda **t: K.layerscale_grads(t["T"], t["W"], t["bias"], t["cs"], t["gamma"]), T=Tm, W=W, bias=bias, cs=cs,
                gamma=gamma)
        guarded(K, arena, poison, lambda **t: K.layerscale_grads(t["T"], t["W"], t["bias"], t["cs"], t["gamma"], dW=t["dW"], dbias=t["db"],
                                                                 dgamma=t["dg"], accumulate=True),
                inout=("dW", "db", "dg"), T=Tm, W=W, bias=bias, cs=cs, gamma=gamma, dW=rnd(25, N, Kd), db=rnd(26, N), dg=rnd(27, N))
    for (M, D), rps in zip(MD, RPS):
        u, res, gamma, s = rnd(30, M, D), rnd(31, M, D), rnd(32, D), rowscale_for(M, rps)
        guarded(K, arena, poison, lambda u, res, gamma, s: (K.branch_dropout_fwd(u, res, gamma, s, rps, 0.3, 99),), u=u, res=res, gamma=gamma,
                s=s)
        for dt in FMTS.values():
            guarded(K, arena, poison, lambda g, s: (K.branch_dropout_cast(g, s, rps, 0.3, 99, dtype=dt),), g=u, s=s)


# ----------------------------------------------------------------------------- whole blocks
C = R.TINY
DEPTH, D_ = 3, R.TINY["embed_dim"]
MASKS = {1: ([0.0, 1.0], [1.0, 0.0]), 2: ([1.0, 0.0], [0.0, 1.0])}      # the injected drop-path masks of the layer-scale oracle test
SEEDS = {0: (11, 2 ** 31 - 2), 1: (0, 987654321), 2: (31337, 42)}


def build_model(init_values=0.1, drop_rate=0.0, use_checkpoint=False):
    m = T.VisionTransformer(img_size=C["img_size"], patch_size=C["patch_size"], embed_dim=D_, depth=DEPTH, num_heads=C["num_heads"],
                            mlp_ratio=4, qkv_bias=True, norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6),
                            all_frames=C["all_frames"], tubelet_size=C["tubelet_size"], num_classes=C["num_classes"], init_scale=1.0,
                            init_values=init_values, drop_rate=drop_rate, drop_path_rate=0.5, use_checkpoint=use_checkpoint)
    P = R.params_for(R.vit_param_shapes(D_, DEPTH, C["num_classes"], tubelet=C["tubelet_size"], patch=C["patch_size"]), seed=5)
    if init_values > 0:
        for i in range(DEPTH):
            for gname in ("gamma_1", "gamma_2"):
                P[f"blocks.{i}.{gname}"] = R.tensor_for(f"ls.{i}.{gname}", (D_,), scale=0.05, shift=0.1)
    m.load_state_dict(P, strict=True)
    return m.cuda().train(), P


def run_blocks(m, xin, dy, seeds=None, masks=MASKS, ckpt=False, reset_grads=True):
    """forward + backward through the blocks with the injected drop-path masks (and dropout seeds); returns (out, dx, grads by name)"""
    for i, (m1, m2) in masks.items():
        keep = 1.0 - m.blocks[i].drop_path.drop_prob
        m.blocks[i].drop_path.presampled = [torch.tensor(m1, device="cuda") / keep, torch.tensor(m2, device="cuda") / keep]
    for i, blk in enumerate(m.blocks):
        blk.forced_drop_seeds = seeds[i] if seeds else None
    if reset_grads:
        for p in m.parameters():
            p.grad = None
    xg = xin.cuda().requires_grad_()
    t = xg
    for blk in m.blocks:
        t = checkpoint.checkpoint(blk, t, use_reentrant=False) if ckpt else blk(t)
    t.backward(dy.cuda())
    return t.detach(), xg.grad, {k: p.grad.clone() for k, p in m.blocks.named_parameters()}


def oracle_blocks(m, P, xin, dy, drop_p=0.0, seeds=None):
    Pd = {k: v.double().requires_grad_() for k, v in P.items() if k.startswith("blocks.")}
    xd = xin.double().requires_grad_()
    r = xd
    for i in range(DEPTH):
        km = [torch.tensor(v, dtype=torch.float64) for v in MASKS[i]] if i in MASKS else None
        r = V.block_fp64(r, Pd, f"blocks.{i}.", C["num_heads"], keep_masks=km,
                         keep_prob=1.0 - m.blocks[i].drop_path.drop_prob if km else 1.0, drop_p=drop_p,
                         drop_seeds=seeds[i] if seeds else (0, 0))
    r.backward(dy.double())
    return r.detach(), xd.grad, {k[len("blocks."):]: v.grad for k, v in Pd.items()}


def rell2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def errors(run, ref):
    e = {"output": rell2(run[0], ref[0]), "input gradient": rell2(run[1], ref[1])}
    e.update({k: rell2(g, ref[2][k]) for k, g in run[2].items()})
    return e


def check_against_oracle(e, n_params, tol_out=5e-3, tol_dx=1e-2, tol_p=2e-2):
    assert len(e) == 2 + n_params
    assert e["output"] < tol_out and e["input gradient"] < tol_dx, (e["output"], e["input gradient"])
    for k, v in e.items():
        assert v < tol_p, (k, v)


XIN = R.tensor_for("ls.x", (2, 8, D_))
DY = R.tensor_for("ls.dy", (2, 8, D_))


def test_layer_scale_blocks_through_the_fused_route_vs_oracle():
    """(a) layer-scale + injected drop-path masks through ops.BlockVariantFn, every gradient against the fp64 oracle at the tolerances of
    test_layer_scale_training_with_drop_path_vs_oracle; next to each error its ratio to the composed route's on the same inputs"""
    m, P = build_model(init_values=0.1)
    assert all(not b._fusable() for b in m.blocks)
    n0 = ops.block_variant_calls
    fused = run_blocks(m, XIN, DY)
    assert ops.block_variant_calls == n0 + DEPTH
    assert all(not b.drop_path.presampled for b in m.blocks if isinstance(b.drop_path, DropPath))
    ops.set_block_variants(False)
    try:
        composed = run_blocks(m, XIN, DY)
        assert ops.block_variant_calls == n0 + DEPTH
    finally:
        ops.set_block_variants(True)
    ref = oracle_blocks(m, P, XIN, DY)
    ef, ec = errors(fused, ref), errors(composed, ref)
    print("\nlayer scale + drop path, 3 blocks: rel-L2 error of the fused route (ratio to the composed route's)")
    for k in ef:
        print(f"  {k:<28} {ef[k]:.2e}  ({ef[k] / max(ec[k], 1e-30):.2f}x)")
    check_against_oracle(ef, DEPTH * 15)
    assert sum("gamma" in k for k in ef) == 2 * DEPTH


@pytest.mark.parametrize("init_values", [0.1, 0.0])
def test_dropout_blocks_vs_fp64_block(init_values):
    """(b) drop_rate 0.3 with injected seeds, with and without layer-scale, against the fp64 block fed the restated mask"""
    m, P = build_model(init_values=init_values, drop_rate=0.3)
    assert all(not b._fusable() and b._variant_fusable() for b in m.blocks)
    n0 = ops.block_variant_calls
    fused = run_blocks(m, XIN, DY, seeds=SEEDS)
    assert ops.block_variant_calls == n0 + DEPTH
    ref = oracle_blocks(m, P, XIN, DY, drop_p=0.3, seeds=SEEDS)
    e = errors(fused, ref)
    worst = max((k for k in e if k not in ("output", "input gradient")), key=e.get)
    print(f"\ndropout 0.3, init_values {init_values}: output {e['output']:.2e} input gradient {e['input gradient']:.2e} "
          f"parameters worst {e[worst]:.2e} ({worst})")
    check_against_oracle(e, DEPTH * (15 if init_values > 0 else 13))
    # other seeds give another mask
    other = run_blocks(m, XIN, DY, seeds={i: (a + 1, b + 1) for i, (a, b) in SEEDS.items()})
    assert not torch.equal(other[0], fused[0])


def test_gradient_sinks_match_returned_gradients_and_accumulate():
    """(c) with FusedAdamW (gradient sinks on every parameter) one backward matches the no-sink run within 1e-6, and two micro-steps
    accumulate to their sum"""
    from simple_tad_amd.optim import FusedAdamW
    m, _ = build_model(init_values=0.1, drop_rate=0.3)
    base = run_blocks(m, XIN, DY, seeds=SEEDS)
    for p in m.parameters():
        p.grad = None
    seen, orig = [], ops.K.layerscale_grads
    try:
        opt = FusedAdamW(list(m.blocks.parameters()), lr=0.0, weight_decay=0.0)
        opt.zero_grad()
        flat = {k: p.grad.data_ptr() for k, p in m.blocks.named_parameters()}
        ops.K.layerscale_grads = lambda *a, **kw: (seen.append(bool(kw.get("accumulate"))), orig(*a, **kw))[1]
        one = run_blocks(m, XIN, DY, seeds=SEEDS, reset_grads=False)
        assert seen == [True] * (2 * DEPTH), "gamma / proj / fc2 gradients must accumulate into the sinks"
        assert {k: p.grad.data_ptr() for k, p in m.blocks.named_parameters()} == flat, "a gradient left the flat buffer"
        assert torch.equal(one[0], base[0])
        assert rell2(one[1], base[1]) < 1e-6
        for k, g in one[2].items():
            assert rell2(g, base[2][k]) < 1e-6, (k, rell2(g, base[2][k]))
        # second micro-step on top of the first (no zero_grad in between)
        two = run_blocks(m, XIN, DY, seeds=SEEDS, reset_grads=False)
        for k, p in m.blocks.named_parameters():
            assert p.grad.data_ptr() == flat[k]
            assert rell2(two[2][k], 2.0 * one[2][k].double()) < 1e-6, (k, rell2(two[2][k], 2.0 * one[2][k].double()))
    finally:
        ops.K.layerscale_grads = orig
        ops.invalidate_weight_cache()


def test_checkpointing_reproduces_the_gradients_bit_for_bit():
    """(d) use_checkpoint: the recomputation draws the same dropout seeds (torch's generator state is restored) and the same gradients"""
    m, _ = build_model(init_values=0.1, drop_rate=0.3)
    for blk in m.blocks:   # (drop path by a fixed mask: the recomputation must not depend on a list that the first forward emptied)
        if isinstance(blk.drop_path, DropPath):
            blk.drop_path.forced_mask = torch.tensor([1.0, 0.0])
    torch.manual_seed(7)
    plain = run_blocks(m, XIN, DY, masks={})
    torch.manual_seed(7)
    n0 = ops.block_variant_calls
    ck = run_blocks(m, XIN, DY, masks={}, ckpt=True)
    assert ops.block_variant_calls == n0 + 2 * DEPTH, "forward and recomputation both take the fused route"
    assert torch.equal(ck[0], plain[0]) and torch.equal(ck[1], plain[1])
    for k, g in ck[2].items():
        assert torch.equal(g, plain[2][k]), k
    torch.manual_seed(8)
    assert not torch.equal(run_blocks(m, XIN, DY, masks={})[0], plain[0])   # another generator state: other seeds, another mask


def test_half_precision_layer_scale_blocks_vs_oracle():
    """(e) the "half" mode through the fused route: output and input gradient within test_half_gpu's kernel tolerance (1e-3), every
    parameter gradient within its per-parameter bound for a small model (5e-3)"""
    m, P = build_model(init_values=0.1)
    T.set_precision("half")
    try:
        n0 = ops.block_variant_calls
        fused = run_blocks(m, XIN, DY)
        assert ops.block_variant_calls == n0 + DEPTH
    finally:
        T.set_precision("fast")
    e = errors(fused, oracle_blocks(m, P, XIN, DY))
    worst = max((k for k in e if k not in ("output", "input gradient")), key=e.get)
    print(f"\nhalf: output {e['output']:.2e} input gradient {e['input gradient']:.2e} parameters worst {e[worst]:.2e} ({worst})")
    check_against_oracle(e, DEPTH * 15, tol_out=1e-3, tol_dx=1e-3, tol_p=5e-3)


def test_eval_mode_routes():
    """(f) eval: a layer-scale block runs through BlockVariantFn.  Measured on MI355X: bit-identical to the composed route on these inputs.
    Bits are not asserted: the composed route rounds proj's f32 output, the product with gamma and the residual sum one after the other,
    while the GEMM epilogue may form res + gamma * (acc + bias) with fewer roundings, so the two may differ at f32 rounding level (bound
    below).  A drop_rate > 0 block in eval is the plain fused block (BlockFn)."""
    m, _ = build_model(init_values=0.1)
    m.eval()
    blk = m.blocks[1]
    x = XIN.cuda()
    with torch.no_grad():
        n0 = ops.block_variant_calls
        a = blk(x)
        assert ops.block_variant_calls == n0 + 1
        ops.set_block_variants(False)
        try:
            b = blk(x)
        finally:
            ops.set_block_variants(True)
        assert ops.block_variant_calls == n0 + 1
    # f32 rounding of two residual sums (a few 2^-24 of the stream), which the 16-bit rounding of norm2's output may turn into one
    # 16-bit ulp (2^-9) of single operand elements of the MLP; behind fc1 / fc2 weights of size 0.02 and gamma of size 0.1 such a flip
    # moves a row of the output by ~1e-6 of the stream: 1e-5 in rel-L2 covers both with room
    d = rell2(a, b)
    print(f"\neval layer-scale block, fused vs composed: rel-L2 {d:.3e}, max |diff| {float((a - b).abs().max()):.3e}, bit-identical: {torch.equal(a, b)}")
    assert d < 1e-5
    md, _ = build_model(init_values=0.0, drop_rate=0.3)
    md.eval()
    with torch.no_grad():
        n0 = ops.block_variant_calls
        assert md.blocks[0]._fusable()
        md.blocks[0](x)
        assert ops.block_variant_calls == n0
