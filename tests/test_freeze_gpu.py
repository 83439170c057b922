"""Frozen layers (engine.freeze_layers + ops.set_skip_frozen): a frozen weight costs no weight-gradient launch, no bias column sums
and no saved operand, its 16-bit operand copies are made once, and everything that is still computed -- the logits, the loss, every
trainable gradient, the input-gradient chain, whole training steps -- keeps its bits against the switch-off path, which computes and
saves everything whatever the flags say.  Shapes: embed 128 / 2 heads (head_dim 64) and embed 320 / 4 heads (head_dim 80: the GEMMs
take reduction lengths that are multiples of 64 only, so 320 is the smallest width with that head), depth 3, patch 16, tubelet 2,
4 frames of 48 x 48 -> 18 tokens (a ragged tile), batch 3: M = 54 rows."""
import types
from contextlib import contextmanager

import pytest
import torch
import torch.nn.functional as F

import golden_recipe as R
import simple_tad_amd as T
from oracle import vit_oracle as O
from simple_tad_amd import engine as E, kernels as K, ops
from simple_tad_amd.modeling_finetune import DropPath
from simple_tad_amd.optim import FusedAdamW
from simple_tad_amd.parallel import DataParallel
from test_grad_parity_gpu import BOUND, HALF_SCALE, whole_err

pytestmark = pytest.mark.gpu

DEPTH, B, NTOK = 3, 3, 18
M = B * NTOK
KPATCH = 3 * 2 * 16 * 16  # columns of the patch matrix
MODES = ["fast", "half"]
WGRAD = ("linear_bwd_weight", "linear_bwd_weight_qkv", "linear_bwd_weight_pair", "patch_embed_bwd", "layerscale_grads")


@pytest.fixture(autouse=True)
def _restore_switches():
    yield
    ops.set_skip_frozen(True)
    ops.set_pooled_tail(True)
    T.set_precision("fast")
    ops.invalidate_weight_cache()


def build(embed=128, freeze=None, **kw):
    torch.manual_seed(0)
    cfg = dict(img_size=48, patch_size=16, embed_dim=embed, depth=DEPTH, num_heads=embed // (64 if embed == 128 else 80), all_frames=4, tubelet_size=2, num_classes=3,
               mlp_ratio=4, qkv_bias=True, init_scale=1.0)
    cfg.update(kw)
    m = T.VisionTransformer(**cfg)
    R.rerandomize_1d(m)
    m = m.cuda().train()
    if freeze is not None:
        assert E.freeze_layers(m, f"first N blocks;{freeze}") > 0
    return m


def batch(seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, 4, 48, 48, generator=g).cuda(), torch.tensor([1, 1, 1]).cuda()  # (one label: see test_grad_parity_gpu)


@contextmanager
def counting(names=None):
    """wrap wrappers of simple_tad_amd.kernels with call recorders (ops looks every one up on the module at call time); yields the
    ordered list of (name, first argument's shape | None).  names=None: every public function the module defines or aliases."""
    if names is None:
        names = [n for n, f in vars(K).items() if isinstance(f, types.FunctionType) and f.__module__ == K.__name__ and not n.startswith("_")]
    calls, orig = [], {}
    for n in names:
        f = getattr(K, n, None)
        if f is None:  # (there is no kernels.patch_embed_bwd: the patch projection's gradient is a linear_bwd_weight over the patch matrix)
            continue
        orig[n] = f

        def rec(*a, _n=n, _f=f, **k):
            calls.append((_n, tuple(a[0].shape) if a and isinstance(a[0], torch.Tensor) else None, a, k))
            return _f(*a, **k)
        setattr(K, n, rec)
    try:
        yield calls
    finally:
        for n, f in orig.items():
            setattr(K, n, f)


def wgrad_counts(calls):
    """launch counts of the weight-gradient wrappers; the patch projection's (a linear_bwd_weight whose x operand is the patch matrix)
    apart, as ``patch``"""
    c = {n: 0 for n in WGRAD + ("patch",)}
    for n, _, a, k in calls:
        if n == "linear_bwd_weight" and a[1].shape[1] == KPATCH:
            c["patch"] += 1
        elif n in c:
            c[n] += 1
    return c


def step(m, x, y, mode, skip, seed=3, scale=None, grab=True):
    """one forward + CE + backward; returns logits, loss, {name: grad | None}, gradient at block 0's input"""
    T.set_precision(mode)
    ops.set_skip_frozen(skip)
    m.zero_grad(set_to_none=True)
    leaf, h = [], None
    if grab:
        def pre(mod, args):
            leaf.append(args[0].detach().requires_grad_())
            return (leaf[0],)
        h = m.blocks[0].register_forward_pre_hook(pre)
    try:
        torch.manual_seed(seed)
        logits = m(x)
        loss = F.cross_entropy(logits, y)
        (loss * (scale or (HALF_SCALE if mode == "half" else 1.0))).backward()
    finally:
        if h is not None:
            h.remove()
    torch.cuda.synchronize()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}
    return logits.detach().clone(), loss.detach().clone(), grads, (leaf[0].grad.clone() if grab else None)


def assert_same_bits(on, off, m):
    (l1, s1, g1, i1), (l0, s0, g0, i0) = on, off
    assert torch.equal(l1, l0) and torch.equal(s1, s0)
    assert torch.equal(i1, i0) and float(i1.abs().sum()) > 0
    for k, p in m.named_parameters():
        if p.requires_grad:
            assert g1[k] is not None and torch.equal(g1[k], g0[k]), k
            assert bool(torch.isfinite(g1[k]).all()), k
        else:
            assert g1[k] is None and g0[k] is None, k
    assert any(float(g.abs().sum()) > 0 for g in g1.values() if g is not None)


# ------------------------------------------------------------------------------------------------- (a) bit identity
CASES_A = {
    "plain": dict(),
    "plain_hd80": dict(embed=320),
    "layer_scale": dict(init_values=0.1),
    "branch_dropout": dict(drop_rate=0.1),
    "layer_scale_dropout": dict(init_values=0.1, drop_rate=0.1),
    "checkpoint": dict(use_checkpoint=True),
    "pooled_tail_all_frozen": dict(freeze=DEPTH),
    "no_qkv_bias": dict(qkv_bias=False),
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(CASES_A))
def test_a_bit_identity(case, mode):
    kw = dict(freeze=2)
    kw.update(CASES_A[case])
    m = build(**kw)
    x, y = batch()
    if case == "pooled_tail_all_frozen":
        assert m.blocks[-1].pools_fused() and not m.blocks[-1].mlp.fc2.weight.requires_grad
    calls0 = ops._PoolStats.calls
    on = step(m, x, y, mode, True)
    off = step(m, x, y, mode, False)
    if case == "pooled_tail_all_frozen":
        assert ops._PoolStats.calls >= calls0 + 2
    assert_same_bits(on, off, m)


@pytest.mark.parametrize("mode", MODES)
def test_a_bit_identity_drop_path(mode):
    m = build(freeze=2, drop_path_rate=0.2)
    x, y = batch()
    dps = [b.drop_path for b in m.blocks if isinstance(b.drop_path, DropPath) and b.drop_path.drop_prob]
    seen = []
    orig = m._presample_drop_path

    def presample(batch_, device):
        orig(batch_, device)
        seen.append(torch.stack([s for d in dps for s in d.presampled]).cpu())
    m._presample_drop_path = presample
    # a seed whose draw drops at least one clip of one branch (the sampler alone is run to find it: one torch.rand per try)
    seed = None
    for s in range(64):
        torch.manual_seed(s)
        presample(B, x.device)
        for d in dps:
            d.presampled = None
        if bool((seen.pop() == 0).any()):
            seed = s
            break
    assert seed is not None
    on = step(m, x, y, mode, True, seed=seed)
    off = step(m, x, y, mode, False, seed=seed)
    assert len(seen) == 2 and torch.equal(seen[0], seen[1])
    assert bool((seen[0] == 0).any()) and bool((seen[0] > 1).any()), seen[0]  # a clip was dropped, and one was kept and rescaled
    assert_same_bits(on, off, m)


# ------------------------------------------------------------------------------------------------- (b) launch accounting
def with_sinks(m):
    """gradient sinks on the trainable parameters (what FusedAdamW installs): the qkv / pair launches run only into sinks"""
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    opt.zero_grad()
    return opt


def backward_calls(m, x, y, mode, skip, names=WGRAD, sinks=False):
    T.set_precision(mode)
    ops.set_skip_frozen(skip)
    opt = with_sinks(m) if sinks else None
    if opt is None:
        m.zero_grad(set_to_none=True)
    loss = F.cross_entropy(m(x), y)
    with counting(names) as calls:
        loss.backward()
        torch.cuda.synchronize()
    return calls


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sinks", [False, True])
@pytest.mark.parametrize("kw", [dict(), dict(init_values=0.1)], ids=["plain", "layer_scale"])
def test_b_launch_accounting(kw, sinks, mode):
    """the pooled tail is off here so that the three blocks launch alike and `share` is exact; its own frozen fc2 is covered by (a)"""
    ops.set_pooled_tail(False)
    x, y = batch()
    base = wgrad_counts(backward_calls(build(**kw), x, y, mode, True, sinks=sinks))
    assert base["patch"] == 1 and sum(base.values()) >= 1 + 3 * DEPTH
    if sinks and not kw:
        assert base["linear_bwd_weight_pair"] == DEPTH  # (the all-trainable block keeps its pair launch)
    problems = lambda c: sum(c.values()) + c["linear_bwd_weight_pair"] - c["layerscale_grads"]  # noqa: E731  (GEMM problems)
    for n in (1, 2, 3):
        on = wgrad_counts(backward_calls(build(freeze=n, **kw), x, y, mode, True, sinks=sinks))
        assert on["patch"] == 0 and on["patch_embed_bwd"] == 0
        for name in WGRAD:
            assert on[name] * DEPTH == base[name] * (DEPTH - n), (n, name, on, base)
        off = wgrad_counts(backward_calls(build(freeze=n, **kw), x, y, mode, False, sinks=sinks))
        # The switch-off path computes every gradient of every node autograd builds.  It builds none for the patch embedding, which
        # under the rule has no differentiable input at all (hence `patch` apart; see below for a node that exists).
        assert off["patch"] == 0
        off["patch"] = base["patch"]
        if not sinks:
            assert off == base, (n, off, base)
        # (a frozen parameter has no sink, so the switch-off path runs its gradients through the single launches: the same problems)
        assert problems(off) == problems(base) and off["layerscale_grads"] == base["layerscale_grads"], (n, off, base)
    # the patch projection frozen beside a trainable bias: the node exists, the switch-off path launches the weight gradient over
    # the patch matrix, the switch-on path takes the column sums alone
    for skip in (True, False):
        m = build(freeze=1, **kw)
        m.patch_embed.proj.bias.requires_grad = True
        calls = backward_calls(m, x, y, mode, skip, names=WGRAD + ("colsum_bf16",), sinks=sinks)
        assert wgrad_counts(calls)["patch"] == (0 if skip else 1)
        assert [n for n, _, _, _ in calls].count("colsum_bf16") == (1 if skip else 0)
        assert m.patch_embed.proj.bias.grad is not None and m.patch_embed.proj.weight.grad is None


# ------------------------------------------------------------------------------------------------- (c) saved bytes
def saved_bytes(m, x, y, mode, skip):
    T.set_precision(mode)
    ops.set_skip_frozen(skip)
    m.zero_grad(set_to_none=True)
    sizes = []

    def pack(t):
        sizes.append(t.numel() * t.element_size())
        return t
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        loss = F.cross_entropy(m(x), y)
    loss.backward()
    return sum(sizes)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("embed", [128, 320])
def test_c_saved_bytes(embed, mode):
    """Under the rule alone the patch embedding has no differentiable input, autograd builds no node for it and NEITHER path keeps the
    patch matrix; the bound with the patch matrix's bytes is therefore asserted with the projection's bias thawed by hand, where the
    switch-off path does keep it."""
    x, y = batch()
    D = embed
    per_block = M * (D + D + 4 * D) * 2
    cols = M * KPATCH * 2
    for n in (1, 2, 3):
        m = build(embed=embed, freeze=n)
        on, off = saved_bytes(m, x, y, mode, True), saved_bytes(m, x, y, mode, False)
        assert off - on >= n * per_block, (n, off, on)
        m.patch_embed.proj.bias.requires_grad = True
        on, off = saved_bytes(m, x, y, mode, True), saved_bytes(m, x, y, mode, False)
        assert off - on >= n * per_block + cols, (n, off, on)
    m = build(embed=embed)
    assert saved_bytes(m, x, y, mode, True) == saved_bytes(m, x, y, mode, False)


@pytest.mark.parametrize("mode", MODES)
def test_c_frozen_projection_takes_the_implicit_route(mode):
    """with the projection frozen the training forward may take the implicit GEMM, which writes no patch matrix (the threshold is
    lowered to this shape's one tile): same logits as the explicit route bit for bit, and the bias -- thawed by hand, so that the node
    has a backward at all -- gets its gradient from column sums, within the mode's bound of the fp64 oracle"""
    x, y = batch()
    m = build(freeze=1)
    m.patch_embed.proj.bias.requires_grad = True
    ref = fp64_grads(m, x, y)["patch_embed.proj.bias"]
    explicit = step(m, x, y, mode, True, grab=False)
    old = ops.IMPLICIT_PATCH_EMBED_MIN_TILES
    ops.IMPLICIT_PATCH_EMBED_MIN_TILES = 1
    try:
        with counting(("patch_embed_fwd_implicit", "patch_embed_fwd", "im2col_tubelets")) as calls:
            implicit = step(m, x, y, mode, True, grab=False)
        assert [n for n, _, _, _ in calls] == ["patch_embed_fwd_implicit"]
        with counting(("patch_embed_fwd_implicit", "patch_embed_fwd")) as calls:
            step(m, x, y, mode, False, grab=False)  # switch off: the explicit route, as before
        assert [n for n, _, _, _ in calls] == ["patch_embed_fwd"]
    finally:
        ops.IMPLICIT_PATCH_EMBED_MIN_TILES = old
    assert torch.equal(implicit[0], explicit[0]) and torch.equal(implicit[1], explicit[1])
    for k, g in explicit[2].items():
        assert (g is None) == (implicit[2][k] is None) and (g is None or torch.equal(g, implicit[2][k])), k
    s = HALF_SCALE if mode == "half" else 1.0
    e = whole_err(implicit[2]["patch_embed.proj.bias"] / s, ref)[0]
    print(f"\n{mode}: patch projection bias gradient from column sums vs fp64: rel-L2 {e:.2e}")
    assert e <= BOUND[mode], e


# ------------------------------------------------------------------------------------------------- (d) all trainable
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sinks", [False, True])
@pytest.mark.parametrize("kw", [dict(), dict(init_values=0.1, drop_rate=0.1), dict(drop_path_rate=0.2)], ids=["plain", "variant", "drop_path"])
def test_d_all_trainable_is_untouched(kw, sinks, mode):
    x, y = batch()
    runs = []
    for skip in (True, False):
        m = build(**kw)
        T.set_precision(mode)
        ops.set_skip_frozen(skip)
        opt = with_sinks(m) if sinks else None
        with counting() as calls:
            torch.manual_seed(3)
            logits = m(x)
            loss = F.cross_entropy(logits, y)
            (loss * (HALF_SCALE if mode == "half" else 1.0)).backward()
            torch.cuda.synchronize()
        runs.append((logits.detach(), loss.detach(), [p.grad.clone() for p in m.parameters()], [(n, s) for n, s, _, _ in calls]))
        del opt
    (l1, s1, g1, c1), (l0, s0, g0, c0) = runs
    assert c1 == c0 and len(c1) > 20
    assert torch.equal(l1, l0) and torch.equal(s1, s0)
    assert all(torch.equal(a, b) for a, b in zip(g1, g0))


# ------------------------------------------------------------------------------------------------- (e) training steps
def train(mode, skip, update_freq=1, parallel=False, steps=3):
    T.set_precision(mode)
    ops.set_skip_frozen(skip)
    m = build(freeze=2)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    model = DataParallel(m) if parallel else m
    opt = E.create_optimizer(model, lr=1e-3, weight_decay=0.05)
    assert isinstance(opt, FusedAdamW)
    scaler = E.NativeScalerWithGradNormCount(model, init_scale=HALF_SCALE)
    loader = [batch(seed=20 + i) for i in range(steps * update_freq)]
    torch.manual_seed(7)
    stats = E.train_one_epoch(model, torch.nn.CrossEntropyLoss(), loader, opt, torch.device("cuda"), 0, scaler, update_freq=update_freq)
    return m, before, opt, stats


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("how", ["plain", "update_freq_2", "data_parallel"])
def test_e_training_steps(how, mode):
    kw = dict(update_freq=2 if how == "update_freq_2" else 1, parallel=how == "data_parallel")
    m1, before, opt, st1 = train(mode, True, **kw)
    m0, _, _, st0 = train(mode, False, **kw)
    moved = 0
    for (k, p), (_, q) in zip(m1.named_parameters(), m0.named_parameters()):
        assert torch.equal(p, q), k
        if p.requires_grad:
            moved += not torch.equal(p, before[k])
        else:
            assert torch.equal(p, before[k]), k
    assert moved == sum(p.requires_grad for p in m1.parameters())
    assert st1 == st0 and all(v is not None for v in st1["grad_norm"][kw["update_freq"] - 1::kw["update_freq"]])
    held = [p for g in opt.param_groups for p in g["params"]]
    assert all(p.requires_grad for p in held) and len(held) == sum(p.requires_grad for p in m1.parameters())
    assert len(opt.state_dict()["state"]) == len(held)  # (state is keyed by position in the groups: no frozen parameter has one)


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    if hasattr(a, "shape"):
        import numpy as np
        return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    return a == b or (a != a and b != b)


@pytest.mark.parametrize("mode", MODES)
def test_e_engine_neighbours_with_a_frozen_model(mode):
    """ModelEma, GradNormCollector and validation_one_epoch around two training steps of a frozen model: no interface change, the same
    results with the switch on and off, and the evaluation afterwards reads the weights as they are (no stale operand copy)"""
    from simple_tad_amd.ema import ModelEma
    from simple_tad_amd.grad_norms import GradNormCollector
    dev = torch.device("cuda")
    loader = [(batch(seed=40 + i)[0], torch.tensor([0, 1, 1]).cuda()) for i in range(2)]
    T.set_precision(mode)
    runs = []
    for skip in (True, False):
        ops.set_skip_frozen(skip)
        m = build(freeze=2, num_classes=2)
        ema = ModelEma(m, decay=0.9)
        opt = E.create_optimizer(m, lr=1e-3, weight_decay=0.05)
        col = GradNormCollector(m, opt)
        scaler = E.NativeScalerWithGradNormCount(m, init_scale=HALF_SCALE)
        stats = E.train_one_epoch(m, torch.nn.CrossEntropyLoss(), loader, opt, dev, 0, scaler, model_ema=ema, grad_norms=col)
        val = E.validation_one_epoch(loader, m, dev)
        val_ema = E.validation_one_epoch(loader, ema.ema, dev)
        m.eval()
        with torch.no_grad():
            out = m(loader[0][0])
        f = build(freeze=2, num_classes=2)
        f.load_state_dict(m.state_dict())
        ops.invalidate_weight_cache()
        f.eval()
        with torch.no_grad():
            assert torch.equal(f(loader[0][0]), out)
        assert "grad_norms" in stats and all(not p.requires_grad for p in ema.ema.parameters())
        runs.append((stats, val[0], val[1], val_ema[0], val_ema[1], [p.detach().clone() for p in ema.ema.parameters()], out))
    assert same(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------- (f) linear probe
@pytest.mark.parametrize("mode", MODES)
def test_f_linear_probe(mode):
    m = build()
    for k, p in m.named_parameters():
        p.requires_grad = k.startswith(("fc_norm.", "head."))
    x, y = batch()
    T.set_precision(mode)
    sizes = []

    def pack(t):
        sizes.append(t.numel())
        return t
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        loss = F.cross_entropy(m(x), y)
    with counting() as calls:
        loss.backward()
        torch.cuda.synchronize()
    block_kernels = ("attn_bwd", "attn_bwd_f32", "linear_bwd_input", "meanpool_bwd", "gelu_grad_bcast") + WGRAD
    assert not [n for n, _, _, _ in calls if n in block_kernels], [n for n, _, _, _ in calls]
    assert [n for n, _, _, _ in calls].count("layernorm_bwd") == 1  # fc_norm's
    assert sizes and max(sizes) < M * 128  # nothing with a row per token: fc_norm's [B, D] input and statistics, the head's operands
    assert all(p.grad is not None for k, p in m.named_parameters() if k.startswith(("fc_norm.", "head.")))
    assert all(p.grad is None for k, p in m.named_parameters() if not k.startswith(("fc_norm.", "head.")))


# ------------------------------------------------------------------------------------------------- (g) mixed flags in one block
def fp64_grads(m, x, y):
    P = {k: v.detach().double().requires_grad_() for k, v in m.state_dict().items()}
    feats = O.forward_features(x.double(), P, depth=DEPTH, num_heads=2, tubelet=2, patch=16)
    F.cross_entropy(F.linear(feats, P["head.weight"], P["head.bias"]), y).backward()
    return {k: P[k].grad for k, _ in m.named_parameters()}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("frozen", ["attn.qkv.weight", "mlp.fc2.bias"])
def test_g_mixed_flags_in_one_block(frozen, mode):
    """one frozen tensor inside otherwise trainable blocks, gradient sinks installed: with qkv.weight frozen the proj gradient comes from
    the single launch (another summation order than the pair's), q_bias / v_bias from column sums alone; with fc2.bias frozen the fc2
    launch takes no column sums.  Whole tensors against the fp64 oracle on the device within test_grad_parity_gpu's bound of the mode."""
    m = build()
    for blk in m.blocks:
        dict(blk.named_parameters())[frozen].requires_grad = False
    x, y = batch()
    ref = fp64_grads(m, x, y)
    T.set_precision(mode)
    s = HALF_SCALE if mode == "half" else 1.0
    with_sinks(m)
    ops.set_pooled_tail(False)  # (every block through the same backward: the counts below are per block)
    loss = F.cross_entropy(m(x), y)
    with counting(WGRAD + ("colsum_bf16",)) as calls:
        (loss * s).backward()
        torch.cuda.synchronize()
    names = [n for n, _, _, _ in calls]
    assert names.count("linear_bwd_weight_pair") == 0 if frozen == "attn.qkv.weight" else names.count("linear_bwd_weight_pair") == DEPTH
    if frozen == "attn.qkv.weight":
        assert names.count("linear_bwd_weight_qkv") == 0 and names.count("colsum_bf16") == DEPTH
        assert names.count("linear_bwd_weight") == 3 * DEPTH + 1  # proj, fc1, fc2 per block and the patch projection
    else:
        fc2 = [k for n, _, a, k in calls if n == "linear_bwd_weight" and a[0].shape[1] == 128 and a[1].shape[1] == 512]
        assert len(fc2) == DEPTH and all(k.get("want_bias") is False for k in fc2)
    errs = {}
    for k, p in m.named_parameters():
        if not p.requires_grad:
            assert p.grad is None and k.endswith(frozen), k
            continue
        errs[k] = whole_err(p.grad / s, ref[k])[0]
    worst = max(errs, key=errs.get)
    print(f"\n{mode}, {frozen} frozen: {len(errs)} trainable gradients vs fp64, rel-L2 worst {errs[worst]:.2e} ({worst})")
    over = {k: v for k, v in errs.items() if not v <= BOUND[mode]}
    assert not over, (mode, BOUND[mode], over)


# ------------------------------------------------------------------------------------------------- (h) operand copies
def weight_casts(m, calls):
    """per weight name: [casts, transpose-casts] among the recorded launches (a copy is made from the f32 master itself)"""
    by_ptr = {p.data_ptr(): k for k, p in m.named_parameters() if p.dim() >= 2}
    out = {k: [0, 0] for k in by_ptr.values()}
    for n, _, a, _ in calls:
        k = by_ptr.get(a[0].data_ptr())
        if k is not None and a[0].numel() == dict(m.named_parameters())[k].numel():
            out[k][n == "transpose_cast_bf16"] += 1
    return out


@pytest.mark.parametrize("mode", MODES)
def test_h_static_operand_copies(mode):
    T.set_precision(mode)
    counts = {}
    for skip in (True, False):
        ops.set_skip_frozen(skip)
        ops.invalidate_weight_cache()
        m = build(freeze=2)
        opt = E.create_optimizer(m, lr=1e-3, weight_decay=0.05)
        scaler = E.NativeScalerWithGradNormCount(m, init_scale=HALF_SCALE)
        loader = [batch(seed=30 + i) for i in range(3)]
        with counting(("cast_bf16", "transpose_cast_bf16")) as calls:
            E.train_one_epoch(m, torch.nn.CrossEntropyLoss(), loader, opt, torch.device("cuda"), 0, scaler)
        counts[skip] = weight_casts(m, calls)
    for k, p in m.named_parameters():
        if p.dim() < 2:
            continue
        if p.requires_grad:
            assert counts[True][k] == counts[False][k], k  # as before (the optimizer's mirrors serve them: no cast at all)
        elif k.startswith("patch_embed."):
            assert counts[True][k] == [1, 0] and counts[False][k] == [3, 0], (k, counts[True][k], counts[False][k])
        else:
            assert counts[True][k] == [1, 1] and counts[False][k] == [3, 3], (k, counts[True][k], counts[False][k])


@pytest.mark.parametrize("mode", MODES)
def test_h_changed_frozen_weight_is_seen(mode):
    T.set_precision(mode)
    m = build(freeze=2)
    x, y = batch()

    def logits_of(model):
        out = model(x)
        F.cross_entropy(out, y).backward()  # (a differentiated forward: the static copies are the ones in use)
        return out.detach().clone()

    def fresh():
        f = build(freeze=2)
        f.load_state_dict(m.state_dict())
        ops.invalidate_weight_cache()
        return logits_of(f)

    first = logits_of(m)
    assert torch.equal(logits_of(m), first)
    # a write that autograd sees (the version counter moves): nothing else is needed
    w = m.blocks[0].mlp.fc1.weight
    with torch.no_grad():
        w.copy_(w * 1.5)
    second = logits_of(m)
    assert not torch.equal(second, first)
    # a write through .data moves no version counter: invalidate_weight_cache() is the documented call after it
    w = m.blocks[1].attn.qkv.weight
    w.data.copy_(w.data * 0.5)
    ops.invalidate_weight_cache()
    third = logits_of(m)
    assert not torch.equal(third, second)
    assert torch.equal(third, fresh())
    w = m.blocks[0].mlp.fc1.weight
    with torch.no_grad():
        w.copy_(w / 1.5)
    fourth = logits_of(m)
    assert not torch.equal(fourth, third) and torch.equal(fourth, fresh())
