"""Stochastic depth: the attention kernels FILL the clips whose branch scale is 0 instead of computing them (the clip_scale argument of
tad_attn_fwd / tad_attn_bwd; csrc/attn_fwd.hip / attn_bwd.hip: SKIP).  The knob tad_attn_tuning("drop_skip", 0) computes every clip as before; every test here
compares the two BIT FOR BIT on what the training step consumes -- the fill is not allowed to change a single bit of the residual
stream, of dqkv, or of any gradient.

What differs on purpose, and is never consumed un-multiplied: the attention output of a dropped clip (zeros instead of values that the
residual epilogue multiplies by 0) and its lse (a finite placeholder)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import simple_tad_amd as T
from guarded import GuardedArena, same_bits
from simple_tad_amd import _lib, ops
from simple_tad_amd.modeling_finetune import Block, DropPath

pytestmark = pytest.mark.gpu

FMTS = {"bf16": torch.bfloat16, "f16": torch.float16}
N_REAL = 1568  # tokens per clip of the benchmarked step: 12.25 query blocks of 128, so workgroups end inside a clip's last block
# B = 3 .. 5 at the real sequence length, and the ragged sequence lengths of tests/test_guarded_gpu.py's attention list (ATT) that
# a batch of several clips can carry (N = 8: one partly filled wave; N = 129: one row in the second query block)
SHAPES = [(3, N_REAL, 2), (4, N_REAL, 1), (5, N_REAL, 1), (3, 8, 1), (4, 129, 2)]


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import kernels
    _lib.load()
    return kernels


@pytest.fixture(scope="module")
def arena():
    return GuardedArena(768 << 20, "cuda")


@pytest.fixture
def knob(K):
    """knob(v): tad_attn_tuning(drop_skip=v); the value found is restored afterwards"""
    found = K.attn_tuning_get("drop_skip")
    yield lambda v: K.attn_tuning(drop_skip=v)
    K.attn_tuning(drop_skip=found)


def patterns(B):
    """dropped clips: the first, the last, two adjacent ones, all, none"""
    return {"first": [0], "last": [B - 1], "adjacent": [B // 2 - 1, B // 2] if B > 3 else [1, 2], "all": list(range(B)), "none": []}


def scale_of(B, dropped, keep=0.9):
    s = torch.full((B,), 1.0 / keep, dtype=torch.float32)
    s[dropped] = 0.0
    return s.cuda()


# ================================================================================================ 1. the wrappers
@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("B,N,H", SHAPES)
def test_attention_fill_is_bit_identical_to_compute(K, knob, B, N, H, fmt):
    """K.attn_fwd / K.attn_bwd with a drop scale, knob on against knob off, followed by the Linears that consume their results in the
    training step: the residual stream behind the proj Linear, dqkv, and the proj weight gradient (dy^T ao: the one product that reads
    the filled attention output in the backward) are bit-identical; the rows of kept clips of out / out_lo / lse as well."""
    op, d, D = FMTS[fmt], 64, 64 * H
    g = torch.Generator().manual_seed(B * 10000 + N * 10 + H)
    qkv = (torch.randn(B * N, 3 * D, generator=g) * 0.7).to(op).cuda()
    x0 = torch.randn(B * N, D, generator=g).cuda()
    gres = torch.randn(B * N, D, generator=g).cuda()             # gradient of the residual stream behind the branch
    wp = (torch.randn(D, D, generator=g) * D ** -0.5).to(op).cuda()
    bp = torch.randn(D, generator=g).cuda()
    scale = d ** -0.5
    for name, dropped in patterns(B).items():
        rs = scale_of(B, dropped)
        # what the LayerNorm backward / tad_scale_cast hand the branch: rowscale * gradient, exact (signed) zeros in the dropped clips
        dy = K.scale_cast_op16(gres, None, rs, N, dtype=op)
        d_ao = K.linear_bwd_input(dy, wp.t().contiguous())
        res = {}
        for on in (1, 0):
            knob(on)
            # the records about to run: the fill kernels (SKIP) with the knob on, the general ones with it off
            assert [r["skip"] for r in K.attn_plan(B, N, H, q_prescaled=True, rowscale=True, out_lo=True)] == [on]
            assert [r["skip"] for r in K.attn_plan(B, N, H, q_prescaled=True, rowscale=True, out_lo=True, backward=True)] == [on, on]
            out, lse, lo = K.attn_fwd(qkv, B, N, H, scale, want_lo=True, q_prescaled=True, rowscale=rs)
            x1, _ = K.linear_fwd(out, wp, bp, out_dtype=torch.float32, epilogue=_lib.EPI_BIAS_RESIDUAL, residual=x0, rowscale=rs, rows_per_scale=N)
            dqkv = K.attn_bwd(qkv, out, d_ao, lse, B, N, H, scale, out_lo=lo, q_prescaled=True, rowscale=rs)
            dwp, _ = K.linear_bwd_weight(dy, out, want_bias=False)
            res[on] = dict(out=out, lse=lse, lo=lo, x1=x1, dqkv=dqkv, dwp=dwp)
        torch.cuda.synchronize()
        a, b = res[1], res[0]
        for k in ("x1", "dqkv", "dwp"):
            assert bool(torch.isfinite(a[k].float()).all()), (name, k)
            assert same_bits(a[k], b[k]), f"{name}: {k} differs in bits between fill and compute"
        kept = [i for i in range(B) if i not in dropped]
        for k, rows in (("out", lambda t: t.reshape(B, N, -1)), ("lo", lambda t: t.reshape(B, N, -1)), ("lse", lambda t: t)):
            assert same_bits(rows(a[k])[kept], rows(b[k])[kept]), f"{name}: {k} of the kept clips"
        if dropped:  # the path was taken: zeros where the computation leaves values, a finite lse
            assert not bool(a["out"].reshape(B, N, -1)[dropped].any()) and not bool(a["lo"].reshape(B, N, -1)[dropped].any())
            assert bool(b["out"].reshape(B, N, -1)[dropped].any())
            assert bool(torch.isfinite(a["lse"][dropped]).all())
            assert not bool(a["dqkv"].reshape(B, N, -1)[dropped].any())


def test_a_forward_fill_met_by_a_computing_backward_stays_finite(K, knob):
    """the knob may change between a forward and its backward: the placeholder lse of a filled clip makes a computing backward see
    P = 0 there (never exp(score - lse) = inf times a zero gradient), so dqkv is still what the all-compute run gives"""
    B, N, H = 3, 393, 1
    g = torch.Generator().manual_seed(5)
    qkv = (torch.randn(B * N, 192, generator=g) * 3.0).to(torch.bfloat16).cuda()  # (scores of tens of log2 units)
    rs = scale_of(B, [1])
    dy = K.scale_cast_op16(torch.randn(B * N, 64, generator=g).cuda(), None, rs, N, dtype=torch.bfloat16)
    knob(0)
    out0, lse0, lo0 = K.attn_fwd(qkv, B, N, H, 0.125, want_lo=True, q_prescaled=True, rowscale=rs)
    ref = K.attn_bwd(qkv, out0, dy, lse0, B, N, H, 0.125, out_lo=lo0, q_prescaled=True, rowscale=rs)
    knob(1)
    out, lse, lo = K.attn_fwd(qkv, B, N, H, 0.125, want_lo=True, q_prescaled=True, rowscale=rs)
    knob(0)
    got = K.attn_bwd(qkv, out, dy, lse, B, N, H, 0.125, out_lo=lo, q_prescaled=True, rowscale=rs)
    assert bool(torch.isfinite(got.float()).all()) and same_bits(got, ref)


# ================================================================================================ 2. + 4. one block, NaN trap, guard bands
def make_block(D, H, seed):
    torch.manual_seed(seed)
    blk = Block(D, H, mlp_ratio=4, qkv_bias=True, init_values=0, drop_path=0.5, norm_layer=lambda n: torch.nn.LayerNorm(n, eps=1e-6))
    for p in blk.parameters():
        if p.dim() == 1:
            torch.nn.init.normal_(p, std=0.2)
    return blk.cuda().train()


@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("mode", ["fast", "half"])
@pytest.mark.parametrize("B,N", [(3, N_REAL), (4, 129), (3, 8)])
def test_block_with_every_buffer_prefilled_with_nan(K, knob, arena, B, N, mode, poison):
    """One fused Block forward + backward with dropped clips in both branches, every output, saved activation and workspace the
    wrappers allocate pre-filled with NaN (or the largest finite value) inside a guarded arena: all gradients are finite and
    bit-identical to the knob-off run -- a fill that left stale memory behind a zero factor would show as NaN here -- and no store
    of the fill leaves its operand (the arena's guard bands are unchanged)."""
    D, H = 128, 2
    blk = make_block(D, H, seed=B * 100 + N)
    g = torch.Generator().manual_seed(N)
    x = torch.randn(B, N, D, generator=g).cuda()
    gy = torch.randn(B, N, D, generator=g).cuda()
    dp1, dp2 = scale_of(B, [0, B - 1], keep=0.5), scale_of(B, [1], keep=0.5)
    T.set_precision(mode)
    runs = {}
    try:
        for on in (1, 0):
            knob(on)
            arena.reset(poison)
            xin = x.clone().requires_grad_()
            blk.zero_grad(set_to_none=True)
            blk.drop_path.presampled = [dp1.clone(), dp2.clone()]
            with arena.route(K):
                y = blk(xin)
                y.backward(gy)
            arena.verify()
            runs[on] = dict(y=y.detach().clone(), dx=xin.grad.clone(), **{k: p.grad.clone() for k, p in blk.named_parameters()})
    finally:
        T.set_precision("fast")
    assert len(runs[1]) == 2 + len(list(blk.parameters()))
    for k, v in runs[1].items():
        assert bool(torch.isfinite(v).all()), f"{k} is not finite"
        assert same_bits(v, runs[0][k]), f"{k} differs in bits between fill and compute"


# ================================================================================================ 3. the model
def vitb_with_masks(B, seed=0):
    """ViT-B/16 16 x 224 x 224 at drop-path rate 0.2 with a fixed mask pattern: every block's two branch scales are presampled from a
    seeded generator at drop probability 0.3 (so that most blocks drop somebody, some two neighbours), the same in every step"""
    torch.manual_seed(seed)
    m = T.create_model("vit_base_patch16_224", pretrained=False, num_classes=2, all_frames=16, tubelet_size=2, final_reduction="fc_norm",
                       use_flash_attn=False, init_scale=1.0, drop_path_rate=0.2)
    m = m.cuda().train()
    g = torch.Generator().manual_seed(1234)
    scales = {}
    for i, blk in enumerate(m.blocks):
        if isinstance(blk.drop_path, DropPath) and blk.drop_path.drop_prob:
            keep = torch.tensor(1.0 - blk.drop_path.drop_prob, dtype=torch.float32)
            scales[i] = [((torch.rand(B, generator=g) >= 0.3).float() / keep).cuda() for _ in range(2)]
    assert sum(int((s == 0).sum()) for v in scales.values() for s in v) >= 8

    def presample(batch, device):
        for i, s in scales.items():
            m.blocks[i].drop_path.presampled = [s[0].clone(), s[1].clone()]
    m._presample_drop_path = presample
    return m


def test_three_optimizer_steps_of_vitb(K, knob):
    """three AdamW steps of ViT-B at drop path 0.2 with a fixed mask pattern, knob on against knob off: loss and logits of every step
    and a seeded sample of the updated parameters are bit-identical; a step raises nothing under the sync debug mode (the masks are
    read on the device only)"""
    from simple_tad_amd.optim import FusedAdamW
    B = 4
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, 3, 16, 224, 224, generator=g).cuda()
    y = torch.tensor([0, 1, 1, 0]).cuda()
    runs = {}
    for on in (1, 0):
        knob(on)
        m = vitb_with_masks(B)
        opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.05)
        trace = []
        for step in range(3):
            opt.zero_grad()
            if on and step == 2:
                torch.cuda.synchronize()
                torch.cuda.set_sync_debug_mode("error")
            try:
                logits = m(x)
                loss = F.cross_entropy(logits, y)
                loss.backward()
            finally:
                torch.cuda.set_sync_debug_mode("default")
            opt.step()
            trace += [loss.detach().clone(), logits.detach().clone()]
        rng = np.random.RandomState(11)
        for k, p in m.named_parameters():
            flat = p.detach().flatten()
            idx = torch.from_numpy(rng.randint(0, flat.numel(), size=min(4096, flat.numel()))).cuda()
            trace.append(flat[idx].clone())
        runs[on] = trace
        del m, opt
    assert len(runs[1]) == len(runs[0])
    for i, (a, b) in enumerate(zip(runs[1], runs[0])):
        assert bool(torch.isfinite(a).all()), i
        assert same_bits(a, b), f"trace entry {i} (loss / logits per step, then parameter samples) differs between fill and compute"
