"""The InternVideo2 family on the GPU against the reference's recorded fp64 results (tests/golden/g26_internvideo2.npz; the full fp64
tensors come from the restatement of tests/iv2_recipe.py, which tests/test_iv2_cpu.py holds to the recorded values).

Yardstick: the same restatement run on the device under ``torch.autocast`` with the mode's 16-bit dtype -- what the reference computes
when it trains.  Per tensor (logits, every parameter's gradient, whole-tensor rel-L2 against fp64): ours <= 2 x the restatement's.  The
factor 2: at 9 tokens and 2 clips both deviations are sums of a few roundings and scatter from tensor to tensor.
"""
from collections import OrderedDict
from functools import partial

import pytest
import torch
import torch.nn.functional as F

import iv2_recipe as R
import simple_tad_amd as T
from simple_tad_amd import engine as E, internvideo2 as IV2, ops
from simple_tad_amd._lib import TadError
from simple_tad_amd.optim import FusedAdamW

pytestmark = pytest.mark.gpu

MODES = {"fast": torch.bfloat16, "half": torch.float16}
HALF_SCALE = 4096.0  # the loss scale of the half-mode tests (tests/test_grad_parity_gpu.py)
FACTOR = 2.0


@pytest.fixture(autouse=True)
def _restore_switches():
    yield
    ops.set_iv2_kernels(True)
    ops.set_attn_q_prescale(True)
    ops.set_skip_frozen(True)
    T.set_precision("fast")
    ops.invalidate_weight_cache()


def rel(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def build(**over):
    torch.manual_seed(0)
    m = IV2.InternVideo2(**dict(R.TINY, **R.REF_ROUTE, **over))
    R.perturb_(m.named_parameters())
    return m.cuda()


def build_block():
    torch.manual_seed(0)
    blk = IV2.Block(norm_layer=partial(IV2.RMSNorm, eps=1e-6), **R.BLOCK)
    R.perturb_(blk.named_parameters())
    return blk.cuda()


_REF = {}


def model_reference():
    """fp64 (logits, loss, grads) of fixture (b) from the restatement on the device: computed once, never changed"""
    if "model" not in _REF:
        m = build()
        out = R.model_loss_and_grads(R.leaves(m.named_parameters(), dtype=torch.float64), R.clip().cuda().double(), R.TINY)
        assert R.matches(out[0], R.load()["b/logits"], 0) <= R.REPRO_TOL, "the restatement on the device is the recorded reference"
        _REF["model"] = {"fp64": out}
    return _REF["model"]


def ours_model(m, mode, x=None):
    T.set_precision(mode)
    m.zero_grad(set_to_none=True)
    x = R.clip().cuda() if x is None else x
    logits = m(x)
    loss = F.cross_entropy(logits, torch.tensor(R.LABELS).cuda())
    s = HALF_SCALE if mode == "half" else 1.0
    (loss * s).backward()
    return logits.detach(), loss.detach(), OrderedDict((k, None if p.grad is None else p.grad / s) for k, p in m.named_parameters())


def compare(ours, yard, ref, what):
    worse = {}
    for k in ref:
        eo, ey = rel(ours[k], ref[k]), rel(yard[k], ref[k])
        print(f"{what} {k}: ours {eo:.3e}  restatement under autocast {ey:.3e}")
        if ref[k].numel() <= 4:  # (logits, head.bias: the values themselves)
            print(f"    fp64 {ref[k].flatten().tolist()}\n    ours {ours[k].flatten().tolist()}\n    autocast {yard[k].flatten().tolist()}")
        if eo > FACTOR * ey:
            worse[k] = (eo, ey)
    assert not worse, f"{what}: ours worse than {FACTOR} x the autocast restatement: {worse}"


def autocast_model(m, mode):
    """the yardstick of a mode: the restatement under autocast, loss scaled in half mode"""
    dt, s = MODES[mode], (HALF_SCALE if mode == "half" else 1.0)
    P = R.leaves(m.named_parameters())
    x = R.clip().cuda()
    labels = torch.tensor(R.LABELS).cuda()
    with torch.autocast(device_type="cuda", dtype=dt):
        logits = R.model(P, x, R.TINY)
    loss = F.cross_entropy(logits.float(), labels)
    grads = torch.autograd.grad(loss * s, list(P.values()))
    return logits.detach().float(), loss.detach(), OrderedDict((k, g / s) for k, g in zip(P, grads))


@pytest.mark.parametrize("kernels", [True, False])
@pytest.mark.parametrize("mode", list(MODES))
def test_model_fixture_against_the_autocast_yardstick(mode, kernels):
    """Measured on an MI355X (ours / the restatement under autocast, whole-tensor rel-L2 against fp64), kernels on and off alike:
      fast: logits 2.64e-3 / 1.04e-2; the gradient tensors 5.7e-4 .. 9.3e-3 / 4.0e-4 .. 1.6e-2; worst ratio 1.43 (head.bias 5.75e-4 / 4.02e-4)
      half: logits 3.8e-4 / 1.07e-3; worst ratio 0.88 (blocks.1.attn.q_norm.weight).
    head.bias' gradient is ONE number g (the tensor is (g, -g): two classes), a function of the per-clip logit differences alone, and the
    restatement's value is a bf16 number that lies 0.04 % from fp64's: the tightest row of the table.  With 16-bit operands in the pooling
    head ours was 6.02e-3 there and failed; the head's Linears run on split operands since (ops.LinearSplitFn).
    clip_projector.norm1_k.bias and cross_attn.k_bias have an exactly zero gradient (a bias on every key shifts all scores of a softmax
    row alike), the fp64 tensors hold 1e-18-sized residue, and the "relative" figures are 1e9 .. 1e13-sized: for those two the comparison is
    one of absolute rounding noise, ours against the restatement's, over the same divisor."""
    m = build()
    ref_logits, ref_loss, ref_grads = model_reference()["fp64"]
    y_logits, _, y_grads = autocast_model(m, mode)
    ops.set_iv2_kernels(kernels)
    logits, loss, grads = ours_model(m, mode)
    assert all(g is not None and torch.isfinite(g).all() for g in grads.values())
    assert set(grads) == set(ref_grads) and "cls_token" in grads and "pos_embed" in grads
    compare({"logits": logits, **grads}, {"logits": y_logits, **y_grads}, {"logits": ref_logits, **ref_grads}, f"model {mode} kernels={kernels}")


@pytest.mark.parametrize("mode", list(MODES))
def test_block_fixture_against_the_autocast_yardstick(mode):
    blk = build_block()
    x, dy = (t.cuda() for t in R.block_input())
    s = HALF_SCALE if mode == "half" else 1.0
    y64, dx64, g64 = R.block_loss_and_grads(R.leaves(blk.named_parameters(), dtype=torch.float64), x.double(), dy.double())
    G = R.load()
    assert R.matches(y64, G["c/y"], 0) <= R.REPRO_TOL and R.matches(dx64, G["c/dx"], 0) <= R.REPRO_TOL
    ya, dxa, ga = R.block_loss_and_grads(R.leaves(blk.named_parameters()), x, dy * s, autocast=MODES[mode])
    T.set_precision(mode)
    xo = x.clone().requires_grad_()
    y = blk(xo)
    (y * dy * s).sum().backward()
    ours = {"y": y.detach(), "dx": xo.grad / s, **{k: p.grad / s for k, p in blk.named_parameters()}}
    yard = {"y": ya.float(), "dx": dxa / s, **{k: g / s for k, g in ga.items()}}
    compare(ours, yard, {"y": y64, "dx": dx64, **g64}, f"block {mode}")


@pytest.mark.parametrize("prescale", [True, False])
def test_both_q_contracts_give_the_model_fixture(prescale):
    """plain q and pre-scaled q (the factor scale * log2(e) applied by the normalisation kernel) are the same model"""
    m = build()
    ref_logits, _, ref_grads = model_reference()["fp64"]
    y_logits, _, y_grads = autocast_model(m, "fast")
    ops.set_attn_q_prescale(prescale)
    logits, _, grads = ours_model(m, "fast")
    keys = ["blocks.0.attn.q_norm.weight", "blocks.1.attn.q_norm.weight", "blocks.0.attn.qkv.weight", "blocks.0.norm1.weight"]
    compare({"logits": logits, **{k: grads[k] for k in keys}}, {"logits": y_logits, **{k: y_grads[k] for k in keys}},
            {"logits": ref_logits, **{k: ref_grads[k] for k in keys}}, f"prescale={prescale}")


@pytest.mark.parametrize("name", list(R.VARIANTS))
@pytest.mark.parametrize("mode", list(MODES))
def test_variants_forward(name, mode):
    over = R.VARIANTS[name]
    m = build(**over).eval()
    G = R.load()
    ref = torch.as_tensor(G[f"d/{name}/logits"]).cuda()
    x = R.clip().cuda()
    P = OrderedDict((k, v.detach()) for k, v in m.named_parameters())
    with torch.no_grad():
        with torch.autocast(device_type="cuda", dtype=MODES[mode]):
            yard = R.model(P, x, dict(R.TINY, **over)).float()
        T.set_precision(mode)
        ours = m(x)
    eo, ey = rel(ours, ref), rel(yard, ref)
    print(f"{name} {mode}: ours {eo:.3e}  restatement under autocast {ey:.3e}")
    assert eo <= FACTOR * ey


def test_frozen_block_gets_no_gradient_and_changes_nothing_else():
    m = build()
    _, _, full = ours_model(m, "fast")
    full = {k: v.clone() for k, v in full.items()}
    for p in m.blocks[0].parameters():
        p.requires_grad_(False)
    _, _, part = ours_model(m, "fast")
    for k, g in part.items():
        if k.startswith("blocks.0."):
            assert g is None, k
        else:
            assert torch.equal(g, full[k]), f"{k} changed when block 0 was frozen"


def test_checkpointed_block_gives_the_same_gradients_bit_for_bit():
    plain, ckpt = build(), build(use_checkpoint=True, checkpoint_num=1)
    assert ckpt.blocks[0].with_cp and not ckpt.blocks[1].with_cp
    l0, _, g0 = ours_model(plain, "fast")
    l1, _, g1 = ours_model(ckpt, "fast")
    assert torch.equal(l0, l1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_three_training_steps_move_every_tensor():
    T.set_precision("half")
    torch.manual_seed(0)
    m = IV2.InternVideo2(**dict(R.TINY, **R.REF_ROUTE, drop_path_rate=0.2, head_drop_path_rate=0.1)).cuda()
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    opt = E.create_optimizer(m, lr=1e-3, weight_decay=0.05, layer_decay=0.6)
    assert isinstance(opt, FusedAdamW) and len(opt.param_groups) == 2 * (m.get_num_layers() + 2)
    scaler = E.NativeScalerWithGradNormCount(m, init_scale=HALF_SCALE)
    g = torch.Generator().manual_seed(9)
    loader = [(torch.randn(2, 3, 2, 28, 28, generator=g).cuda(), torch.tensor([i % 2, 1]).cuda()) for i in range(3)]
    torch.manual_seed(7)
    stats = E.train_one_epoch(m, torch.nn.CrossEntropyLoss(), loader, opt, torch.device("cuda"), 0, scaler)
    assert len(stats["loss"]) == 3 and all(torch.isfinite(torch.tensor(v)) for v in stats["loss"])
    still = [k for k, p in m.named_parameters() if torch.equal(p.detach(), before[k])]
    assert not still, f"tensors that did not move in three steps: {still}"
    assert all(torch.isfinite(p).all() for p in m.parameters())


def test_real_size_small_model_forward_backward():
    torch.manual_seed(0)
    m = T.create_model("internvideo2_small_patch14_224", num_classes=2).cuda()
    seen = []
    orig = ops.K.attn_fwd

    def spy(qkv, B, N, H, *a, **k):
        seen.append((B, N, H))
        return orig(qkv, B, N, H, *a, **k)
    ops.K.attn_fwd = spy
    try:
        x = torch.randn(2, 3, 8, 224, 224, generator=torch.Generator().manual_seed(1)).cuda()
        logits = m(x)
        F.cross_entropy(logits, torch.tensor([0, 1]).cuda()).backward()
    finally:
        ops.K.attn_fwd = orig
    assert seen == [(2, 2049, 6)] * 12
    assert logits.shape == (2, 2) and torch.isfinite(logits).all()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k


def test_head_dims_without_a_kernel_refuse_to_run():
    blk = IV2.Block(176, 2, norm_layer=partial(IV2.RMSNorm, eps=1e-6), qk_normalization=True, init_values=0.1).cuda()  # head_dim 88, as the 1B model
    with pytest.raises(TadError, match="head_dim 88 has no kernel"):
        blk(torch.randn(1, 4, 176).cuda())


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("rows", [2, 18])
def test_split_operand_linear_is_f32_accurate_in_every_mode(mode, rows):
    """ops.LinearSplitFn (the pooling head's Linears) against fp64, forward and backward, per element.  Each operand is hi + lo of bf16: 16
    significant bits, 2^-17 relative each, so a product errs by 2^-16 of |a||b| to first order; accumulation in f32 over n terms adds at
    most n 2^-24.  Bound per element: (2^-15 + n 2^-24) sum |a||b| -- twice the first-order operand term."""
    T.set_precision(mode)
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, 128, generator=g).cuda().requires_grad_()
    w = (0.1 * torch.randn(64, 128, generator=g)).cuda().requires_grad_()
    b = torch.randn(64, generator=g).cuda().requires_grad_()
    dy = torch.randn(rows, 64, generator=g).cuda()
    y = ops.LinearSplitFn.apply(x, w, b)
    y.backward(dy)
    x64, w64, dy64 = x.detach().double(), w.detach().double(), dy.double()

    def within(got, ref, mag, n, what):
        lim = (2.0 ** -15 + n * 2.0 ** -24) * mag + 2.0 ** -23 * ref.abs()
        err = (got.double() - ref).abs()
        print(f"{what} {mode} rows {rows}: worst error / bound {(err / lim).max():.3f}")
        assert (err <= lim).all(), what

    within(y.detach(), x64 @ w64.t() + b.detach().double(), x64.abs() @ w64.abs().t(), 128, "y")
    within(x.grad, dy64 @ w64, dy64.abs() @ w64.abs(), 64, "dx")
    within(w.grad, dy64.t() @ x64, dy64.abs().t() @ x64.abs(), rows, "dW")
    within(b.grad, dy64.sum(0), dy64.abs().sum(0), rows, "db")
    # a frozen weight gets no gradient; the rest is unchanged bit for bit
    x2, w2 = x.detach().clone().requires_grad_(), w.detach().clone()
    b2 = b.detach().clone().requires_grad_()
    ops.LinearSplitFn.apply(x2, w2, b2).backward(dy)
    assert w2.grad is None and torch.equal(x2.grad, x.grad) and torch.equal(b2.grad, b.grad)
