"""InternVideo2 MAE pre-training on the GPU against the reference's recorded fp64 results (tests/golden/g27_iv2_pretrain.npz; the full fp64
tensors come from the restatement of tests/iv2_pretrain_recipe.py, run on the host and held there to every recorded value -- prediction,
loss and all 44 gradients -- within REPRO_TOL before they are used).

Yardstick, as in tests/test_iv2_gpu.py: the same restatement run on the device under ``torch.autocast`` with the mode's 16-bit dtype.
Per tensor (the prediction, every parameter's gradient; whole-tensor rel-L2 against fp64): ours <= 2 x the restatement's."""
from collections import OrderedDict
from functools import partial

import pytest
import torch
import torch.nn as nn

import iv2_pretrain_recipe as PR
import iv2_recipe as R
import simple_tad_amd as T
from simple_tad_amd import engine as E, engine_pretrain as EP, internvideo2_pretrain as IVP, kernels as K, ops
from simple_tad_amd.optim import FusedAdamW

pytestmark = pytest.mark.gpu

MODES = {"fast": torch.bfloat16, "half": torch.float16}
HALF_SCALE = 4096.0  # the loss scale of the half-mode tests (tests/test_iv2_gpu.py)
FACTOR = 2.0


@pytest.fixture(autouse=True)
def _restore_switches():
    yield
    ops.set_visible_token_kernels(True)
    ops.set_iv2_kernels(True)
    ops.set_skip_frozen(True)
    T.set_precision("fast")
    ops.invalidate_weight_cache()


def rel(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def build(**over):
    torch.manual_seed(0)
    m = IVP.PretrainVideoMAEInternVideo2(norm_layer=partial(nn.LayerNorm, eps=1e-6), **dict(PR.TINY, **over))
    R.perturb_(m.named_parameters())
    return m.cuda()


_REF = {}


def model_reference():
    """fp64 (prediction, loss, grads) of fixture (b) on the device: computed once, never changed.  The restatement runs in fp64 ON THE
    HOST, where its arithmetic is the recording's own -- the reference's RMSNorm computes in float32 inside the fp64 run, and a device's
    float32 mean and rsqrt are not the host's to the last bit -- and the prediction, the loss and EVERY gradient must reproduce the
    recorded values within REPRO_TOL before the tensors move to the device and serve as the reference."""
    if "model" not in _REF:
        m = build()
        P = R.leaves(m.named_parameters(), dtype=torch.float64, device="cpu")
        out, loss, grads = PR.model_loss_and_grads(P, PR.clip().double(), PR.mask(), PR.target().double(), PR.TINY)
        G = PR.load()
        assert R.matches(out, G["b/output"], 1000) <= PR.REPRO_TOL, "the restatement is the recorded reference"
        assert abs(float(loss) - float(G["b/loss"])) <= PR.REPRO_TOL * float(G["b/loss"])
        assert len(grads) == 44
        off = {k: d for i, (k, g) in enumerate(grads.items()) if (d := R.matches(g, G["b/grad/" + k], i)) > PR.REPRO_TOL}
        assert not off, f"gradients of the restatement that deviate from the recorded ones by more than {PR.REPRO_TOL}: {off}"
        _REF["model"] = (out.cuda(), loss.cuda(), OrderedDict((k, g.cuda()) for k, g in grads.items()))
    return _REF["model"]


def ours_model(m, mode):
    T.set_precision(mode)
    m.zero_grad(set_to_none=True)
    out = m(PR.clip().cuda(), PR.mask().cuda(), num_masked=PR.N - PR.NV)
    loss = ops.MseLossFn.apply(out, PR.target().cuda())
    s = HALF_SCALE if mode == "half" else 1.0
    (loss * s).backward()
    return out.detach(), loss.detach(), OrderedDict((k, None if p.grad is None else p.grad / s) for k, p in m.named_parameters())


def autocast_model(m, mode):
    """the yardstick of a mode: the restatement under autocast, loss scaled in half mode"""
    s = HALF_SCALE if mode == "half" else 1.0
    out, loss, grads = PR.model_loss_and_grads(R.leaves(m.named_parameters()), PR.clip().cuda(), PR.mask().cuda(), PR.target().cuda(), PR.TINY,
                                               autocast=MODES[mode], scale=s)
    return out.float(), loss, OrderedDict((k, g / s) for k, g in grads.items())


def compare(ours, yard, ref, what):
    worse = {}
    for k in ref:
        eo, ey = rel(ours[k], ref[k]), rel(yard[k], ref[k])
        print(f"{what} {k}: ours {eo:.3e}  restatement under autocast {ey:.3e}")
        if eo > FACTOR * ey:
            worse[k] = (eo, ey)
    assert not worse, f"{what}: ours worse than {FACTOR} x the autocast restatement: {worse}"


@pytest.mark.parametrize("kernels", [True, False])
@pytest.mark.parametrize("mode", list(MODES))
def test_model_fixture_against_the_autocast_yardstick(mode, kernels):
    m = build()
    ref_out, ref_loss, ref_grads = model_reference()
    y_out, _, y_grads = autocast_model(m, mode)
    ops.set_visible_token_kernels(kernels)
    out, loss, grads = ours_model(m, mode)
    assert out.shape == (2, 12, 588) and torch.isfinite(loss)
    assert all(g is not None and torch.isfinite(g).all() for g in grads.values())
    assert set(grads) == set(ref_grads) and len(grads) == 44 and "encoder.pos_embed" in grads and "mask_token" in grads
    compare({"output": out, **grads}, {"output": y_out, **y_grads}, {"output": ref_out, **ref_grads}, f"model {mode} kernels={kernels}")


@pytest.mark.parametrize("kernels", [True, False])
@pytest.mark.parametrize("name", list(PR.VARIANTS))
@pytest.mark.parametrize("mode", list(MODES))
def test_variants_forward(name, mode, kernels):
    over = PR.VARIANTS[name]
    cfg = dict(PR.TINY, **over)
    m = build(**over).eval()
    x, mask = PR.clip().cuda(), PR.mask().cuda()
    P = OrderedDict((k, v.detach()) for k, v in m.named_parameters())
    with torch.no_grad():
        ref = PR.model(OrderedDict((k, v.double()) for k, v in P.items()), x.double(), mask, cfg)
        assert R.matches(ref, PR.load()[f"c/{name}/output"], 1000) <= PR.REPRO_TOL, "the restatement on the device is the recorded reference"
        with torch.autocast(device_type="cuda", dtype=MODES[mode]):
            yard = PR.model(P, x, mask, cfg).float()
        T.set_precision(mode)
        ops.set_visible_token_kernels(kernels)
        ours = m(x, mask)
    eo, ey = rel(ours, ref), rel(yard, ref)
    print(f"{name} {mode} kernels={kernels}: ours {eo:.3e}  restatement under autocast {ey:.3e}")
    assert eo <= FACTOR * ey


def test_the_sep_pos_variant_splits_the_table_gradient_by_autograd():
    m = build(sep_pos_embed=True)
    _, _, grads = ours_model(m, "fast")
    assert grads["encoder.pos_embed_spatial"].abs().sum() > 0 and grads["encoder.pos_embed_temporal"].abs().sum() > 0
    assert grads["encoder.pos_embed_cls"] is None  # (built and never used, as in the reference)


def test_checkpointed_block_gives_the_same_gradients_bit_for_bit():
    plain, ckpt = build(), build(use_checkpoint=True, checkpoint_num=1)
    assert ckpt.encoder.blocks[0].with_cp and not ckpt.encoder.blocks[1].with_cp
    o0, _, g0 = ours_model(plain, "fast")
    o1, _, g1 = ours_model(ckpt, "fast")
    assert torch.equal(o0, o1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_frozen_patch_embed_gets_no_gradient_and_no_dx():
    """with the projection frozen nothing in front of the visible-token entry wants a gradient: its backward is launched for the
    table's gradient alone (no dx), and every other gradient keeps its bits"""
    m = build()
    calls = []
    orig = K.visible_tokens_bwd

    def spy(g, slot, want_dx=True, want_dpos=True, into=None):
        calls.append((want_dx, want_dpos))
        return orig(g, slot, want_dx=want_dx, want_dpos=want_dpos, into=into)
    K.visible_tokens_bwd = spy
    try:
        _, _, full = ours_model(m, "fast")
        full = {k: v.clone() for k, v in full.items()}
        assert calls == [(True, True)]
        for p in m.encoder.patch_embed.parameters():
            p.requires_grad_(False)
        _, _, part = ours_model(m, "fast")
        assert calls == [(True, True), (False, True)]
    finally:
        K.visible_tokens_bwd = orig
    for k, g in part.items():
        if k.startswith("encoder.patch_embed."):
            assert g is None, k
        else:
            assert torch.equal(g, full[k]), f"{k} changed when the patch embedding was frozen"


def test_three_steps_of_train_one_epoch_double_move_every_tensor():
    T.set_precision("half")
    torch.manual_seed(0)
    m = IVP.PretrainVideoMAEInternVideo2(norm_layer=partial(nn.LayerNorm, eps=1e-6), **PR.TINY).cuda()
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    opt = E.create_optimizer(m, lr=1e-3, weight_decay=0.05)
    assert isinstance(opt, FusedAdamW)
    scaler = E.NativeScalerWithGradNormCount(m, init_scale=HALF_SCALE)
    g = torch.Generator().manual_seed(9)
    mask = PR.mask()
    # two in-memory loaders of different batch sizes: 2 clips on the device, 1 clip on the host with its mask as [T, H*W]
    loader1 = [(torch.randn(2, 3, 4, 28, 28, generator=g).cuda(), mask.cuda()) for _ in range(3)]
    loader2 = [(torch.randn(1, 3, 4, 28, 28, generator=g), mask[1:].view(1, 4, 4)) for _ in range(4)]
    seen = []
    orig = K.visible_tokens_bwd

    def spy(g_, slot, want_dx=True, want_dpos=True, into=None):
        seen.append((tuple(g_.shape), want_dx, want_dpos, into is not None))
        return orig(g_, slot, want_dx=want_dx, want_dpos=want_dpos, into=into)
    K.visible_tokens_bwd = spy
    try:
        stats = EP.train_one_epoch_double(m, loader1, loader2, opt, torch.device("cuda"), 0, scaler, patch_size=14, tubelet_size=1)
    finally:
        K.visible_tokens_bwd = orig
    assert len(stats["loss"]) == 3 and all(torch.isfinite(torch.tensor(v)) for v in stats["loss"])
    assert seen == [((3, PR.NV, 128), True, True, True)] * 3, "three clips per step, the table's gradient straight into the optimizer's flat buffer"
    still = [k for k, p in m.named_parameters() if torch.equal(p.detach(), before[k])]
    assert not still, f"tensors that did not move in three steps: {still}"
    assert all(torch.isfinite(p).all() for p in m.parameters())
    assert "averaged" in stats and set(stats) >= {"loss", "grad_norm", "lr", "min_lr", "loss_scale", "weight_decay"}


def test_real_size_factory_forward_backward():
    torch.manual_seed(0)
    m = T.create_model("pretrain_videomae_internvideo2_patch14_224").cuda()
    from simple_tad_amd.masking_generator import TubeMaskingGenerator
    mask = torch.from_numpy(TubeMaskingGenerator((8, 16, 16), 0.75)()).bool().reshape(1, -1).repeat(2, 1).cuda()
    assert int(mask[0].sum()) == 1536
    x = torch.randn(2, 3, 8, 224, 224, generator=torch.Generator().manual_seed(1)).cuda()
    out = m(x, mask, num_masked=1536)
    assert out.shape == (2, 1536, 588) and torch.isfinite(out).all()
    ops.MseLossFn.apply(out, torch.zeros_like(out)).backward()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert m.encoder.pos_embed.grad.abs().sum() > 0
