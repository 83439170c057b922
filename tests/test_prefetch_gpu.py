"""ClipPrefetcher on the device: content under slot reuse, the 16-bit clip route of PatchEmbed, and the engines on a wrapped loader.

Everything here is an identity: a prefetched batch holds the loader's bits, a clip shipped in the operand format gives the bits the f32
clip gives (the im2col rounds the f32 clip the way the staging pass does), and an engine fed through the wrapper computes what it
computes from batches that already are on the device.  So every comparison is bit for bit; there is no tolerance to choose."""
import copy
import functools

import numpy as np
import pytest
import torch

import simple_tad_amd as T
from simple_tad_amd import ClipPrefetcher, engine as E

pytestmark = pytest.mark.gpu

OPERAND = {"fast": torch.bfloat16, "half": torch.float16}
TINY = dict(img_size=32, patch_size=16, embed_dim=128, depth=1, num_heads=2, mlp_ratio=4, qkv_bias=True, all_frames=4, tubelet_size=2,
            num_classes=2, init_scale=1.0)


@pytest.fixture
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    yield torch.device("cuda", torch.cuda.current_device())
    T.set_precision("fast")


@functools.lru_cache(maxsize=None)
def tiny_state():
    torch.manual_seed(11)
    m = T.VisionTransformer(norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6), **TINY)
    return {k: v.clone() for k, v in m.state_dict().items()}


def tiny_model(dev):
    m = T.VisionTransformer(norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6), **TINY)
    m.load_state_dict(copy.deepcopy(tiny_state()))
    return m.to(dev)


@functools.lru_cache(maxsize=None)
def host_batches():
    """three (clip f32 [2,3,4,32,32], target [2], names, extra_info) batches in pageable memory; computed once, never written"""
    g = torch.Generator().manual_seed(23)
    return tuple((torch.randn(2, 3, 4, 32, 32, generator=g), torch.tensor([i % 2, 1 - i % 2]), [f"v{i}a", f"v{i}b"],
                  {"ttc": torch.rand(2, generator=g), "smoothed_labels": torch.rand(2, 2, generator=g)}) for i in range(3))


def on_device(batches, dev):
    return [(b[0].to(dev), b[1].to(dev), b[2], {k: v.to(dev) for k, v in b[3].items()}) for b in batches]


# ------------------------------------------------------------------------------------------------- content under slot reuse
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_every_batch_holds_its_own_index(dev, pinned):
    """depth 2, eight batches, every yielded tensor kept and compared at the end: a slot rewritten before its copy had left it, or a
    device tensor reused while the consumer still holds it, shows as another batch's index"""
    def src(i):
        u8 = torch.full((2, 16, 224, 224, 3), i + 1, dtype=torch.uint8)
        f32 = torch.full((2, 3, 4, 32, 32), i + 0.25)
        return (u8.pin_memory(), f32.pin_memory(), i) if pinned else (u8, f32, i)

    pf = ClipPrefetcher([src(i) for i in range(8)], dev, depth=2)
    kept = []
    for out in pf:
        assert out[0].device == dev and out[1].device == dev and out[0].dtype == torch.uint8 and out[1].dtype == torch.float32
        kept.append(out)
        out[1].mul(2.0)  # (work on the consumer's stream that reads the batch)
    assert [o[2] for o in kept] == list(range(8))
    if pinned:
        assert pf._slots == {}  # a pinned leaf is copied from directly
    else:
        assert sorted(pf._slots) == [(0,), (1,)] and all(s.is_pinned() for ring in pf._slots.values() for s in ring)
        assert all(len(ring) == 2 for ring in pf._slots.values())
    torch.cuda.synchronize()
    for i, (u8, f32, _) in enumerate(kept):
        assert torch.equal(u8.cpu(), torch.full((2, 16, 224, 224, 3), i + 1, dtype=torch.uint8)), f"uint8 batch {i}: {u8.unique().tolist()}"
        assert torch.equal(f32.cpu().view(torch.int32), torch.full((2, 3, 4, 32, 32), i + 0.25).view(torch.int32)), f"f32 batch {i}"
    assert len({t.data_ptr() for o in kept for t in o[:2]}) == 16


# ------------------------------------------------------------------------------------------------- the clip's dtype
def logits_and_grads(m, clip, target):
    for p in m.parameters():
        p.grad = None
    out = m(clip)
    torch.nn.functional.cross_entropy(out.float(), target).backward()
    return out.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("mode", ["fast", "half"])
def test_clip_in_the_operand_format_gives_the_bits_of_the_f32_clip(dev, mode):
    from guarded import same_bits
    T.set_precision(mode)
    op, other = OPERAND[mode], OPERAND["half" if mode == "fast" else "fast"]
    m = tiny_model(dev).train()
    clip = host_batches()[0][0].to(dev)
    target = host_batches()[0][1].to(dev)
    assert bool(torch.isfinite(clip).all())
    ref_out, ref_g = logits_and_grads(m, clip, target)
    out16, g16 = logits_and_grads(m, clip.to(op), target)
    assert same_bits(out16, ref_out)
    assert sorted(g16) == sorted(ref_g) and len(ref_g) == len([p for p in m.parameters() if p.requires_grad])
    for k in ref_g:
        assert same_bits(g16[k], ref_g[k]), k
    # a view the 16-byte loads cannot take goes through the f32 route: the same bits again
    buf = torch.empty(clip.numel() + 8, dtype=op, device=dev)
    off = buf[4:4 + clip.numel()].view(clip.shape)
    off.copy_(clip)
    assert off.data_ptr() % 16 == 8
    out_off, g_off = logits_and_grads(m, off, target)
    assert same_bits(out_off, ref_out) and all(same_bits(g_off[k], ref_g[k]) for k in ref_g)
    # the OTHER 16-bit format is not the operand format: today's upcast route, bit for bit
    x_other = clip.to(other)
    out_up, g_up = logits_and_grads(m, x_other.float(), target)
    out_ot, g_ot = logits_and_grads(m, x_other, target)
    assert same_bits(out_ot, out_up) and all(same_bits(g_ot[k], g_up[k]) for k in g_up)
    # without a backward pass (eval, no_grad) a 16-bit clip takes the explicit route: the same logits as the f32 clip
    m.eval()
    with torch.no_grad():
        assert same_bits(m(clip.to(op)), m(clip))


def test_precise_keeps_the_upcast_route(dev):
    from guarded import same_bits
    T.set_precision("precise")
    m = tiny_model(dev).eval()
    x16 = host_batches()[0][0].to(dev).bfloat16()
    with torch.no_grad():
        assert same_bits(m(x16), m(x16.float()))


# ------------------------------------------------------------------------------------------------- the engines on a wrapped loader
def three_steps(dev, loader):
    m = tiny_model(dev)
    opt = E.create_optimizer(m, lr=1e-3, weight_decay=0.05)
    stats = E.train_one_epoch(m, torch.nn.CrossEntropyLoss(), loader, opt, dev, 0, E.NativeScalerWithGradNormCount(m), max_norm=1.0)
    return stats, {k: v.detach().clone() for k, v in m.state_dict().items()}


@pytest.fixture(scope="module")
def resident_run():
    """the run every wrapped run is compared with: the same batches placed on the device beforehand (computed once)"""
    dev = torch.device("cuda", torch.cuda.current_device())
    T.set_precision("fast")
    return three_steps(dev, on_device(host_batches(), dev))


@pytest.mark.parametrize("wire", ["same", "operand"])
def test_three_training_steps_from_a_wrapped_pageable_loader(dev, resident_run, wire):
    ref_stats, ref_params = resident_run
    pf = ClipPrefetcher(list(host_batches()), dev, depth=2, wire=wire)
    stats, params = three_steps(dev, pf)
    assert len(stats["loss"]) == 3 and stats["loss"] == ref_stats["loss"], (stats["loss"], ref_stats["loss"])
    assert stats["grad_norm"] == ref_stats["grad_norm"] and stats["class_acc"] == ref_stats["class_acc"]
    assert sorted(params) == sorted(ref_params)
    for k in ref_params:
        assert torch.equal(params[k], ref_params[k]), k
    assert any(not torch.equal(ref_params[k].cpu(), tiny_state()[k]) for k in ref_params)  # (the steps did move the weights)
    pf.close()


def test_frame_loss_inputs_come_from_the_wrapped_extra_info(dev):
    """with_ttc / smoothed_labels_for_loss read batch[3]: the dict arrives with its tensors on the device and the same values"""
    def run(loader):
        m = tiny_model(dev)
        opt = E.create_optimizer(m, lr=1e-3, weight_decay=0.05)
        st = E.train_one_epoch(m, T.SoftTargetCrossEntropy(), loader, opt, dev, 0, E.NativeScalerWithGradNormCount(m), smoothed_labels_for_loss=True)
        return st["loss"]

    assert run(ClipPrefetcher(list(host_batches()), dev, depth=1)) == run(on_device(host_batches(), dev))


def test_validation_accepts_the_wrapped_loader(dev):
    m = tiny_model(dev)
    a = E.validation_one_epoch(list(host_batches()), m, dev)
    b = E.validation_one_epoch(ClipPrefetcher(list(host_batches()), dev, depth=2), m, dev)
    np.testing.assert_equal(b[0], a[0])
    np.testing.assert_equal(b[1], a[1])


def test_pretrain_engine_accepts_the_wrapped_loader(dev):
    import simple_tad_amd.modeling_pretrain as mp
    from simple_tad_amd import engine_pretrain as EP
    torch.manual_seed(4)
    proto = mp.PretrainVisionTransformer(img_size=32, patch_size=16, encoder_embed_dim=128, encoder_depth=1, encoder_num_heads=2,
                                         decoder_num_classes=1536, decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=1, mlp_ratio=4,
                                         qkv_bias=True, norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6), init_values=0., tubelet_size=2)
    state = copy.deepcopy(proto.state_dict())
    g = torch.Generator().manual_seed(9)
    masks = torch.zeros(2, 32, dtype=torch.bool)
    masks[:, torch.randperm(32, generator=g)[:24]] = True  # the model's 16 frames: 32 tokens per clip (8 x 2 x 2), 24 masked in each
    batches = [(torch.randn(2, 3, 16, 32, 32, generator=g), masks.clone()) for _ in range(3)]

    def run(loader):
        m = copy.deepcopy(proto)
        m.load_state_dict(copy.deepcopy(state))
        m = m.to(dev)
        opt = E.create_optimizer(m, lr=1e-3, weight_decay=0.05)
        st = EP.train_one_epoch(m, loader, opt, dev, 0, E.NativeScalerWithGradNormCount(m), max_norm=1.0, patch_size=16)
        return st["loss"], st["grad_norm"], {k: v.detach().clone() for k, v in m.state_dict().items()}

    la, na, pa = run(batches)
    lb, nb, pb = run(ClipPrefetcher(batches, dev, depth=2, wire="same"))
    assert la == lb and na == nb and len(la) == 3
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
