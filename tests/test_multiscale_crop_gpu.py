"""The MAE pre-training crop on the MI355X: ``tad_multiscale_crop`` against the reference's frames (golden G18: every case, through
``apply`` and through the seeded call) with 0 differing bytes; the fused f32 output against ``frames_to_clip`` of the uint8 output;
the same bits whatever the base alignment and the batch; guard bands around every operand; no host sync; the pre-training engine
with ``augment_fn`` against the same loop fed pre-augmented clips."""
import functools
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import multiscale_crop_recipe as MR
from guarded import GuardedArena, same_bits
from simple_tad_amd import kernels as K
from simple_tad_amd import transforms as TF
from simple_tad_amd.rand_augment import frames_to_clip
from test_multiscale_crop_cpu import transform_of

pytestmark = pytest.mark.gpu
MEAN, STD = TF.IMAGENET_DEFAULT_MEAN, TF.IMAGENET_DEFAULT_STD
CASE = {c[0]: c for c in MR.CASES}


@functools.lru_cache(maxsize=None)
def frames(Hs, Ws, kind="noise"):
    return torch.from_numpy(MR.frames(Hs, Ws, kind))


def golden_plan(g, key):
    return [TF.Crop(b, *[int(v) for v in row]) for b, row in enumerate(g[f"{key}.crops"])]


def differing(got, want, what):
    n = int((got != want).sum())
    print(f"multiscale crop {what}: {n} of {want.size} bytes differ from the reference")
    return n


@pytest.mark.parametrize("case", MR.CASES, ids=MR.CASE_IDS)
def test_every_case_equals_the_reference(golden, case):
    g = golden("g18_multiscale_crop")
    key, seed, (Hs, Ws), S, _, kind = case
    tf = transform_of(case)
    x = frames(Hs, Ws, kind).cuda()
    out = tf.apply(x, golden_plan(g, key))
    assert out.dtype == torch.uint8 and tuple(out.shape) == (MR.B, MR.T, S, S, 3)
    assert torch.equal(x.cpu(), frames(Hs, Ws, kind))                      # the input is only read
    assert differing(out.cpu().numpy(), g[f"{key}.out"], f"{key} apply") == 0
    random.seed(seed)
    called = tf(x)
    assert random.random() == float(g[f"{key}.next_py"])
    assert differing(called.cpu().numpy(), g[f"{key}.out"], f"{key} seeded call") == 0
    # the fused f32 output is frames_to_clip of the uint8 output, bit for bit; out= is honoured
    want = frames_to_clip(out, MEAN, STD)
    buf = torch.full((MR.B, 3, MR.T, S, S), float("nan"), device="cuda")
    got = tf.apply(x, golden_plan(g, key), out=buf, normalize=(MEAN, STD))
    assert got is buf and tuple(got.shape) == (MR.B, 3, MR.T, S, S) and same_bits(got, want) and torch.equal(got, want)


VARIATION_CASES = ("down.45x80.s5", "up.20x23", "portrait.100x37", "k17.120x200")


@pytest.mark.parametrize("key", VARIATION_CASES)
def test_same_bits_whatever_the_base_offset_and_the_batch(golden, key):
    g = golden("g18_multiscale_crop")
    _, _, (Hs, Ws), S, _, kind = CASE[key]
    tf, plan, x = transform_of(CASE[key]), golden_plan(g, key), frames(Hs, Ws, kind)
    want = torch.from_numpy(g[f"{key}.out"])
    want_f32 = frames_to_clip(want.cuda(), MEAN, STD).cpu()
    for off in (1, 2, 3):                                                   # the input's base 1..3 bytes behind an aligned address,
        flat = torch.cat([torch.full((off,), 99, dtype=torch.uint8), x.flatten()]).cuda()
        xo = flat[off:].view(x.shape)
        obuf = torch.full((want.numel() + off,), 55, dtype=torch.uint8, device="cuda")          # and the uint8 output's
        fbuf = torch.full((want_f32.numel() + off,), 7.0, device="cuda")                        # the f32 output's by floats
        assert xo.data_ptr() % 4 == off and xo.is_contiguous()
        out = tf.apply(xo, plan, out=obuf[off:].view(want.shape))
        assert torch.equal(out.cpu(), want) and bool((obuf[:off] == 55).all()), off
        clip = tf.apply(xo, plan, out=fbuf[off:].view(want_f32.shape), normalize=(MEAN, STD))
        assert same_bits(clip.cpu(), want_f32) and bool((fbuf[:off] == 7.0).all()), off
        assert torch.equal(flat.cpu()[off:].view(x.shape), x) and bool((flat[:off] == 99).all())
    # a batch of 6 mixing crops: the three clips twice, the second time under the crops of the clips after them
    twice = torch.cat([x, x]).cuda()
    plan6 = plan + [TF.Crop(3 + b, *plan[(b + 1) % 3][1:]) for b in range(3)]
    out6 = tf.apply(twice, plan6).cpu()
    assert torch.equal(out6[:3], want)
    for b in range(3):
        c = plan[(b + 1) % 3]
        assert np.array_equal(out6[3 + b].numpy(), MR.crop_resize(x[b:b + 1].numpy(), [(c.w, c.h, c.x0, c.y0)], S, S)[0]), b


def test_rectangular_output_and_several_tiles():
    """[S_w, S_h] = [70, 37]: three column tiles and two row tiles with ragged edges, S_w * 3 and S_w no multiple of 4"""
    x = frames(100, 37)
    tf = TF.GroupMultiScaleCrop([70, 37])
    plan = [TF.Crop(0, 37, 100, 0, 0), TF.Crop(1, 30, 61, 7, 39), TF.Crop(2, 25, 25, 3, 70)]
    want = np.stack([np.stack([MR.resize(x[c.clip, t, c.y0:c.y0 + c.h, c.x0:c.x0 + c.w].numpy(), 70, 37) for t in range(MR.T)]) for c in plan])
    out = tf.apply(x.cuda(), plan)
    assert tuple(out.shape) == (3, MR.T, 37, 70, 3) and differing(out.cpu().numpy(), want, "70 x 37") == 0
    assert torch.equal(tf.apply(x.cuda(), plan, normalize=(MEAN, STD)), frames_to_clip(out, MEAN, STD))


# ------------------------------------------------------------------ guard bands
def guarded_operands(arena, tf, plan, x, offset):
    B, _, Hs, Ws, _ = x.shape
    table, nh, nv = tf.table(plan, B, Hs, Ws)
    flat = arena.place(torch.cat([torch.full((offset,), 99, dtype=torch.uint8), x.flatten()]), role="input", name="frames")
    # guards of the table hold words in [0, 3): what is read past its ends would be small valid values and show in the result
    tab = arena.place(table, role="input", name="table (the workspace)", index_range=3)
    return flat[offset:].view(x.shape), tab, nh, nv


@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("key", ("down.45x80.s1", "up.20x23", "k17.120x200"))
@pytest.mark.parametrize("offset", [0, 3])
def test_kernel_stays_inside_its_operands(golden, key, poison, offset):
    g = golden("g18_multiscale_crop")
    _, _, (Hs, Ws), S, _, kind = CASE[key]
    tf = transform_of(CASE[key])
    arena = GuardedArena(8 << 20, "cuda", poison=poison)
    x, tab, nh, nv = guarded_operands(arena, tf, golden_plan(g, key), frames(Hs, Ws, kind), offset)
    with arena.route(K):
        out = K.multiscale_crop(x, tab, nh, nv, S, S)
        clip = K.multiscale_crop(x, tab, nh, nv, S, S, MEAN, STD)
    arena.verify()                                                          # the input and the table are unchanged, the guards too
    assert arena.contains(out) and arena.contains(clip)
    assert differing(out.cpu().numpy(), g[f"{key}.out"], f"{key} guarded {poison} +{offset}") == 0
    assert torch.equal(clip, frames_to_clip(out, MEAN, STD))


def test_malformed_rows_are_never_an_address():
    """rows the host check would refuse (tests/multiscale_crop_recipe.py: wild_table): a sample outside the batch does nothing; a
    crop, set indices, ksize and bounds far outside are cut to the source and the sets, and the clip they name holds what the clamps
    define; the valid row is carried out and nothing outside the output is written.  The same table runs through the kernel's text
    on the CPU under sanitizers first (tools/multiscale_crop_host_check.py, tests/test_multiscale_crop_cpu.py)."""
    Hs, Ws, S = 45, 80, 32
    tf = TF.GroupMultiScaleCrop(S)
    arena = GuardedArena(8 << 20, "cuda")
    x, tab, nh, nv = guarded_operands(arena, tf, [TF.Crop(b, *c) for b, c in enumerate(MR.WILD_PLAN)], frames(Hs, Ws), 0)
    bad, want2 = MR.wild_table(tab.cpu().numpy(), frames(Hs, Ws).numpy(), S)
    tab.copy_(torch.from_numpy(bad))
    arena.snapshot()
    with arena.route(K):
        out = K.multiscale_crop(x, tab, nh, nv, S, S)
    arena.verify()
    assert np.array_equal(out[0].cpu().numpy(), MR.crop_resize(frames(Hs, Ws).numpy(), [MR.WILD_PLAN[0]], S, S)[0])
    assert bool((out[1] == 0x7F).all())                                     # the clip no row names: as the arena filled it
    assert np.array_equal(out[2].cpu().numpy(), want2)


# ------------------------------------------------------------------ host side
def test_call_does_not_synchronise_with_the_host():
    args = SimpleNamespace(input_size=32, mask_type="tube", window_size=(1, 2, 2), mask_ratio=0.75)
    aug = TF.DataAugmentationForVideoMAE(args)
    tf = TF.GroupMultiScaleCrop(32)
    x = frames(45, 80).cuda()
    random.seed(3)
    np.random.seed(3)
    aug(x), tf(x)                                      # (first call: library load, allocator warm-up)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):             # the mode is live in this build: a host read of device memory is refused
            x.sum().item()
        for _ in range(6):
            clips, masks = aug(x)
            tf(x)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert tuple(clips.shape) == (3, 3, 2, 32, 32) and tuple(masks.shape) == (3, 4) and not masks.is_cuda


def test_data_augmentation_is_the_crop_the_normalisation_and_one_mask_per_clip():
    args = SimpleNamespace(input_size=32, mask_type="tube", window_size=(1, 2, 2), mask_ratio=0.75)
    x = frames(45, 80).cuda()
    for cls, scales in ((TF.DataAugmentationForVideoMAE, MR.DEFAULT_SCALES), (TF.DataAugmentationForVideoMAE_LightCrop, MR.LIGHT_SCALES)):
        random.seed(5)
        np.random.seed(5)
        clips, masks = cls(args)(x)
        py, npy = random.random(), np.random.random()
        random.seed(5)
        np.random.seed(5)
        crops = [MR.sample_crop(80, 45, 32, 32, scales=scales) for _ in range(MR.B)]
        from simple_tad_amd.masking_generator import TubeMaskingGenerator
        gen = TubeMaskingGenerator((1, 2, 2), 0.75)
        want_masks = np.stack([gen() for _ in range(MR.B)])
        assert (py, npy) == (random.random(), np.random.random())
        want = frames_to_clip(torch.from_numpy(MR.crop_resize(x.cpu().numpy(), crops, 32, 32)).cuda(), MEAN, STD)
        assert torch.equal(clips, want) and np.array_equal(masks.numpy(), want_masks)


# ------------------------------------------------------------------ the pre-training engine
def test_engine_with_augment_fn_equals_the_loop_fed_pre_augmented_clips(golden):
    from simple_tad_amd import engine as E, engine_pretrain as EP
    from simple_tad_amd.parallel import DataParallel
    from test_pretrain import setup
    args = SimpleNamespace(input_size=32, mask_type="tube", window_size=(8, 2, 2), mask_ratio=0.75)
    rng = np.random.default_rng(18)
    batches = [torch.from_numpy(rng.integers(0, 256, (2, 16, 45, 80, 3), dtype=np.uint8)) for _ in range(2)]

    def run(hook):
        _, _, m, P, _, _ = setup(golden)
        m.load_state_dict(P)
        m = DataParallel(m.cuda())
        opt = E.create_optimizer(m, lr=1e-3, weight_decay=0.05)
        scaler = E.NativeScalerWithGradNormCount(m)
        random.seed(11)
        np.random.seed(11)
        aug = TF.DataAugmentationForVideoMAE(args)
        if hook:
            data = [(f,) for f in batches]
        else:                                                               # the same draws, made before the loop
            data = [tuple(v.cpu() for v in aug(f.cuda())) for f in batches]
        stats = EP.train_one_epoch(m, data, opt, torch.device("cuda"), 0, scaler, patch_size=16, augment_fn=aug if hook else None)
        return stats["loss"]

    with_hook, without = run(True), run(False)
    print(f"pre-training losses with augment_fn {with_hook}, fed pre-augmented clips {without}")
    assert len(with_hook) == 2 and with_hook == without
