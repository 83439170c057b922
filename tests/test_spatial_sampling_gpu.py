"""The fine-tune spatial sampling on the MI355X: ``tad_spatial_sample`` against the numpy restatement of the arithmetic
include/tad_mi355x.h states (tests/spatial_sampling_recipe.py) bit for bit, and so against the reference's f32 output (golden G20)
within the reference's own error, for every case through ``apply`` and through the seeded call; the uint8 route against the f32 route
on ``frames_to_clip``; the same bits whatever the base alignment and the batch; several tiles; guard bands around every operand; no
host sync; the fine-tune engine with the whole device-side chain against the same loop fed pre-augmented clips."""
import functools
import random

import numpy as np
import pytest
import torch

import golden_recipe as R
import mixup_recipe as MXR
import spatial_sampling_recipe as SR
from guarded import GuardedArena, same_bits
from simple_tad_amd import engine as E
from simple_tad_amd import kernels as K
from simple_tad_amd.loss import SoftTargetCrossEntropy
from simple_tad_amd.mixup import Mixup
from simple_tad_amd.rand_augment import create_random_augment, frames_to_clip
from simple_tad_amd.random_erasing import RandomErasing
from simple_tad_amd.spatial_sampling import SpatialSampling, Window
from test_mixup_cpu import _build_tiny

pytestmark = pytest.mark.gpu
MEAN, STD = SR.MEAN, SR.STD
CASE = {c[0]: c for c in SR.CASES}


@functools.lru_cache(maxsize=None)
def clips(H, W):
    return torch.from_numpy(SR.clips(H, W))


@functools.lru_cache(maxsize=None)
def frames(H, W):
    return torch.from_numpy(SR.frames(H, W))


def golden_plan(g, key):
    return [Window(*[int(v) for v in row]) for row in g[f"{key}.windows"]]


_restated = {}


def restated(g, key):
    """the numpy restatement of a case under its golden windows: computed once, shared, never written"""
    if key not in _restated:
        _, _, (H, W), kw = CASE[key]
        out = SR.sample(SR.clips(H, W), g[f"{key}.windows"], kw["crop_size"])
        out.setflags(write=False)
        _restated[key] = out
    return torch.from_numpy(_restated[key])


def within_bound(got, g, key, what):
    err, bound = float(np.abs(got.double().cpu().numpy() - g[f"{key}.out"]).max()), SR.bound(g, key)
    print(f"spatial sampling {what}: max |device - reference| {err:.3g}, bound 2 gap + 4 ulp = {bound:.3g}, ratio {err / bound:.3f}")
    return err <= bound


@pytest.mark.parametrize("case", SR.CASES, ids=SR.CASE_IDS)
def test_every_case_equals_the_restatement_bit_for_bit(golden, case):
    g = golden("g20_spatial_sampling")
    key, seed, (H, W), kw = case
    S = kw["crop_size"]
    ss, plan, want = SpatialSampling(**kw), golden_plan(g, key), restated(g, key)
    x = clips(H, W).cuda()
    out = ss.apply(x, plan)
    assert out.dtype == torch.float32 and tuple(out.shape) == (SR.B, 3, SR.T, S, S)
    assert same_bits(x.cpu(), clips(H, W))                                  # the input is only read
    assert same_bits(out.cpu(), want), int((out.cpu() != want).sum())
    assert within_bound(out, g, key, f"{key} apply")
    if key in SR.EXACT_CASES:
        assert same_bits(out.cpu(), torch.from_numpy(g[f"{key}.out"]))
    random.seed(seed)
    np.random.seed(seed)
    called = ss(x)
    assert (random.random(), np.random.uniform()) == (float(g[f"{key}.next_py"]), float(g[f"{key}.next_np"]))
    assert same_bits(called.cpu(), want) and within_bound(called, g, key, f"{key} seeded call")
    # uint8 frames with normalize: the bits of the f32 route on frames_to_clip(x); out= is honoured
    u8 = frames(H, W).cuda()
    clip = frames_to_clip(u8, MEAN, STD)
    assert same_bits(clip.cpu(), clips(H, W))
    buf = torch.full((SR.B, 3, SR.T, S, S), float("nan"), device="cuda")
    got = ss.apply(u8, plan, out=buf, normalize=(MEAN, STD))
    assert got is buf and same_bits(got, ss.apply(clip, plan)) and same_bits(got.cpu(), want)
    assert torch.equal(u8.cpu(), frames(H, W))
    random.seed(seed)
    np.random.seed(seed)
    assert same_bits(ss(u8, normalize=(MEAN, STD)).cpu(), want)


VARIATION_CASES = ("down.37x53", "s18.37x53", "shift.37x53")


@pytest.mark.parametrize("key", VARIATION_CASES)
def test_same_bits_whatever_the_base_offset_and_the_batch(golden, key):
    g = golden("g20_spatial_sampling")
    _, _, (H, W), kw = CASE[key]
    ss, plan, want = SpatialSampling(**kw), golden_plan(g, key), restated(g, key)
    x, u8 = clips(H, W), frames(H, W)
    for off in (1, 2, 3):
        # the uint8 frames' base 1..3 bytes behind an aligned address; the f32 output 1..3 floats behind a 16-byte boundary
        flat = torch.cat([torch.full((off,), 99, dtype=torch.uint8), u8.flatten()]).cuda()
        uo = flat[off:].view(u8.shape)
        fbuf = torch.full((want.numel() + off,), 7.0, device="cuda")
        out = fbuf[off:].view(want.shape)
        assert uo.data_ptr() % 4 == off and out.data_ptr() % 16 == 4 * off
        assert ss.apply(uo, plan, out=out, normalize=(MEAN, STD)) is out
        assert same_bits(out.cpu(), want) and bool((fbuf[:off] == 7.0).all()), off
        assert torch.equal(flat.cpu()[off:].view(u8.shape), u8) and bool((flat[:off] == 99).all())
        # the f32 clips 1..3 floats behind a 16-byte boundary as well
        xbuf = torch.cat([torch.full((off,), 5.0), x.flatten()]).cuda()
        fbuf.fill_(7.0)
        assert ss.apply(xbuf[off:].view(x.shape), plan, out=out) is out
        assert same_bits(out.cpu(), want) and bool((fbuf[:off] == 7.0).all()), off
    # a batch of 6: the three clips twice, the second time under the windows of the clips after them
    twice = torch.cat([x, x])
    rows = g[f"{key}.windows"]
    moved = rows.copy()
    moved[:, 0] = 3 + (rows[:, 0] - 1) % 3                                 # clip 3 + b takes the windows of clip (b + 1) % 3
    rows6 = np.concatenate([rows, moved])
    want6 = SR.sample(twice.numpy(), rows6, kw["crop_size"])
    assert np.array_equal(want6[:3].view(np.int32), want.numpy().view(np.int32))
    out6 = ss.apply(twice.cuda(), [Window(*[int(v) for v in r]) for r in rows6])
    assert same_bits(out6.cpu(), torch.from_numpy(want6))


def test_several_tiles_with_ragged_edges():
    """S = 70: three column tiles and three row tiles, the last ones ragged, S no multiple of 4; windows stated by hand, one per frame:
    a box upscaled, a box downscaled, a jittered grid with a crop offset, with and without the flip"""
    H, W, S = 45, 80, 70
    rng = np.random.default_rng(70)
    u8 = rng.integers(0, 256, (2, 2, H, W, 3), dtype=np.uint8)
    x = SR.normalise(u8)
    rows = np.array([(0, 0, 3, 5, 30, 41, S, S, 0, 0, 0), (0, 1, 0, 0, H, W, S, S, 0, 0, 1),
                     (1, 0, 0, 0, H, W, 90, 160, 7, 33, 1), (1, 1, 0, 0, H, W, 70, 124, 0, 54, 0)])
    want = torch.from_numpy(SR.sample(x, rows, S))
    ss = SpatialSampling(crop_size=S)
    plan = [Window(*[int(v) for v in r]) for r in rows]
    assert same_bits(ss.apply(torch.from_numpy(x).cuda(), plan).cpu(), want)
    assert same_bits(ss.apply(torch.from_numpy(u8).cuda(), plan, normalize=(MEAN, STD)).cpu(), want)


# ------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("key", ("down.37x53", "s18.37x53", "wide1.37x53", "jitter.20x27"))
@pytest.mark.parametrize("offset", [0, 3])
def test_kernel_stays_inside_its_operands(golden, key, poison, offset):
    g = golden("g20_spatial_sampling")
    _, _, (H, W), kw = CASE[key]
    S = kw["crop_size"]
    table = SpatialSampling(**kw).table(golden_plan(g, key), SR.B, SR.T, H, W)
    arena = GuardedArena(8 << 20, "cuda", poison=poison)
    x = arena.place(clips(H, W), role="input", name="clips")
    u8 = frames(H, W)
    flat = arena.place(torch.cat([torch.full((offset,), 99, dtype=torch.uint8), u8.flatten()]), role="input", name="frames")
    # guards of the table hold words in [0, 3): what is read past its ends would be small valid values and show in the result
    tab = arena.place(table, role="input", name="table (the workspace)", index_range=3)
    with arena.route(K):
        out = K.spatial_sample(x, tab, S)
        fused = K.spatial_sample(flat[offset:].view(u8.shape), tab, S, MEAN, STD)
    arena.verify()                                                          # the inputs and the table are unchanged, the guards too
    assert arena.contains(out) and arena.contains(fused)
    assert same_bits(out.cpu(), restated(g, key)) and same_bits(fused.cpu(), restated(g, key))


def test_malformed_rows_are_never_an_address():
    """rows the host check refuses: a sample outside the batch does nothing; a window, offsets and scales far outside (NaN and infinity
    among them) are cut to the source; nothing outside the output is written, the valid row is carried out, and the row whose
    clamps define a value holds it"""
    H, W, S = 20, 27, 12
    B, T = 2, 2
    x = clips(H, W)[:B, :, :T].contiguous()
    rows = np.array([(b, t, 2, 3, 15, 20, S, S, 0, 0, t) for b in range(B) for t in range(T)])
    ss = SpatialSampling(crop_size=S, **SR.RECIPE)
    table = ss.table([Window(*[int(v) for v in r]) for r in rows], B, T, H, W)
    bad = table.numpy().copy()
    bad[1, 0] = 99                                                          # ignored: frame (0, 1) stays unwritten
    bad[2, 1:10] = 1 << 20, -5, 1 << 30, -(1 << 30), 0, -7, 1 << 30, -(1 << 30), 5
    bad[2, 10:12] = np.array([np.nan, np.inf], dtype=np.float32).view(np.int32)
    bad[3, 7:9] = 2 ** 31 - 1, -(2 ** 31)
    bad[3, 10:12] = np.array([-3.0, 1e30], dtype=np.float32).view(np.int32)
    arena = GuardedArena(8 << 20, "cuda")
    xd = arena.place(x, role="input", name="clips")
    tab = arena.place(torch.from_numpy(bad), role="input", name="table (the workspace)", index_range=3)
    with arena.route(K):
        out = K.spatial_sample(xd, tab, S)
    arena.verify()
    out = out.cpu()
    assert same_bits(out[0, :, 0], torch.from_numpy(SR.sample_frame(x[0, :, 0].numpy(), rows[0, 2:], S)))
    assert bool(torch.isnan(out[0, :, 1]).all())                             # the frame no row names: as the arena filled it
    # row 2 is cut to the one pixel (H - 1, 0) of its frame; a NaN scale and a coordinate at minus infinity both give tap 0, weight 1
    assert same_bits(out[1, :, 0], x[1, :, 0, H - 1, 0].view(3, 1, 1).expand(3, S, S).contiguous())


# ------------------------------------------------------------------ host side
def test_call_does_not_synchronise_with_the_host():
    ss = SpatialSampling(crop_size=16, **SR.RECIPE)
    x, u8 = clips(37, 53).cuda(), frames(37, 53).cuda()
    random.seed(3)
    np.random.seed(3)
    ss(x), ss(u8, normalize=(MEAN, STD))                # (first call: library load, allocator warm-up)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):             # the mode is live in this build: a host read of device memory is refused
            x.sum().item()
        for _ in range(6):
            a = ss(x)
            b = ss(u8, normalize=(MEAN, STD))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert tuple(a.shape) == tuple(b.shape) == (3, 3, 4, 16, 16)


# ------------------------------------------------------------------ the fine-tune loop with the whole device-side chain
def test_engine_with_the_device_side_chain_equals_the_loop_fed_pre_augmented_clips():
    c = R.G12
    size = R.TINY["img_size"]
    rng = np.random.default_rng(20)
    batches = [(torch.from_numpy(rng.integers(0, 256, (2, R.TINY["all_frames"], 24, 30, 3), dtype=np.uint8)), torch.tensor(c["labels"][i]), None, None)
               for i in range(c["micro_batches"])]

    def run(hook, **sampling):
        m = _build_tiny("cuda", torch.float32)
        opt = E.create_optimizer(m, lr=c["base_lr"], weight_decay=c["weight_decay"], layer_decay=c["layer_decay"])
        random.seed(20)
        np.random.seed(20)
        torch.manual_seed(20)
        randaug = create_random_augment((24, 30), auto_augment="rand-m7-n4-mstd0.5-inc1", interpolation="bicubic")
        sampler = SpatialSampling(crop_size=size, **sampling)
        augment = lambda x: sampler(randaug(x), normalize=(MEAN, STD))
        if hook:
            data = batches
        else:     # the same draws in the same order: a loader that augments every batch right before the loop erases and mixes it
            data = ((augment(x.cuda()).cpu(), y, a, b) for x, y, a, b in batches)
        stats = E.train_one_epoch(m, SoftTargetCrossEntropy(), data, opt, torch.device("cuda"), 0, E.NativeScalerWithGradNormCount(m),
                                  max_norm=c["clip_grad"], update_freq=c["update_freq"], augment_fn=augment if hook else None,
                                  erase_fn=RandomErasing(probability=1.0, mode="const", max_area=0.1), mixup_fn=Mixup(**MXR.TRAJECTORY_MIXUP))
        return stats["loss"], random.random(), np.random.uniform()

    with_hook, without = run(True, **SR.RECIPE), run(False, **SR.RECIPE)
    print(f"fine-tune losses with augment_fn {with_hook[0]}, fed pre-augmented clips {without[0]}")
    assert len(with_hook[0]) == c["micro_batches"] and with_hook == without
    # (the crop does move the loss: the comparison is not vacuous)
    assert run(True, spatial_idx=1, min_scale=size, max_scale=size)[0] != with_hook[0]
