"""RandomErasing on the MI355X: ``tad_erase_clips`` against the reference's changed masks (golden G15) and against the float64
restatement of the documented noise (tests/erasing_recipe.py); the same bits whatever the alignment, the grid and the batch size;
moments of the noise; guard bands around the clip and the box table; no host sync; one fine-tune epoch with ``erase_fn``."""
import functools
import random

import numpy as np
import pytest
import torch

import erasing_recipe as ER
import golden_recipe as R
from guarded import GuardedArena, bits, same_bits
from simple_tad_amd import engine as E
from simple_tad_amd import kernels as K
from simple_tad_amd._lib import ERASE_BOX_WORDS
from simple_tad_amd.random_erasing import RandomErasing
from test_mixup_cpu import _build_tiny

pytestmark = pytest.mark.gpu
CASES = list(ER.cases())
IDS = [c[0] for c in CASES]
# |z| <= sqrt(2 * 24 * ln 2) ~ 5.8 for 24-bit uniforms; four ulp of f32 at that magnitude is 2.8e-6; three chained roundings (logf, sqrtf
# of it, the product with cospif) stay below 1e-5
NOISE_TOL = 1e-5


def _noise_seed(seed):
    """the seed RandomErasing draws for the kernel after torch.manual_seed(seed)"""
    torch.manual_seed(seed)
    return int(torch.randint(0, 2 ** 31 - 1, (1,)).item())


@functools.lru_cache(maxsize=None)
def _erased(key, mode, name, seed, shape):
    """one device run per golden case, shared by the tests below: (input, result, boxes, stream position) on the host"""
    before = ER.clip(key, shape)
    x = before.cuda()
    assert RandomErasing._fused(x)
    fn = RandomErasing(**ER.erasing_kwargs(mode, name))
    random.seed(seed)
    torch.manual_seed(seed)
    out = fn(x)
    after = random.random()
    assert out is x
    random.seed(seed)
    boxes = fn.plan(shape[0], *shape[2:])
    return before, x.cpu(), boxes, after


@pytest.mark.parametrize("key,mode,name,seed,shape", CASES, ids=IDS)
def test_device_erases_exactly_the_reference_mask(golden, key, mode, name, seed, shape):
    g = golden("g15_random_erasing")
    before, got, _, after = _erased(key, mode, name, seed, shape)
    want = torch.from_numpy(ER.unpack_mask(g[f"{key}.mask"], shape))
    changed = bits(got) != bits(before)
    assert torch.equal(changed, want)                  # every element of the mask is rewritten, every other one keeps its bits
    assert after == float(g[f"{key}.next"])
    if mode == "const":
        assert np.array_equal(ER.digest(got), g[f"{key}.sha"]) and np.array_equal(ER.sample(got), g[f"{key}.sample"])


@pytest.mark.parametrize("key,mode,name,seed,shape", CASES, ids=IDS)
def test_device_noise_is_the_documented_generator(key, mode, name, seed, shape):
    """Device values against the float64 restatement of the generator of include/tad_mi355x.h, within NOISE_TOL.  Measured on the
    MI355X: largest deviation 3.7e-7 over the nine cases (pixel.count2.305; const cases 0)."""
    before, got, boxes, _ = _erased(key, mode, name, seed, shape)
    want, own = ER.device_values(boxes, mode, shape, _noise_seed(seed) if mode != "const" else 0)
    inside = own >= 0
    dev = np.abs(got.numpy().astype(np.float64)[inside] - want[inside])
    print(f"erase noise {key}: {int(inside.sum())} elements, max |device - float64 restatement| = {dev.max():.3e}")
    assert dev.max() <= NOISE_TOL
    assert same_bits(got[torch.from_numpy(~inside)], before[torch.from_numpy(~inside)])
    if mode == "rand":
        g = got.numpy()
        seen = 0
        for k, (s, t0, t1, y0, y1, x0, x1) in enumerate(boxes):
            per_frame = []
            for t in range(t0, t1):
                for c in range(shape[1]):
                    mine = g[s, c, t, y0:y1, x0:x1][own[s, c, t, y0:y1, x0:x1] == k]
                    if mine.size:
                        assert (mine == mine[0]).all()                     # one value per (box, frame, channel)
                        per_frame.append((t, c, mine[0]))
            for (ta, ca, va) in per_frame:
                for (tb, cb, vb) in per_frame:
                    if (ta, ca) < (tb, cb):
                        assert va != vb                                     # frames (and channels) of one box differ
                        seen += 1
        assert seen > 0


def _run_table(x_host, table, seed, offset=0, batch=None):
    """tad_erase_clips on a copy of x_host whose base is ``offset`` floats behind a 16-byte boundary, in a batch of ``batch`` clips
    (the extra clips follow x_host's); returns the first len(x_host) clips on the host"""
    B = x_host.shape[0]
    batch = batch or B
    extra = ER.clip("extra", (batch - B,) + tuple(x_host.shape[1:])) if batch > B else x_host[:0]
    whole = torch.cat([x_host, extra])
    flat = torch.cat([torch.full((offset,), 123.0), whole.flatten()]).cuda()
    x = flat[offset:].view(whole.shape)
    assert x.data_ptr() % 16 == (4 * offset) % 16 and x.is_contiguous()
    K.erase_clips(x, table.cuda(), seed)
    res = x.cpu()
    assert offset == 0 or bool((flat[:offset] == 123.0).all())
    assert same_bits(res[B:], extra)
    return res[:B]


@pytest.mark.parametrize("shape", [ER.SQUARE5, ER.WIDE5], ids=["w20", "w22"])
@pytest.mark.parametrize("mode", ["pixel", "rand"])
def test_same_bits_whatever_the_alignment_the_grid_and_the_batch(mode, shape):
    """W = 20 on a 16-byte-aligned base (whole rows of vector groups), the base offset by one float, W = 22 (every row at another
    alignment), a grid forced to ONE workgroup per box (the cap divides ERASE_MAX_BLOCKS = 2048 by the number of rows: trailing rows
    with an unknown mode are ignored but counted) and a batch twice as large: the same bits per element"""
    B, C, Tn, H, W = shape
    random.seed(305)
    boxes = RandomErasing(1.0, max_count=2, num_splits=2, mode=mode).plan(B, Tn, H, W)
    assert len(boxes) >= B + 1
    table = K.erase_box_table([(s, ER.MODE_ID[mode], *rest) for s, *rest in boxes], B, Tn, H, W)
    x_host = ER.clip("align", shape)
    seed = 20240607
    base = _run_table(x_host, table, seed)
    want, own = ER.device_values(boxes, mode, shape, seed)
    inside = own >= 0
    assert inside.any() and np.abs(base.numpy().astype(np.float64)[inside] - want[inside]).max() <= NOISE_TOL
    assert same_bits(base[torch.from_numpy(~inside)], x_host[torch.from_numpy(~inside)])
    for off in (1, 2, 3):
        assert same_bits(_run_table(x_host, table, seed, offset=off), base), off
    ignored = torch.zeros((2048, ERASE_BOX_WORDS), dtype=torch.int32)
    ignored[:, 1] = 7                                   # an unknown mode: no row of these is a box
    assert same_bits(_run_table(x_host, torch.cat([table, ignored]), seed), base)
    assert same_bits(_run_table(x_host, table, seed, batch=2 * B), base)
    assert same_bits(_run_table(x_host, table, seed, offset=1, batch=2 * B), base)


def test_noise_moments():
    """five-sigma bounds on the mean and the variance of the n erased elements"""
    shape = (2, 3, 8, 64, 64)
    x = ER.clip("moments", shape).cuda()
    was = x.clone()
    random.seed(20)
    torch.manual_seed(20)
    RandomErasing(1.0, mode="pixel")(x)
    erased = bits(x) != bits(was)
    z = x[erased].double().cpu().numpy()
    n = z.size
    print(f"erase noise moments: n = {n}, mean = {z.mean():.4e} (bound {5 / np.sqrt(n):.4e}), var - 1 = {z.var() - 1:.4e} "
          f"(bound {5 * np.sqrt(2 / n):.4e}), max |z| = {np.abs(z).max():.3f}")
    assert n >= 4096
    assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2 / n)


# ------------------------------------------------------------------ guard bands
GUARD_CASES = {
    # name: (shape, rows (sample, mode, t0, t1, y0, y1, x0, x1) as given to the kernel, floats the clip's base is offset by)
    "one_box_w20": (ER.SQUARE4, [(1, 2, 0, 4, 3, 11, 5, 14)], 0),
    "borders_w22": (ER.WIDE5, [(0, 2, 0, 5, 0, 7, 0, 9), (3, 1, 2, 5, 11, 18, 13, 22)], 0),
    "overlap_offset": (ER.WIDE4, [(2, 2, 0, 4, 2, 12, 3, 17), (2, 1, 1, 3, 8, 16, 10, 21), (2, 0, 2, 4, 0, 4, 0, 22)], 1),
    "whole_clip_last_sample": (ER.SQUARE4, [(3, 2, 0, 4, 0, 20, 0, 20)], 3),
    "out_of_range_and_unknown": (ER.WIDE5, [(1, 2, -3, 9, 12, 40, -5, 6), (0, 9, 0, 5, 0, 18, 0, 22), (4, 2, 0, 5, 0, 18, 0, 22),
                                            (-1, 2, 0, 5, 0, 18, 0, 22), (2, 1, 3, 1, 2, 9, 4, 8), (3, 2, 4, 5, 17, 18, 21, 22)], 2),
}


def _as_kernel_sees(rows, shape):
    """the rows cut to the clip as load_box of erasing.hip cuts them; an ignored row becomes an empty box (it keeps its index)"""
    B, C, Tn, H, W = shape
    cut = lambda v, lo, hi: min(max(v, lo), hi)
    boxes, modes = [], []
    for s, m, t0, t1, y0, y1, x0, x1 in rows:
        t0, y0, x0 = cut(t0, 0, Tn), cut(y0, 0, H), cut(x0, 0, W)
        t1, y1, x1 = cut(t1, t0, Tn), cut(y1, y0, H), cut(x1, x0, W)
        if m not in (0, 1, 2) or not 0 <= s < B:
            s, t0, t1 = 0, 0, 0
        boxes.append((s, t0, t1, y0, y1, x0, x1))
        modes.append({0: "const", 1: "rand", 2: "pixel"}.get(m, "const"))
    return boxes, modes


@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("case", list(GUARD_CASES))
def test_erase_kernel_stays_inside_its_operands(case, poison):
    shape, rows, offset = GUARD_CASES[case]
    x_host = ER.clip("guard." + case, shape)
    arena = GuardedArena(8 << 20, "cuda", poison=poison)
    flat = arena.place(torch.cat([torch.full((offset,), 123.0), x_host.flatten()]), role="inout", name="clips")
    x = flat[offset:].view(shape)
    assert x.data_ptr() % 16 == (4 * offset) % 16 and x.is_contiguous()
    table = torch.tensor(rows, dtype=torch.int32)
    assert tuple(table.shape) == (len(rows), ERASE_BOX_WORDS)
    # guards of the table hold words in [0, 3): rows read past its end would be boxes of samples 0..2 and show in the result
    boxes_dev = arena.place(table, role="input", name="boxes", index_range=3)
    seed = 77
    with arena.route(K):
        K.erase_clips(x, boxes_dev, seed)
    arena.verify()
    boxes, modes = _as_kernel_sees(rows, shape)
    want, own = ER.device_values(boxes, modes, shape, seed)
    inside = own >= 0
    got = x.cpu()
    assert inside.any() and np.abs(got.numpy().astype(np.float64)[inside] - want[inside]).max() <= NOISE_TOL
    assert same_bits(got[torch.from_numpy(~inside)], x_host[torch.from_numpy(~inside)])
    assert offset == 0 or bool((flat[:offset] == 123.0).all())


# ------------------------------------------------------------------ host side
@pytest.mark.parametrize("mode", ["const", "rand", "pixel"])
def test_erasing_call_does_not_synchronise_with_the_host(mode):
    x = ER.clip("nosync", (8, 3, 4, 16, 16)).cuda()
    fn = RandomErasing(0.5, mode=mode, max_count=2)
    random.seed(3)
    fn(x)               # (first call: library load, allocator warm-up)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):     # the mode is live in this build: a host read of device memory is refused
            x.sum().item()
        for _ in range(6):
            fn(x)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


def test_a_batch_without_a_box_launches_nothing_and_still_draws_the_seed():
    x = ER.clip("nobox", (4, 3, 4, 16, 16)).cuda()
    was = x.clone()
    calls = []
    saved = K.erase_clips
    K.erase_clips = lambda *a, **k: calls.append(a) or saved(*a, **k)
    try:
        torch.manual_seed(5)
        RandomErasing(0.0, mode="pixel")(x)
        drawn = torch.randint(0, 100, (1,)).item()
        torch.manual_seed(5)
        torch.randint(0, 2 ** 31 - 1, (1,))
        assert drawn == torch.randint(0, 100, (1,)).item()      # one seed draw, whatever the plan
        torch.manual_seed(5)
        RandomErasing(0.0, mode="const")(x)
        torch.manual_seed(5)
        first = torch.randint(0, 100, (1,)).item()
        torch.manual_seed(5)
        RandomErasing(1.0, mode="const")(x.clone())
        assert torch.randint(0, 100, (1,)).item() == first      # const draws nothing
    finally:
        K.erase_clips = saved
    assert len(calls) == 1 and torch.equal(x, was)


# ------------------------------------------------------------------ the fine-tune loop
def _tiny_epoch(batches, erase_fn):
    c = R.G12
    m = _build_tiny("cuda", torch.float32)
    opt = E.create_optimizer(m, lr=c["base_lr"], weight_decay=c["weight_decay"], layer_decay=c["layer_decay"])
    lr_sched = E.cosine_scheduler(c["base_lr"], c["min_lr"], 1, c["steps"], warmup_epochs=c["warmup_epochs"],
                                  start_warmup_value=c["start_warmup_value"], warmup_steps=c["warmup_steps"])
    return E.train_one_epoch(m, torch.nn.CrossEntropyLoss(), batches, opt, torch.device("cuda"), 0, E.NativeScalerWithGradNormCount(m),
                             max_norm=c["clip_grad"], start_steps=0, lr_schedule_values=lr_sched, num_training_steps_per_epoch=c["steps"],
                             update_freq=c["update_freq"], erase_fn=erase_fn, mixup_fn=None)


def test_train_one_epoch_with_erase_fn_equals_the_run_on_clips_erased_beforehand():
    kw = dict(probability=1.0, mode="const", max_area=0.1)
    random.seed(15)
    on_device = _tiny_epoch(R.g12_batches(), RandomErasing(**kw))
    after = random.random()
    cpu_fn = RandomErasing(**kw)
    random.seed(15)
    erased = []
    for x, y, a, b in R.g12_batches():
        was = x.clone()
        assert cpu_fn(x) is x and not torch.equal(x, was)
        erased.append((x, y, a, b))
    assert random.random() == after
    beforehand = _tiny_epoch(erased, None)
    assert len(on_device["loss"]) == len(erased) and on_device["loss"] == beforehand["loss"]
    plain = _tiny_epoch(R.g12_batches(), None)
    assert plain["loss"] != on_device["loss"]                   # (the erased boxes do move the loss: the comparison is not vacuous)
