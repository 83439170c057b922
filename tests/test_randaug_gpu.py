"""RandAugment on the MI355X: ``tad_randaug_apply`` against PIL's frames (golden G16: every per-op and policy case) at the fixture's one
shape 3 x 2 x 20 x 23; the same bits whatever the base alignment and the batch; ``frames_to_clip`` against the torch CPU expression
of the reference's three steps; guard bands around every operand; no host sync."""
import functools
import random

import numpy as np
import pytest
import torch

import randaug_recipe as RR
import simple_tad_amd.rand_augment as RA
from guarded import GuardedArena, same_bits
from simple_tad_amd import kernels as K
from test_randaug_cpu import policy_transform

pytestmark = pytest.mark.gpu
OP_CASES = RR.op_cases()
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# an op outside RR.EXACT (none at present: the device equals PIL on every op) may differ by 1 in at most 0.1 % of a case's bytes
MAX_SHARE = 0.001


@functools.lru_cache(maxsize=None)
def frames():
    return torch.from_numpy(RR.frames())


def forced(name, arg, rs, clips=RR.B):
    """(RandAugment of the one op, plan rows that apply it to every clip)"""
    ra = RA.RandAugment([RA.AugmentOp(name, prob=1.0)], num_layers=1)
    resample = (rs,) * RR.T if name in RA.GEOMETRIC else None
    return ra, [RA.PlanRow(b, 0, RA.OP_NAMES.index(name), True, arg, resample) for b in range(clips)]


def golden_arg(g, key, name):
    arg = float(g[f"{key}.arg"])
    return None if np.isnan(arg) else (int(arg) if name.startswith(("Posterize", "Solarize")) else arg)


def compare(got, want, exact, what):
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    share = float((d != 0).mean())
    print(f"randaug {what}: {int((d != 0).sum())} of {d.size} bytes differ from PIL (share {share:.5f}), largest difference {int(d.max())}")
    if exact:
        assert d.max() == 0
    else:
        assert d.max() <= 1 and share <= MAX_SHARE


@pytest.mark.parametrize("key,name,m,seed,rs", OP_CASES, ids=[c[0] for c in OP_CASES])
def test_every_op_equals_pil(golden, key, name, m, seed, rs):
    g = golden("g16_rand_augment")
    ra, rows = forced(name, golden_arg(g, key, name), rs)
    x = frames().cuda()
    out = ra.apply(x, rows)
    assert out.dtype == torch.uint8 and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    assert torch.equal(x.cpu(), frames())                                  # the input is only read
    compare(out.cpu().numpy(), g[f"{key}.out"], name in RR.EXACT, key)


@pytest.mark.parametrize("key,seed,oplist,interp", RR.POLICIES, ids=[p[0] for p in RR.POLICIES])
def test_every_policy_case_equals_pil_through_the_seeded_call(golden, key, seed, oplist, interp):
    g = golden("g16_rand_augment")
    ra = policy_transform(oplist, interp)
    random.seed(seed)
    np.random.seed(seed)
    out = ra(frames().cuda())
    assert random.random() == float(g[f"{key}.next_py"]) and np.random.random() == float(g[f"{key}.next_np"])
    exact = all(n in RR.EXACT for n, a in zip(g[f"{key}.ops"], g[f"{key}.applied"]) if a)
    compare(out.cpu().numpy(), g[f"{key}.out"], exact, key)


def test_a_single_clip_is_a_batch_of_one(golden):
    g = golden("g16_rand_augment")
    key, name, m, seed, rs = next(c for c in OP_CASES if c[1] == "Equalize")
    ra, rows = forced(name, None, rs, clips=1)
    out = ra.apply(frames()[1].cuda(), rows)
    assert tuple(out.shape) == (RR.T, RR.H, RR.W, 3) and np.array_equal(out.cpu().numpy(), g[f"{key}.out"][1])


VARIATION_OPS = ("AutoContrast", "Equalize", "Solarize", "ContrastIncreasing", "Color", "Sharpness", "Rotate", "ShearX")


@pytest.mark.parametrize("name", VARIATION_OPS)
def test_same_bits_whatever_the_base_offset_and_the_batch(golden, name):
    g = golden("g16_rand_augment")
    key, _, m, seed, rs = [c for c in OP_CASES if c[1] == name][-1]
    arg = golden_arg(g, key, name)
    ra, rows = forced(name, arg, rs)
    base = ra.apply(frames().cuda(), rows).cpu()
    for off in (1, 2, 3):                                                   # the input's base 1..3 bytes behind an aligned address
        flat = torch.cat([torch.full((off,), 99, dtype=torch.uint8), frames().flatten()]).cuda()
        x = flat[off:].view(frames().shape)
        assert x.data_ptr() % 16 == off and x.is_contiguous()
        assert torch.equal(ra.apply(x, rows).cpu(), base), off
        assert torch.equal(flat.cpu()[off:].view(frames().shape), frames()) and bool((flat[:off] == 99).all())
    twice = torch.cat([frames(), frames()]).cuda()                         # the three clips twice under the same plan rows
    ra6, rows6 = forced(name, arg, rs, clips=2 * RR.B)
    out = ra6.apply(twice, rows6).cpu()
    assert torch.equal(out[:RR.B], base) and torch.equal(out[RR.B:], base) and torch.equal(twice.cpu()[:RR.B], frames())


# ------------------------------------------------------------------ frames_to_clip
def reference_clip(x):
    """torchvision's ToTensor (x.float().div(255)), the reference's tensor_normalize ((v - mean) / std over [...,3]) and its permute"""
    v = x.to(torch.float32).div(255)
    v = (v - torch.tensor(MEAN)) / torch.tensor(STD)
    return v.permute(0, 4, 1, 2, 3).contiguous()


def test_frames_to_clip_equals_the_torch_expression_bit_for_bit():
    x = frames()
    want = reference_clip(x)
    got = RA.frames_to_clip(x.cuda(), MEAN, STD)
    assert got.dtype == torch.float32 and tuple(got.shape) == (RR.B, 3, RR.T, RR.H, RR.W) and same_bits(got.cpu(), want)
    for off in (1, 3):                                                      # input offset by bytes, output by floats
        flat = torch.cat([torch.full((off,), 99, dtype=torch.uint8), x.flatten()]).cuda()
        xo = flat[off:].view(x.shape)
        buf = torch.full((want.numel() + off,), 7.0, device="cuda")
        out = buf[off:].view(want.shape)
        assert xo.data_ptr() % 4 == off and out.data_ptr() % 16 == 4 * off
        assert RA.frames_to_clip(xo, MEAN, STD, out=out) is out and same_bits(out.cpu(), want) and bool((buf[:off] == 7.0).all())
    odd = x[:, :, :19, :21].contiguous()                                    # 19 x 21: planes that are no multiple of four floats
    assert same_bits(RA.frames_to_clip(odd.cuda(), MEAN, STD).cpu(), reference_clip(odd))


def test_the_converted_clip_is_what_random_erasing_and_mixup_take():
    from simple_tad_amd.mixup import Mixup
    from simple_tad_amd.random_erasing import RandomErasing
    clip = RA.frames_to_clip(torch.cat([frames(), frames()[:1]]).cuda(), MEAN, STD)
    assert RandomErasing._fused(clip)
    random.seed(2)
    assert RandomErasing(1.0, mode="const")(clip) is clip
    np.random.seed(2)
    mixed, target = Mixup(mixup_alpha=0.8, num_classes=4)(clip, torch.tensor([0, 1, 2, 3], device="cuda"))
    assert mixed.shape == clip.shape and tuple(target.shape) == (4, 4)


# ------------------------------------------------------------------ guard bands
GUARD_POLICIES = ("policy.drive.1", "policy.default.9", "policy.random.3")


@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("key", GUARD_POLICIES)
@pytest.mark.parametrize("offset", [0, 3])
def test_randaug_kernels_stay_inside_their_operands(golden, key, poison, offset):
    g = golden("g16_rand_augment")
    _, seed, oplist, interp = next(p for p in RR.POLICIES if p[0] == key)
    ra = policy_transform(oplist, interp)
    random.seed(seed)
    np.random.seed(seed)
    table, stats = ra.table(ra.plan(RR.B, RR.T), RR.B, RR.T, RR.H, RR.W)
    arena = GuardedArena(8 << 20, "cuda", poison=poison)
    flat = arena.place(torch.cat([torch.full((offset,), 99, dtype=torch.uint8), frames().flatten()]), role="input", name="frames")
    x = flat[offset:].view(frames().shape)
    # guards of the table hold words in [0, 3): rows read past its end would be valid rows of the clips 0..2 and show in the result
    tab = arena.place(table, role="input", name="table", index_range=3)
    with arena.route(K):
        out = K.randaug_apply(x, tab, stats)
    arena.verify()
    assert arena.contains(out)
    exact = all(n in RR.EXACT for n, a in zip(g[f"{key}.ops"], g[f"{key}.applied"]) if a)
    compare(out.cpu().numpy(), g[f"{key}.out"], exact, f"{key} guarded {poison} +{offset}")


@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("offset", [0, 1])
def test_frames_to_clip_stays_inside_its_operands(poison, offset):
    arena = GuardedArena(8 << 20, "cuda", poison=poison)
    flat = arena.place(torch.cat([torch.full((offset,), 99, dtype=torch.uint8), frames().flatten()]), role="input", name="frames")
    x = flat[offset:].view(frames().shape)
    with arena.route(K):
        out = K.frames_to_clip(x, MEAN, STD)
    arena.verify()
    assert arena.contains(out) and same_bits(out.cpu(), reference_clip(frames()))


def test_unknown_rows_are_ignored_on_the_device(golden):
    """rows the host check would refuse: an unknown op copies its clip, a sample outside the batch does nothing; the valid row of the
    layer is carried out and nothing outside the operands is written"""
    g = golden("g16_rand_augment")
    ra, rows = forced("Invert", None, RR.BILINEAR)
    table, stats = ra.table(rows, RR.B, RR.T, RR.H, RR.W)
    table[0, 1, 1] = 77
    table[0, 2, 0] = 5
    arena = GuardedArena(8 << 20, "cuda")
    x = arena.place(frames(), role="input", name="frames")
    tab = arena.place(table, role="input", name="table", index_range=3)
    with arena.route(K):
        out = K.randaug_apply(x, tab, stats)
    arena.verify()
    assert np.array_equal(out[0].cpu().numpy(), g["op.Invert.m5.out"][0]) and torch.equal(out[1].cpu(), frames()[1])


# ------------------------------------------------------------------ host side
def test_call_does_not_synchronise_with_the_host():
    ra = policy_transform("drive", None)
    x = frames().cuda()
    random.seed(3)
    np.random.seed(3)
    RA.frames_to_clip(ra(x), MEAN, STD)               # (first call: library load, allocator warm-up)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):             # the mode is live in this build: a host read of device memory is refused
            x.sum().item()
        for _ in range(6):
            RA.frames_to_clip(ra(x), MEAN, STD)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
