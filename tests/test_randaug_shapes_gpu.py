"""RandAugment on the MI355X beyond the fixture's 3 x 2 x 20 x 23: the paths of csrc/randaug.hip that 460 pixels per frame and 6 frames
per batch never run -- second and later trips of every grid-stride loop and the grid cap of one workgroup per frame, Equalize with a
step above 1, the high word of the resample mask, layer counts 0, 2, 4 and 32 with statistics layers in a row, frames below 3 pixels in
a direction, frame bases of all 16 residues inside one launch.

Every comparison is bit for bit against ``RR.apply`` / ``RR.apply_rows`` (tests/randaug_recipe.py, numpy, computed here), which
tests/test_randaug_shapes_cpu.py holds to PIL at these frame sizes (fixture G25); there is no allowance of differing bytes, and every
test checks that the input is unchanged."""
import functools

import numpy as np
import pytest
import torch

import randaug_recipe as RR
import simple_tad_amd.rand_augment as RA
from guarded import GuardedArena, same_bits
from simple_tad_amd import kernels as K
from test_randaug_gpu import MEAN, STD, reference_clip

pytestmark = pytest.mark.gpu
OP_CASES = RR.op_cases()
CASE = {c[0]: c for c in OP_CASES}
SMALL = tuple(s for s in RR.SHAPES if s[:2] == (2, 3))
REAL, MID = (1, 2, 224, 224), (2, 2, 45, 80)
CAPPED = (33, 64, 67, 63)                     # B * T = 2112: 4096 / (B * T) == 1 workgroup per frame; 12663-byte frames
CAPPED_CLIPS = (0, 16, 32)                    # the clips that carry the op; the other 30 carry a not-applied row
MASKED = (1, 64, 9, 11)
LAYERED = ((3, 2, 20, 23), (2, 2, 67, 63))


@functools.lru_cache(maxsize=None)
def frames_at(shape):
    return torch.from_numpy(RR.frames_at(*shape, RR.SHAPES_SEED))


@pytest.fixture(scope="module")
def args(golden):
    """{case key: the argument the reference's level function returned}; the same at every shape (test_randaug_shapes_cpu.py)"""
    return RR.golden_args(golden("g25_rand_augment_shapes"), REAL)


def rows_of(name, arg, resample, B, clips=None, layer=0):
    """one plan row per clip for layer ``layer``: the op on ``clips`` (default: all), a failed coin on the others; resample: one
    filter or one per frame"""
    geo = name in RA.GEOMETRIC
    return [RA.PlanRow(b, layer, RA.OP_NAMES.index(name), True, arg, tuple(resample) if geo else None) if clips is None or b in clips
            else RA.PlanRow(b, layer, RA.OP_NAMES.index(name), False, None, None) for b in range(B)]


def run(host, rows, num_layers=1, names=None, offset=0):
    """the plan on a device copy of ``host`` (its base ``offset`` bytes behind a 256-byte boundary); checks that the input is unchanged"""
    names = names or sorted({RA.OP_NAMES[r.op] for r in rows}) or ["Invert"]
    ra = RA.RandAugment([RA.AugmentOp(n, prob=1.0) for n in names], num_layers=num_layers)
    flat = torch.cat([torch.full((offset,), 99, dtype=torch.uint8), host.flatten()]).cuda()
    x = flat[offset:].view(host.shape)
    assert x.data_ptr() % 16 == offset and x.is_contiguous()
    out = ra.apply(x, rows)
    assert out.dtype == torch.uint8 and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    assert torch.equal(flat[offset:].cpu().view(host.shape), host) and bool((flat[:offset] == 99).all())
    return x, out


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8
    bad = got != want
    print(f"randaug {what}: {int(bad.sum())} of {bad.size} bytes differ from the recipe")
    if bad.any():
        where = np.argwhere(bad)
        d = np.abs(got.astype(np.int16) - want.astype(np.int16))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} bytes differ (largest difference {int(d.max())}); first at "
                             f"{tuple(where[0])}: {got[tuple(where[0])]} for {want[tuple(where[0])]}, last at {tuple(where[-1])}")


def recipe(host, name, arg, resample, clips=None):
    """RR.apply on every frame of ``clips`` (default: all): uint8 [len(clips), T, H, W, 3]; resample: one filter per frame"""
    x = host.numpy()
    clips = range(x.shape[0]) if clips is None else clips
    return np.stack([np.stack([RR.apply(x[b, t], name, arg, resample[t]) for t in range(x.shape[1])]) for b in clips])


# ------------------------------------------------------------------ a. small and degenerate frames, b. a real frame, c. a mid size
@pytest.mark.parametrize("key", list(CASE))
def test_every_op_on_small_and_degenerate_frames(args, key):
    """B, T = 2, 3 at 1x1, 1x7, 7x1, 2x2, 3x3, 2x9, 3x40: every Sharpness pixel is border below 3 pixels in a direction, H * W < 16 is
    one short pointwise item, a single row / column goes through the affine clamps, frame bases are 3 * H * W apart (every residue)"""
    _, name, m, seed, rs = CASE[key]
    for shape in SMALL:
        host = frames_at(shape)
        _, out = run(host, rows_of(name, args[key], (rs,) * shape[1], shape[0]))
        assert_same(out.cpu().numpy(), recipe(host, name, args[key], (rs,) * shape[1]), f"{key} at {RR.shape_key(shape)}")


@pytest.mark.parametrize("key", list(CASE))
def test_every_op_on_a_real_frame(args, key):
    """1 x 2 x 224 x 224, 196 workgroups per frame (the cap does not bind): Equalize's step is 167 .. 194, so its start value step / 2
    matters, and the entry of the last occupied level is 256 before the cut on some channels and 255 on others"""
    _, name, m, seed, rs = CASE[key]
    host = frames_at(REAL)
    _, out = run(host, rows_of(name, args[key], (rs,) * 2, 1))
    assert_same(out.cpu().numpy(), recipe(host, name, args[key], (rs,) * 2), key)


MID_KEYS = [k for k, c in CASE.items() if c[1] in RR.GEOMETRIC or c[1] in ("Sharpness", "SharpnessIncreasing", "Equalize")]


@pytest.mark.parametrize("key", MID_KEYS)
def test_neighbourhood_ops_on_a_non_square_mid_size(args, key):
    """2 x 2 x 45 x 80: W > H, rows of 240 bytes, 10800-byte frames (bases 0 and 8 mod 16); Equalize's step is 0 (the two-level channel) or 11 .. 13"""
    _, name, m, seed, rs = CASE[key]
    host = frames_at(MID)
    _, out = run(host, rows_of(name, args[key], (rs,) * 2, 2))
    assert_same(out.cpu().numpy(), recipe(host, name, args[key], (rs,) * 2), key)


# ------------------------------------------------------------------ d. the capped grid
MIXED = tuple(RR.BICUBIC if t % 3 == 0 else RR.BILINEAR for t in range(CAPPED[1]))     # both mask words are mixed
CAPPED_OPS = (("not-applied", "op.Invert.m5", None), ("Solarize", "op.Solarize.m7", None), ("Equalize", "op.Equalize.m5", None),
              ("AutoContrast", "op.AutoContrast.m5", None), ("Contrast", "op.Contrast.m9", None), ("Color", "op.Color.m2", None),
              ("Sharpness", "op.Sharpness.m9", None), ("Rotate", "op.Rotate.m6.pos.bicubic", MIXED),
              ("TranslateXRel", "op.TranslateXRel.m6.neg.bilinear", None))


def test_the_capped_shape_is_what_the_tests_say():
    B, T, H, W = CAPPED
    HW = H * W
    assert 4096 // (B * T) == 1 and 4096 // ((B - 1) * T) == 2 and T == 64          # the smallest batch of 64-frame clips with a cap of 1
    assert -(-HW // 256) == 17 and HW % 256                                         # 17 ragged trips of the per-pixel loops
    assert -(-HW // 16) == 264 and HW % 16 == 13                                    # pointwise: two trips, the last item 13 pixels
    assert {-(-((HW * 3 - head) // 16) // 256) for head in range(16)} == {4}        # histogram: four trips over ~790 vectors
    assert {(f * HW * 3) % 16 for f in range(B * T)} == set(range(16))              # every base residue inside one launch
    assert {((b * T + t) * HW * 3) % 16 for b in CAPPED_CLIPS for t in range(T)} == set(range(16))    # ... and among the compared clips
    x = frames_at(CAPPED).numpy()
    assert {RR.kind_of(b, t, T) for b in CAPPED_CLIPS for t in range(T)} == set(RR.KINDS)
    steps = {(HW - int(h[np.nonzero(h)[0][-1]])) // 255 for b in CAPPED_CLIPS for t in range(T) for h in RR._histograms(x[b, t])}
    assert 0 in steps and max(steps) >= 14, steps


@pytest.mark.parametrize("label,key,resample", CAPPED_OPS, ids=[o[0] for o in CAPPED_OPS])
def test_one_workgroup_per_frame_strides_over_the_whole_frame(args, label, key, resample):
    """33 x 64 x 67 x 63: gridDim.x == 1, so every loop of the apply kernel runs its later trips (17 per pixel, 2 per pointwise item, 4
    per histogram vector); the op on clips 0, 16 and 32 against the recipe, the other 30 clips must come out as they went in"""
    B, T, H, W = CAPPED
    _, name, m, seed, rs = CASE[key]
    resample = resample or (rs,) * T
    clips = () if label == "not-applied" else CAPPED_CLIPS
    host = frames_at(CAPPED)
    x, out = run(host, rows_of(name, args[key], resample, B, clips))
    others = [b for b in range(B) if b not in clips]
    assert torch.equal(out[others], x[others])
    if clips:
        want = recipe(host, name, args[key], resample, clips)
        assert (want != host.numpy()[list(clips)]).reshape(len(clips) * T, -1).any(1).sum() > len(clips) * T // 2   # (most frames change)
        if name == "TranslateXRel":
            assert (want.reshape(-1, 3) == RR.FILL).all(1).mean() > 0.2                                              # the fill region appears
        assert_same(out[list(clips)].cpu().numpy(), want, f"{label} at {RR.shape_key(CAPPED)}")


def test_frames_to_clip_with_one_workgroup_per_frame():
    """1056 items of four pixels per frame: five trips, the last item one pixel; planes of 64 * 4221 floats (a multiple of four),
    frame bases of every residue mod 4, so the vector and the scalar path alternate inside the launch"""
    host = frames_at(CAPPED)
    x = host.cuda()
    got = RA.frames_to_clip(x, MEAN, STD)
    assert torch.equal(x.cpu(), host)
    assert got.dtype == torch.float32 and same_bits(got.cpu(), reference_clip(host))


# ------------------------------------------------------------------ e. the resample mask
MASKS = ((31,), (32,), (63,), (0, 31, 32, 63), tuple(range(64)), ())


@pytest.mark.parametrize("bicubic", MASKS, ids=lambda m: ",".join(map(str, m)) if 0 < len(m) < 9 else ("all" if m else "none"))
def test_every_frame_reads_its_own_bit_of_the_resample_mask(args, bicubic):
    B, T, H, W = MASKED
    key = "op.Rotate.m6.pos.bicubic"
    host = frames_at(MASKED)
    resample = tuple(RR.BICUBIC if t in bicubic else RR.BILINEAR for t in range(T))
    both = [recipe(host, "Rotate", args[key], (rs,) * T)[0] for rs in (RR.BILINEAR, RR.BICUBIC)]
    assert all((both[0][t] != both[1][t]).any() for t in range(T))              # a wrong bit cannot pass on any frame
    _, out = run(host, rows_of("Rotate", args[key], resample, B))
    assert_same(out.cpu().numpy(), recipe(host, "Rotate", args[key], resample), f"Rotate with frames {bicubic or 'none'} bicubic")


# ------------------------------------------------------------------ f. layer counts
CHAIN = (("Equalize", "op.Equalize.m5", None), ("ContrastIncreasing", "op.ContrastIncreasing.m6.pos", None),
         ("AutoContrast", "op.AutoContrast.m5", None), ("Sharpness", "op.Sharpness.m9", None),
         ("Rotate", "op.Rotate.m6.pos.bicubic", RR.BICUBIC), ("SolarizeAdd", "op.SolarizeAdd.m3", None), ("Color", "op.Color.m9", None),
         ("ShearX", "op.ShearX.m6.neg.bilinear", RR.BILINEAR))
# statistics ops in layers 0 and 31 only (Contrast last: it changes every frame, whatever the 31 layers before it left)
ENDS = (CHAIN[0],) + tuple(CHAIN[3 + l % 5] for l in range(30)) + (CHAIN[1],)


def chain_rows(args, ops, shape, n_layers, shift):
    """clip b runs ops[(l + shift * b) % len(ops)] in layer l: with shift = 1 the clips of a layer carry out different operators"""
    B, T = shape[:2]
    rows = []
    for b in range(B):
        for l in range(n_layers):
            name, key, rs = ops[(l + shift * b) % len(ops)]
            rows.append(RA.PlanRow(b, l, RA.OP_NAMES.index(name), True, args[key], (rs,) * T if rs else None))
    return rows


def check_plan(host, rows, n_layers, stats=None, what=""):
    names = [c[0] for c in CHAIN]
    if stats is not None:
        ra = RA.RandAugment([RA.AugmentOp(n, prob=1.0) for n in names], num_layers=n_layers)
        assert ra.table(rows, *host.shape[:4])[1] == stats
    _, out = run(host, rows, n_layers, names)
    plain = lambda rr: [(r.clip, r.op, r.applied, r.arg, r.resample) for r in rr]
    want = RR.apply_rows(host.numpy(), plain(rows), RA.OP_NAMES)
    if n_layers:                                # the last layer changes every clip: the result of the layer before it cannot pass
        before = RR.apply_rows(host.numpy(), plain(r for r in rows if r.layer < n_layers - 1), RA.OP_NAMES)
        assert all((want[b] != before[b]).any() for b in range(host.shape[0]))
    assert_same(out.cpu().numpy(), want, what)
    return want


@pytest.mark.parametrize("shape", LAYERED, ids=RR.shape_key)
@pytest.mark.parametrize("n_layers", [0, 2, 4, 32])
def test_layer_counts_and_statistics_layers_in_a_row(args, shape, n_layers):
    """0: the copy arm (a new tensor); an even count: the first layer writes the workspace buffer; 32: bit 31 of the statistics mask.
    Equalize, Contrast and AutoContrast follow one another on a clip: each takes its statistics from the layer's source buffer"""
    host = frames_at(shape)
    rows = chain_rows(args, CHAIN, shape, n_layers, shift=1)
    stats = sum(1 << l for l in range(n_layers) if any((l + b) % 8 < 3 for b in range(shape[0])))
    want = check_plan(host, rows, n_layers, stats, f"{n_layers} layers at {RR.shape_key(shape)}")
    if n_layers == 0:
        assert np.array_equal(want, host.numpy())
    else:
        # statistics of the input instead of the layer's source would show: Contrast's mean after Equalize is not the input's
        x = host.numpy()
        assert all(RR.l_mean(RR.apply(x[0, t], "Equalize", None)) != RR.l_mean(x[0, t]) for t in range(shape[1]))


@pytest.mark.parametrize("shape", LAYERED, ids=RR.shape_key)
def test_32_layers_with_statistics_in_the_first_and_the_last_only(args, shape):
    host = frames_at(shape)
    want = check_plan(host, chain_rows(args, ENDS, shape, 32, shift=0), 32, 0x80000001, f"32 layers (statistics in 0 and 31) at {RR.shape_key(shape)}")
    assert all(len(np.unique(want[b, t])) > 8 for b in range(shape[0]) for t in range(shape[1]))     # (the frames are still pictures)


# ------------------------------------------------------------------ g. guard bands
def guarded(host, ra, rows, poison, offset, nbytes):
    B, T, H, W = host.shape[:4]
    table, stats = ra.table(rows, B, T, H, W)
    arena = GuardedArena(nbytes, "cuda", poison=poison)
    flat = arena.place(torch.cat([torch.full((offset,), 99, dtype=torch.uint8), host.flatten()]), role="input", name="frames")
    x = flat[offset:].view(host.shape)
    # guards of the table hold words in [0, 2): rows read past its end would be valid rows of the clips 0 and 1 and show in the result
    tab = arena.place(table, role="input", name="table", index_range=2)
    with arena.route(K):
        out = K.randaug_apply(x, tab, stats)
    arena.verify()                                                                  # (the input's body is among the bytes that must not change)
    assert arena.contains(out)
    return x, out


@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("offset", [0, 3])
@pytest.mark.parametrize("label", ["Equalize", "Rotate"])
def test_capped_launches_stay_inside_their_operands(args, label, poison, offset):
    B, T = CAPPED[:2]
    _, key, resample = next(o for o in CAPPED_OPS if o[0] == label)
    _, name, m, seed, rs = CASE[key]
    resample = (RR.BICUBIC,) * T if label == "Rotate" else (rs,) * T
    host = frames_at(CAPPED)
    ra = RA.RandAugment([RA.AugmentOp(name, prob=1.0)], num_layers=1)
    x, out = guarded(host, ra, rows_of(name, args[key], resample, B, CAPPED_CLIPS), poison, offset, 80 << 20)
    others = [b for b in range(B) if b not in CAPPED_CLIPS]
    assert torch.equal(out[others], x[others])
    clips = (CAPPED_CLIPS[0], CAPPED_CLIPS[-1])                                     # (the first and the last: the neighbours of the guards)
    assert_same(out[list(clips)].cpu().numpy(), recipe(host, name, args[key], resample, clips), f"{label} guarded {poison} +{offset}")


@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("offset", [0, 3])
def test_four_layers_stay_inside_their_operands(args, poison, offset):
    shape = LAYERED[1]
    host = frames_at(shape)
    rows = chain_rows(args, CHAIN, shape, 4, shift=1)
    ra = RA.RandAugment([RA.AugmentOp(c[0], prob=1.0) for c in CHAIN], num_layers=4)
    _, out = guarded(host, ra, rows, poison, offset, 8 << 20)
    want = RR.apply_rows(host.numpy(), [(r.clip, r.op, r.applied, r.arg, r.resample) for r in rows], RA.OP_NAMES)
    assert_same(out.cpu().numpy(), want, f"4 layers guarded {poison} +{offset}")
