"""RandAugment beyond the one shape of fixture G16, without a GPU: the numpy restatement of every operator (tests/randaug_recipe.py)
against the SHA-256 of PIL's output frames at the shapes of fixture G25 (tools/make_goldens_randaug_shapes.py) -- what licenses
``RR.apply`` as the reference of tests/test_randaug_shapes_gpu.py; that the seeded inputs reach the arithmetic those tests are about;
and the table words the fixture shape never sets (frames 31, 32 and 63 of the resample mask, layer 31 of the statistics mask)."""
import functools

import numpy as np
import pytest

import randaug_recipe as RR
import simple_tad_amd.rand_augment as RA

OP_CASES = RR.op_cases()
REAL = (1, 2, 224, 224)


@pytest.fixture(scope="module")
def g25(golden):
    g = golden("g25_rand_augment_shapes")
    assert [tuple(s) for s in g["shapes"]] == list(RR.SHAPES) and int(g["seed"]) == RR.SHAPES_SEED
    return g


@functools.lru_cache(maxsize=None)
def frames_at(shape):
    x = RR.frames_at(*shape, RR.SHAPES_SEED)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def recipe_outputs(shape, args):
    """{case key: RR.apply on every frame of the shape}, computed once (args: the (key, argument) pairs of the shape)"""
    x, args = frames_at(shape), dict(args)
    return {key: np.stack([np.stack([RR.apply(x[b, t], name, args[key], rs) for t in range(shape[1])]) for b in range(shape[0])])
            for key, name, m, seed, rs in OP_CASES}


def outputs(g25, shape):
    return recipe_outputs(shape, tuple(RR.golden_args(g25, shape).items()))


# ------------------------------------------------------------------ the restatement against PIL at every shape
@pytest.mark.parametrize("shape", RR.SHAPES, ids=RR.shape_key)
def test_numpy_restatement_equals_pil_at_every_shape(g25, shape):
    sk = RR.shape_key(shape)
    x = frames_at(shape)
    assert x.shape == shape + (3,) and x.dtype == np.uint8 and np.array_equal(RR.digest(x), g25[f"{sk}.input.sha"])
    assert np.array_equal(RR.frames_at(*shape, RR.SHAPES_SEED), x)                       # seeded: the same frames again
    out, want = outputs(g25, shape), g25[f"{sk}.sha"]
    assert want.shape == (len(OP_CASES),) + shape[:2] + (32,)
    wrong = [(c[0], b, t) for k, c in enumerate(OP_CASES) for b in range(shape[0]) for t in range(shape[1])
             if not np.array_equal(RR.digest(out[c[0]][b, t]), want[k, b, t])]
    assert not wrong, f"{len(wrong)} frames differ from PIL's: {wrong[:8]}"


def test_arguments_do_not_depend_on_the_shape(g25):
    """(every level function of the policy is relative: the GPU tests may take a case's argument at any shape)"""
    first = g25[f"{RR.shape_key(RR.SHAPES[0])}.args"]
    assert first.shape == (len(OP_CASES),) and all(np.array_equal(g25[f"{RR.shape_key(s)}.args"], first, equal_nan=True) for s in RR.SHAPES)
    for name in RR.NEGATING:
        args = [a for c, a in zip(OP_CASES, first) if c[1] == name]
        pivot = 1.0 if name.endswith("Increasing") else 0.0
        assert min(args) < pivot < max(args)


# ------------------------------------------------------------------ the inputs reach what the tests are about
def test_frame_kinds_are_what_they_say():
    for shape in RR.SHAPES + ((3, 5, 67, 63),):
        B, T, H, W = shape
        x = frames_at(shape)
        seen = set()
        for b in range(B):
            for t in range(T):
                f, kind = x[b, t], RR.kind_of(b, t, T)
                seen.add(kind)
                if kind == "full" and H * W >= 2:
                    assert all((f[..., c].min(), f[..., c].max()) == (0, 255) for c in range(3))
                if kind == "constant":
                    assert f[..., 1].min() == f[..., 1].max()
                if kind == "two-level" and H * W >= 2:
                    h = RR._histograms(f)[2]
                    assert np.count_nonzero(h) == 2 and h[np.nonzero(h)[0][-1]] > H * W - 255
                    if H * W >= 256:                       # Equalize's step is 0 on a frame that is far from constant
                        assert (H * W - h[np.nonzero(h)[0][-1]]) // 255 == 0 and RR.equalize_lut(h) == list(range(256))
                        assert RR.autocontrast_lut(h) != list(range(256))
                if kind == "gradient" and H * W >= 64:
                    assert all(np.count_nonzero(h) > 8 for h in RR._histograms(f))
        assert seen == set(RR.KINDS) or B * T < 4
    assert {RR.kind_of(b, t, 2) for b in range(2) for t in range(2)} == set(RR.KINDS)


def test_no_case_is_a_no_op_on_the_real_frame(g25):
    x, out = frames_at(REAL), outputs(g25, REAL)
    same = [key for key in out if np.array_equal(out[key], x)]
    assert not same, same
    # both filters of every geometric case give different frames (a wrong resample bit cannot pass)
    for name in RR.GEOMETRIC:
        for sign in ("neg", "pos"):
            assert not np.array_equal(out[f"op.{name}.m6.{sign}.bilinear"], out[f"op.{name}.m6.{sign}.bicubic"])


def equalize_last_entry(h):
    """(Equalize's step, the table's entry at the last occupied level BEFORE the cut to 255)"""
    nz = np.nonzero(h)[0]
    step = (int(h.sum()) - int(h[nz[-1]])) // 255
    return step, (step // 2 + int(h[:nz[-1]].sum())) // step if step else None


def test_real_frames_reach_both_ends_of_the_equalize_cut():
    """at 224 x 224 the step is far above 1 (196 where the last level is rare), the start value step / 2 matters, and the entry of the
    last occupied level is 255 or 256 before the cut, by the remainder of the division: both occur among the fixture's channels"""
    B, T, H, W = REAL
    x = frames_at(REAL)
    found = [equalize_last_entry(h) for b in range(B) for t in range(T) for h in RR._histograms(x[b, t])]
    print("equalize (step, entry at the last occupied level) per (frame, channel):", found)
    assert all(step >= 2 for step, _ in found) and {255, 256} <= {last for _, last in found}
    # and the start value is seen in the table: without it at least one entry of every table differs
    for b in range(B):
        for t in range(T):
            for h in RR._histograms(x[b, t]):
                step, _ = equalize_last_entry(h)
                below = np.concatenate([[0], np.cumsum(h)[:-1]])
                assert [min(255, int(n) // step) for n in below] != RR.equalize_lut(h)


# ------------------------------------------------------------------ table words the fixture shape never sets
@pytest.fixture(scope="module")
def lib():
    from simple_tad_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


MASKS = (((31,), 0x80000000, 0), ((32,), 0, 1), ((63,), 0, 0x80000000), ((0, 31, 32, 63), 0x80000001, 0x80000001),
         (tuple(range(64)), 0xFFFFFFFF, 0xFFFFFFFF), ((), 0, 0))


@pytest.mark.parametrize("bicubic,lo,hi", MASKS, ids=[",".join(map(str, m[0])) if len(m[0]) < 9 else "all" for m in MASKS])
def test_resample_mask_of_64_frames_is_split_into_words_4_and_5(lib, bicubic, lo, hi):
    T = 64
    ra = RA.RandAugment([RA.AugmentOp("Rotate", prob=1.0)], num_layers=1)
    resample = tuple(RR.BICUBIC if t in bicubic else RR.BILINEAR for t in range(T))
    tab, stats = ra.table([RA.PlanRow(0, 0, RA.OP_NAMES.index("Rotate"), True, 18.0, resample)], 1, T, 9, 11)
    row = tab.numpy()[0, 0].view(np.uint32)
    assert stats == 0 and row[1] == 11 and (int(row[4]), int(row[5])) == (lo, hi)
    assert [t for t in range(T) if (row[4 + t // 32] >> (t % 32)) & 1] == list(bicubic)
    assert list(tab.numpy()[0, 0, 8:20].view(np.float64)) == RR.rotate_matrix(18.0, 11, 9)


def test_statistics_mask_reaches_layer_31(lib):
    names = ["Equalize"] + ["Invert", "Sharpness", "Rotate"] * 10 + ["ContrastIncreasing"]
    assert len(names) == 32
    ra = RA.RandAugment([RA.AugmentOp(n, prob=1.0) for n in dict.fromkeys(names)], num_layers=32)
    arg = {"Equalize": None, "Invert": None, "Sharpness": 1.72, "Rotate": 18.0, "ContrastIncreasing": 1.54}
    rows = [RA.PlanRow(b, l, RA.OP_NAMES.index(n), True, arg[n], (RR.BICUBIC,) * 2 if n == "Rotate" else None)
            for b in range(2) for l, n in enumerate(names)]
    tab, stats = ra.table(rows, 2, 2, 9, 11)
    assert tuple(tab.shape)[:2] == (32, 2) and stats == 0x80000001
    # a statistics op on one clip of a layer is enough, and a coin that failed needs none
    rows[1] = rows[1]._replace(op=RA.OP_NAMES.index("AutoContrast"), arg=None)
    rows[31] = rows[31]._replace(applied=False, arg=None)
    rows[32 + 31] = rows[32 + 31]._replace(applied=False, arg=None)
    assert ra.table(rows, 2, 2, 9, 11)[1] == 0b11
    with pytest.raises(RA.TadError, match="num_layers"):
        RA.RandAugment([], num_layers=33)
