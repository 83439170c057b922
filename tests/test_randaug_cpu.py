"""RandAugment without a GPU: ``RandAugment.plan`` and the config parser against what the reference's own transform chose (golden G16,
tools/make_goldens_randaug.py), the numpy restatement of every operator (tests/randaug_recipe.py) against PIL's output frames bit for
bit, the host-side validation of the new C entry points, and the place of ``augment_fn`` in the fine-tune loop."""
import ctypes
import inspect
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_recipe as R
import randaug_recipe as RR
import simple_tad_amd.rand_augment as RA
from oracle import vit_oracle as O
from simple_tad_amd import engine as E
from simple_tad_amd._lib import RANDAUG_ROW_WORDS, TadError
from test_mixup_cpu import _build_tiny

OP_CASES = RR.op_cases()


@pytest.fixture(scope="module")
def g16(golden):
    return golden("g16_rand_augment")


@pytest.fixture(scope="module")
def frames(g16):
    x = RR.frames()
    assert np.array_equal(RR.digest(x), g16["input.sha"])
    return x


def policy_transform(oplist, interp):
    hp = {"translate_const": int(RR.H * 0.45)}
    if interp is not None:
        hp["interpolation"] = interp
    return RA.rand_augment_transform(RR.POLICY, hp, RA.DRIVE_TRANSFORMS if oplist == "drive" else None)


def seeded_plan(seed, oplist, interp):
    ra = policy_transform(oplist, interp)
    random.seed(seed)
    np.random.seed(seed)
    return ra, ra.plan(RR.B, RR.T)


# ------------------------------------------------------------------ the draws
@pytest.mark.parametrize("key,seed,oplist,interp", RR.POLICIES, ids=[p[0] for p in RR.POLICIES])
def test_plan_reproduces_the_choices_of_the_reference_and_both_stream_positions(g16, key, seed, oplist, interp):
    ra, rows = seeded_plan(seed, oplist, interp)
    assert random.random() == float(g16[f"{key}.next_py"]) and np.random.random() == float(g16[f"{key}.next_np"])
    assert [(r.clip, r.layer) for r in rows] == [(b, l) for b in range(RR.B) for l in range(3)]
    assert [RA.OP_NAMES[r.op] for r in rows] == list(g16[f"{key}.ops"])
    assert [r.applied for r in rows] == list(g16[f"{key}.applied"])
    for r, arg, rs in zip(rows, g16[f"{key}.args"], g16[f"{key}.resample"]):
        if r.arg is None:
            assert np.isnan(arg)
        else:
            assert float(r.arg) == float(arg)                         # the very double the reference handed to PIL
        assert (list(r.resample) if r.resample else [0] * RR.T) == list(rs)
    if interp is None:
        assert any(r.resample and len(set(r.resample)) > 1 for r in rows)   # the per-frame draw is exercised


def test_config_strings_and_the_surface():
    assert RA.parse_config("rand-m6-n3-mstd0.5-inc1") == dict(magnitude=6, num_layers=3, magnitude_std=0.5, increasing=True)
    assert RA.parse_config("rand-m9-n3-mstd0.5") == dict(magnitude=9, num_layers=3, magnitude_std=0.5, increasing=False)
    assert RA.parse_config("rand-mstd1") == dict(magnitude=10.0, num_layers=2, magnitude_std=1.0, increasing=False)
    assert RA.parse_config("rand-inc0")["increasing"] is True             # the reference's bool("0")
    for bad in ("rand-mstd1-w0", "rand-m6-w0"):
        with pytest.raises(TadError, match="weighted"):
            RA.rand_augment_transform(bad, {})
    hp = {"translate_const": 9}
    ra = RA.rand_augment_transform("rand-m6-n3-mstd0.5-inc1", hp)
    assert hp["magnitude_std"] == 0.5 and ra.num_layers == 3 and [o.name for o in ra.ops] == RA._RAND_INCREASING_TRANSFORMS
    assert all(o.prob == 0.5 and o.magnitude == 6 and o.magnitude_std == 0.5 and o.fill == (128, 128, 128) for o in ra.ops)
    assert [o.name for o in RA.rand_augment_transform("rand-m6", {}).ops] == RA._RAND_TRANSFORMS
    ra = RA.create_random_augment((224, 224), "rand-m6-n3-mstd0.5-inc1", "bicubic", RA.DRIVE_TRANSFORMS)
    assert isinstance(ra, RA.RandAugment) and [o.name for o in ra.ops] == RA.DRIVE_TRANSFORMS
    assert all(o.resample == RA.BICUBIC and o.hparams["translate_const"] == 100 for o in ra.ops)
    assert RA.create_random_augment(224, "rand-m6", "random").ops[0].resample == (RA.BILINEAR, RA.BICUBIC)
    with pytest.raises(NotImplementedError):
        RA.create_random_augment(224, None)
    with pytest.raises(TadError, match="not built"):
        RA.AugmentOp("TranslateX")
    for angle in (90.0, 180.0, -90.0):
        with pytest.raises(TadError, match="transposes"):
            RA._affine_coefficients("Rotate", angle, 23, 20)
    assert list(inspect.signature(RA.rand_augment_transform).parameters) == ["config_str", "hparams", "do_transforms"]
    assert list(inspect.signature(RA.create_random_augment).parameters) == ["input_size", "auto_augment", "interpolation", "do_transforms"]
    assert list(inspect.signature(RA.RandAugment.__init__).parameters)[1:] == ["ops", "num_layers", "choice_weights"]
    import simple_tad_amd as T
    assert T.RandAugment is RA.RandAugment and T.rand_augment is RA and T.frames_to_clip is RA.frames_to_clip


def test_cpu_tensors_and_other_layouts_are_refused():
    ra = policy_transform("drive", RR.BICUBIC)
    for x in (torch.zeros(2, 2, 8, 8, 3, dtype=torch.uint8), torch.zeros(2, 8, 8, 3, dtype=torch.uint8)):
        with pytest.raises(TadError, match="no CPU path"):
            ra(x)
    with pytest.raises(TadError):
        ra(torch.zeros(8, 8, 3, dtype=torch.uint8))
    with pytest.raises(TadError, match="no CPU path"):
        RA.frames_to_clip(torch.zeros(2, 2, 8, 8, 3, dtype=torch.uint8), (0.5,) * 3, (0.2,) * 3)


# ------------------------------------------------------------------ the restatement against PIL
@pytest.mark.parametrize("key,name,m,seed,rs", OP_CASES, ids=[c[0] for c in OP_CASES])
def test_numpy_restatement_equals_pil_bit_for_bit_per_op(g16, frames, key, name, m, seed, rs):
    arg = float(g16[f"{key}.arg"])
    arg = None if np.isnan(arg) else (int(arg) if name.startswith(("Posterize", "Solarize")) else arg)
    want = g16[f"{key}.out"]
    for b in range(RR.B):
        for t in range(RR.T):
            assert np.array_equal(RR.apply(frames[b, t], name, arg, rs), want[b, t]), (b, t)


@pytest.mark.parametrize("key,seed,oplist,interp", RR.POLICIES, ids=[p[0] for p in RR.POLICIES])
def test_numpy_restatement_equals_pil_bit_for_bit_per_policy(g16, frames, key, seed, oplist, interp):
    _, rows = seeded_plan(seed, oplist, interp)
    got = RR.apply_rows(frames, [(r.clip, r.op, r.applied, r.arg, r.resample) for r in rows], RA.OP_NAMES)
    assert np.array_equal(got, g16[f"{key}.out"])


def test_golden_cases_cover_every_name_sign_filter_and_factor_range(g16, frames):
    names = {c[1] for c in OP_CASES}
    assert names == set(RA.OP_NAMES) == set(RR.ALL_NAMES) and set(RA._RAND_TRANSFORMS + RA._RAND_INCREASING_TRANSFORMS + RA.DRIVE_TRANSFORMS) == names
    for name in RR.NEGATING:
        args = [float(g16[f"{c[0]}.arg"]) for c in OP_CASES if c[1] == name]
        pivot = 1.0 if name.endswith("Increasing") else 0.0
        assert min(args) < pivot < max(args)
    for name in RR.GEOMETRIC:
        assert {c[4] for c in OP_CASES if c[1] == name} == {RR.BILINEAR, RR.BICUBIC}
    for name in ("Color", "Contrast", "Brightness", "Sharpness"):
        args = [float(g16[f"{c[0]}.arg"]) for c in OP_CASES if c[1] == name]
        assert min(args) < 1.0 < max(args)
    # the frames: a constant channel, channels on sub-ranges, a full-range frame; statistics differ between the frames of a clip
    assert frames[1, 0, :, :, 1].min() == frames[1, 0, :, :, 1].max() and (frames[0, 1].min(), frames[0, 1].max()) == (0, 255)
    assert (frames[0, 0, :, :, 0].min(), frames[0, 0, :, :, 0].max()) == (37, 201)
    assert RR.autocontrast_lut(RR._histograms(frames[0, 0])[0]) != RR.autocontrast_lut(RR._histograms(frames[0, 1])[0])
    assert any(RR.equalize_lut(h) != list(range(256)) for b in range(RR.B) for t in range(RR.T) for h in RR._histograms(frames[b, t]))


# ------------------------------------------------------------------ host validation of the C entry points
@pytest.fixture(scope="module")
def lib():
    from simple_tad_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_table_check_rejects_malformed_tables(lib):
    from simple_tad_amd import kernels as K
    ra, rows = seeded_plan(1, "drive", RR.BICUBIC)
    tab, stats = ra.table(rows, RR.B, RR.T, RR.H, RR.W)
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (3, RR.B, RANDAUG_ROW_WORDS) and stats == 0b101   # (layer 1: a shear and two failed coins)
    t = tab.numpy()
    err = lib.tad_last_error_string
    check = lambda a, words=None, L=3, B=RR.B, Tn=RR.T: lib.tad_randaug_plan_check(a.ctypes.data, a.size if words is None else words, L, B, Tn)
    assert check(t) == 0
    assert check(t, words=t.size - 1) == -1 and b"words" in err()
    assert check(t, L=2) == -1 and b"words" in err()
    bad = t.copy(); bad[1, 2, 0] = RR.B
    assert check(bad) == -1 and b"sample=3" in err() and b"layer 1 row 2" in err()
    bad = t.copy(); bad[0, 1, 0] = -1
    assert check(bad) == -1 and b"sample=-1" in err()
    bad = t.copy(); bad[2, 1, 0] = 0
    assert check(bad) == -1 and b"two rows" in err()
    bad = t.copy(); bad[0, 0, 1] = 12
    assert check(bad) == -1 and b"unknown op=12" in err()
    bad = t.copy(); bad[0, 0, 1] = -1
    assert check(bad) == -1 and b"unknown op=-1" in err()
    bad = t.copy(); bad[0, 0, 1] = 7; bad.view(np.float32)[0, 0, 6] = np.nan
    assert check(bad) == -1 and b"not finite" in err()
    bad = t.copy(); bad[0, 0, 1] = 11; bad[0, 0, 8:20] = np.array([1, 0, np.inf, 0, 1, 0], dtype=np.float64).view(np.int32)
    assert check(bad) == -1 and b"coefficient 2" in err()
    bad = t.copy(); bad[0, 0, 1] = 2; bad[0, 0, 2] = 9
    assert check(bad) == -1 and b"bits=9" in err()
    assert lib.tad_randaug_plan_check(None, 0, 0, 1, 1) == -1 and b"null" in err()
    assert check(t, Tn=65) == -1 and b"T=65" in err()
    assert check(t[:0], L=0) == 0                                          # no layer: a valid (copying) plan
    p = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(256)))
    assert lib.tad_randaug_apply(None, p, p, 1, 0, p, 1 << 20, 1, 1, 8, 8, None) == -1 and b"two buffers" in err()
    assert lib.tad_randaug_apply(p, p, p, 1, 0, p, 1 << 20, 1, 1, 8, 8, None) == -1 and b"two buffers" in err()
    assert lib.tad_randaug_workspace_bytes(1, 3, 2, 20, 23) == 3 * 2 * 1024
    assert lib.tad_randaug_workspace_bytes(3, 3, 2, 20, 23) == 3 * 2 * 1024 + (3 * 2 * 20 * 23 * 3 + 255) // 256 * 256
    assert lib.tad_frames_to_clip(None, p, None, None, 1, 1, 8, 8, None) == -1 and b"null" in err()
    # the wrapper and RandAugment.table go through the same check
    with pytest.raises(TadError, match="unknown op"):
        K.randaug_table([[(0, 99, 0, 0.0, None, (0, 0, 0), 0)]], 1, 1)
    with pytest.raises(TadError, match="one row per"):
        ra.table(rows[:-1], RR.B, RR.T, RR.H, RR.W)
    with pytest.raises(TadError, match="one row per"):
        ra.table(rows + rows[:1], RR.B, RR.T, RR.H, RR.W)


def test_table_states_the_plan(lib):
    ra, rows = seeded_plan(3, "drive", None)
    tab, stats = ra.table(rows, RR.B, RR.T, RR.H, RR.W)
    t = tab.numpy()
    for r in rows:
        row = t[r.layer, r.clip]
        name = RA.OP_NAMES[r.op]
        assert row[0] == r.clip
        if not r.applied:
            assert row[1] == 0
        elif name in RA.GEOMETRIC:
            assert row[1] == 11 and row.view(np.uint32)[3] == 128 | 128 << 8 | 128 << 16
            assert list(row[8:20].view(np.float64)) == [float(v) for v in RR.matrix_of(name, r.arg, RR.W, RR.H)]
            assert [RR.BICUBIC if row[4] >> f & 1 else RR.BILINEAR for f in range(RR.T)] == list(r.resample)
        elif name in ("Color", "Contrast", "Brightness", "Sharpness"):
            assert row.view(np.float32)[6] == np.float32(r.arg)
    assert stats == sum(1 << l for l in range(3) if np.isin(t[l, :, 1], (5, 6, 9)).any())


# ------------------------------------------------------------------ the fine-tune loop with augment_fn
def _stub_epoch(batches, **fns):
    c, tiny = R.G12, R.TINY
    m = _build_tiny("cpu", torch.float64)
    kw = dict(depth=tiny["depth"], num_heads=tiny["num_heads"], tubelet=tiny["tubelet_size"], patch=tiny["patch_size"])

    def oracle_forward(x):           # (the package's modules run HIP kernels only: the fp64 oracle stands in, as in test_mixup_cpu.py)
        P = dict(m.named_parameters())
        return F.linear(O.forward_features(x, P, **kw), P["head.weight"], P["head.bias"])

    m.forward = oracle_forward
    opt = E.create_optimizer(m, lr=c["base_lr"], weight_decay=c["weight_decay"], layer_decay=c["layer_decay"], fused_kernel=False)
    return E.train_one_epoch(m, torch.nn.CrossEntropyLoss(), batches, opt, torch.device("cpu"), 0, E.NativeScalerWithGradNormCount(m),
                             update_freq=2, **fns)


def test_train_one_epoch_calls_augment_fn_once_per_micro_step_before_erase_fn():
    batches = R.g12_batches(torch.float64)[:4]
    calls = []

    def augment(samples):
        calls.append(("augment", samples.data_ptr()))
        return samples

    def erase(samples):
        calls.append(("erase", samples.data_ptr()))
        return samples

    with_fn = _stub_epoch(batches, augment_fn=augment, erase_fn=erase)
    assert [k for k, _ in calls] == ["augment", "erase"] * 4
    assert all(calls[2 * i][1] == calls[2 * i + 1][1] for i in range(4))          # the eraser gets what the augmenter returned
    plain = _stub_epoch(batches)
    assert plain["loss"] == with_fn["loss"] and _stub_epoch(batches, augment_fn=None)["loss"] == plain["loss"]
    p = inspect.signature(E.train_one_epoch).parameters
    assert p["augment_fn"].default is None and list(p)[-3:] == ["augment_fn", "erase_fn", "mixup_fn"]
    # an augmenter that changes the batch changes the run (the hook is live)
    assert _stub_epoch(batches, augment_fn=lambda s: s * 0.5)["loss"] != plain["loss"]
