"""The MAE pre-training crop without a GPU: the numpy restatement (tests/multiscale_crop_recipe.py) against the reference's frames
(golden G18) and against PIL directly; ``GroupMultiScaleCrop.plan`` against the reference's crops and stream position; the host's
tables through ``tad_multiscale_crop_plan_check`` and every malformation it refuses; the filter-scale limit; the engine's signature."""
import inspect
import random

import numpy as np
import pytest
import torch

import multiscale_crop_recipe as MR
from simple_tad_amd import _lib
from simple_tad_amd import transforms as TF
from simple_tad_amd._lib import TadError

CASES = MR.CASES


def transform_of(case):
    return TF.GroupMultiScaleCrop(case[3], **{k: list(v) if k == "scales" else v for k, v in case[4].items()})


def test_the_golden_was_made_from_these_inputs(golden):
    assert np.array_equal(golden("g18_multiscale_crop")["input.sha"], MR.inputs_digest())


@pytest.mark.parametrize("case", CASES, ids=MR.CASE_IDS)
def test_recipe_equals_the_reference_byte_for_byte(golden, case):
    g = golden("g18_multiscale_crop")
    crops, nxt, out = MR.run_case(case)
    assert np.array_equal(crops, g[f"{case[0]}.crops"]) and nxt == float(g[f"{case[0]}.next_py"])
    diff = int((out != g[f"{case[0]}.out"]).sum())
    print(f"multiscale crop recipe {case[0]}: {diff} of {out.size} bytes differ from the reference")
    assert diff == 0


@pytest.mark.parametrize("size,S", [((45, 80), (32, 32)), ((20, 23), (32, 32)), ((100, 37), (48, 40)), ((120, 200), (25, 16))])
def test_recipe_equals_pil_directly(size, S):
    Image = pytest.importorskip("PIL.Image")
    x = MR.frames(*size)[0, 0]
    want = np.asarray(Image.fromarray(x).resize(S, Image.BILINEAR))
    assert np.array_equal(MR.resize(x, *S), want)


@pytest.mark.parametrize("case", CASES, ids=MR.CASE_IDS)
def test_plan_reproduces_the_reference_crops_and_stream_position(golden, case):
    g = golden("g18_multiscale_crop")
    _, seed, (Hs, Ws), S, _, _ = case
    random.seed(seed)
    plan = transform_of(case).plan(MR.B, (Ws, Hs))
    assert [p.clip for p in plan] == list(range(MR.B))
    assert [[p.w, p.h, p.x0, p.y0] for p in plan] == g[f"{case[0]}.crops"].tolist()
    assert random.random() == float(g[f"{case[0]}.next_py"])


def test_fix_crop_offers_5_or_13_offsets_and_the_crop_sizes_snap():
    assert len(TF.GroupMultiScaleCrop(32, more_fix_crop=False).fixed_offsets(80, 45, 39, 29)) == 5
    assert len(TF.GroupMultiScaleCrop(32).fixed_offsets(80, 45, 39, 29)) == 13
    pairs = TF.GroupMultiScaleCrop(32).crop_pairs((60, 34))          # int(34 * 1) = 34 is within 3 of 32
    assert pairs[0] == (32, 32) and {w for w, _ in pairs} == {32, 29, 25, 22} and len(pairs) == 10
    assert len(TF.GroupMultiScaleCrop(32, max_distort=0).crop_pairs((60, 34))) == 4


@pytest.mark.parametrize("in_size,out_size", [(39, 32), (17, 32), (32, 32), (120, 16), (100, 48)])
def test_host_coefficients_equal_the_recipe(in_size, out_size):
    ksize, bounds, kk = MR.coefficients(in_size, out_size)
    n_in, k2, b2, kk2 = TF.resample_coefficients(in_size, out_size)
    assert (n_in, k2) == (in_size, ksize) and np.array_equal(b2, bounds) and np.array_equal(kk2, kk)
    if in_size == out_size:                                           # the identity: one tap of weight 1
        assert (kk[:, 0] == 1 << 22).all() and (kk[:, 1:] == 0).all() and (bounds[:, 0] == np.arange(out_size)).all()


# ---------------------------------------------------------------------------------------------------- the plan check
@pytest.mark.parametrize("case", CASES, ids=MR.CASE_IDS)
def test_plan_check_accepts_the_host_tables(case):
    _, seed, (Hs, Ws), S, _, _ = case
    random.seed(seed)
    tf = transform_of(case)
    table, nh, nv = tf.table(tf.plan(MR.B, (Ws, Hs)), MR.B, Hs, Ws)
    lib = _lib.load()
    assert table.dtype == torch.int32 and table.numel() * 4 == lib.tad_multiscale_crop_workspace_bytes(MR.B, nh, nv, S, S)
    assert table.numel() == MR.B * 8 + (nh + nv) * (4 + S * 19)


HS, WS, S = 45, 80, 32
PLAN = [TF.Crop(0, 39, 33, 8, 1), TF.Crop(1, 45, 39, 20, 0), TF.Crop(2, 39, 45, 41, 0)]


def good_table():
    table, nh, nv = TF.GroupMultiScaleCrop(S).table(PLAN, 3, HS, WS)
    assert (nh, nv) == (2, 3)
    return table.numpy().copy()


def plan_check(tab, n_words=None, B=3, nh=2, nv=3):
    tab = np.ascontiguousarray(tab, dtype=np.int32)
    return _lib.load().tad_multiscale_crop_plan_check(tab.ctypes.data, tab.size if n_words is None else n_words, B, nh, nv, HS, WS, S, S)


SLOT = 4 + S * 19
HSET0, VSET0 = 3 * 8, 3 * 8 + 2 * SLOT


def test_plan_check_accepts_the_hand_stated_plan():
    assert plan_check(good_table()) == 0


MALFORMED = {
    "a word short": lambda t: t[:-1],
    "a word long": lambda t: np.concatenate([t, [0]]),
    "a sample twice": lambda t: _set(t, 8 * 2 + 0, 1),
    "a sample outside the batch": lambda t: _set(t, 8 * 1 + 0, 3),
    "a negative sample": lambda t: _set(t, 0, -1),
    "a crop past the right edge": lambda t: _set(t, 8 * 2 + 1, 42),
    "a crop past the bottom": lambda t: _set(t, 8 * 0 + 2, 13),
    "a negative offset": lambda t: _set(t, 8 * 0 + 1, -1),
    "an empty crop": lambda t: _set(t, 8 * 0 + 3, 0),
    "a horizontal set index out of range": lambda t: _set(t, 8 * 0 + 5, 2),
    "a vertical set index out of range": lambda t: _set(t, 8 * 1 + 6, -1),
    "a set stated for another crop width": lambda t: _set(t, 8 * 0 + 5, 1),
    "a count above ksize": lambda t: _set(t, HSET0 + 4 + 2 * 5 + 1, 6),            # (39 -> 32 samples: ksize 5)
    "a negative count": lambda t: _set(t, VSET0 + 4 + 2 * 7 + 1, -1),
    "bounds past the crop": lambda t: _set(t, HSET0 + 4 + 2 * 31, 38),
    "a negative xmin": lambda t: _set(t, HSET0 + 4 + 2 * 0, -1),
    "ksize above the limit": lambda t: _set(t, HSET0 + 2, 18),
    "ksize zero": lambda t: _set(t, VSET0 + 2, 0),
    "a set's output extent": lambda t: _set(t, VSET0 + 1, 31),
}


def _set(t, i, v):
    t = t.copy()
    t[i] = v
    return t


@pytest.mark.parametrize("name", list(MALFORMED))
def test_plan_check_refuses(name):
    lib = _lib.load()
    assert plan_check(MALFORMED[name](good_table())) != 0
    assert b"multiscale_crop_plan_check" in lib.tad_last_error_string()


def test_plan_check_refuses_wrong_counts_of_sets_and_clips():
    t = good_table()
    assert plan_check(t, nh=3, nv=2) != 0                  # the same word count split otherwise: a vertical index is out of range
    assert plan_check(t, B=2) != 0 and plan_check(t, nh=0) != 0 and plan_check(t, n_words=t.size - SLOT, nv=2) != 0
    assert _lib.load().tad_multiscale_crop_plan_check(None, 0, 3, 2, 3, HS, WS, S, S) != 0


def test_plan_check_refuses_a_filter_scale_above_8():
    """S = 4: a hand-stated table whose horizontal set shrinks 33 samples to 4 (32 -> 4, scale 8, passes)"""
    slot = 4 + 4 * 19
    for n_in, ok in ((32, True), (33, False)):
        t = np.zeros(8 + 2 * slot, dtype=np.int32)
        t[:8] = 0, 0, 0, n_in, 4, 0, 0, 0
        t[8:11] = n_in, 4, 17
        t[8 + slot:8 + slot + 3] = 4, 4, 3
        rc = _lib.load().tad_multiscale_crop_plan_check(t.ctypes.data, t.size, 1, 1, 1, HS, WS, 4, 4)
        assert (rc == 0) == ok
        if not ok:
            assert b"filter scale above 8" in _lib.load().tad_last_error_string()


def test_table_refuses_plans_that_are_not_one_crop_per_clip():
    tf = TF.GroupMultiScaleCrop(S)
    for plan in (PLAN[:2], PLAN + [TF.Crop(1, 39, 39, 0, 0)], [PLAN[0], PLAN[1], TF.Crop(3, 39, 39, 0, 0)],
                 [PLAN[0], PLAN[1], TF.Crop(2, 39, 39, 42, 0)]):
        with pytest.raises(TadError):
            tf.table(plan, 3, HS, WS)


def test_filter_scale_above_8_is_refused_before_any_launch():
    TF.resample_coefficients(128, 16)                                  # scale 8: ksize 17, the limit
    with pytest.raises(TadError, match="filter scale"):
        TF.resample_coefficients(129, 16)
    tf = TF.GroupMultiScaleCrop(16)
    with pytest.raises(TadError, match="filter scale"):
        tf.table([TF.Crop(0, 129, 129, 0, 0)], 1, 140, 200)
    random.seed(0)
    with pytest.raises(TadError, match="filter scale"):               # int(140 * 1) = 140 -> 16 is in every draw's reach
        for _ in range(40):
            tf.table(tf.plan(1, (200, 140)), 1, 140, 200)


def test_a_cpu_tensor_is_refused():
    tf = TF.GroupMultiScaleCrop(S)
    x = torch.zeros(3, 2, HS, WS, 3, dtype=torch.uint8)
    with pytest.raises(TadError):
        tf.apply(x, PLAN)
    with pytest.raises(TadError):
        tf(x)


def test_data_augmentation_surface():
    from types import SimpleNamespace
    args = SimpleNamespace(input_size=32, mask_type="tube", window_size=(8, 2, 2), mask_ratio=0.75)
    a, b = TF.DataAugmentationForVideoMAE(args), TF.DataAugmentationForVideoMAE_LightCrop(args)
    assert a.train_augmentation.scales == [1, .875, .75, .66] and b.train_augmentation.scales == [1, 1, .975, .95, .9, .875, .85]
    assert a.input_mean == [0.485, 0.456, 0.406] and a.input_std == [0.229, 0.224, 0.225]
    assert a.masked_position_generator.total_masks == 8 * 3 and "TubeMaskingGenerator" in repr(a)
    with pytest.raises(TadError):
        TF.DataAugmentationForVideoMAE(SimpleNamespace(input_size=32, mask_type="random", window_size=(8, 2, 2), mask_ratio=0.75))


def test_the_pretrain_engine_keeps_its_parameters_and_takes_augment_fn_last():
    from simple_tad_amd import engine_pretrain as EP
    params = list(inspect.signature(EP.train_one_epoch).parameters.values())
    assert [p.name for p in params] == ["model", "data_loader", "optimizer", "device", "epoch", "loss_scaler", "max_norm", "patch_size",
                                        "normlize_target", "start_steps", "lr_schedule_values", "wd_schedule_values", "tubelet_size",
                                        "log", "augment_fn"]
    assert params[-1].default is None and params[-2].default is None and params[6].default == 0


def test_the_kernel_text_on_the_host_under_sanitizers(tmp_path):
    """tools/multiscale_crop_host_check.py: the kernel's own text in a stand-alone CPU program built with the address and
    undefined-behaviour sanitizers equals every golden, and a malformed table is never an address"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import multiscale_crop_host_check as HC
    if HC.compiler() is None:
        pytest.skip("no C++ compiler")
    assert HC.check(HC.build(str(tmp_path)), str(tmp_path), verbose=False)


def test_the_pretrain_engine_says_when_a_step_has_no_masks():
    from simple_tad_amd import engine_pretrain as EP
    model = torch.nn.Linear(1, 1)
    clips = torch.zeros(1, 3, 2, 4, 4)
    for augment_fn, what in ((None, "is None"), (lambda v: v, "returned the clips alone")):
        with pytest.raises(ValueError, match=what):
            EP.train_one_epoch(model, [(clips,)], None, torch.device("cpu"), 0, None, augment_fn=augment_fn)
