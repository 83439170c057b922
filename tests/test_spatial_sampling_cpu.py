"""The fine-tune spatial sampling without a GPU: ``SpatialSampling.plan`` against the windows, flips and stream positions the
reference produced (golden G20), the host-side table and ``tad_spatial_sample_plan_check``, and the numpy restatement of the device
arithmetic (tests/spatial_sampling_recipe.py) against the reference's f32 output.

Measured (the reference on CPU torch 2.10, this restatement): the worst max |restatement - reference| / (2 gap + 4 ulp) over the 18
cases is 0.330 (idx0.15x10: 4.77e-7 against a bound of 1.45e-6; s18.37x53, the case with the largest gap, 3.15e-6: 2.38e-6 against
7.25e-6, ratio 0.329); scale1.20x27 differs in 0 bits."""
import ctypes
import random

import numpy as np
import pytest
import torch

import spatial_sampling_recipe as SR
from simple_tad_amd import _lib
from simple_tad_amd._lib import TadError
from simple_tad_amd.spatial_sampling import SpatialSampling, Window

CASE = {c[0]: c for c in SR.CASES}


def golden_plan(g, key):
    return [Window(*[int(v) for v in row]) for row in g[f"{key}.windows"]]


def test_the_goldens_were_made_from_these_inputs(golden):
    assert np.array_equal(golden("g20_spatial_sampling")["input.sha"], SR.inputs_digest())


@pytest.mark.parametrize("case", SR.CASES, ids=SR.CASE_IDS)
def test_plan_reproduces_the_reference_windows_and_both_stream_positions(golden, case):
    g = golden("g20_spatial_sampling")
    key, seed, (H, W), kw = case
    random.seed(seed)
    np.random.seed(seed)
    plan = SpatialSampling(**kw).plan(SR.B, SR.T, H, W)
    nxt = random.random(), np.random.uniform()
    assert np.array_equal(np.array(plan, dtype=np.int64), g[f"{key}.windows"]), key
    assert nxt == (float(g[f"{key}.next_py"]), float(g[f"{key}.next_np"]))


@pytest.mark.parametrize("case", SR.CASES, ids=SR.CASE_IDS)
def test_table_and_plan_check_accept_every_golden_plan(golden, case):
    g = golden("g20_spatial_sampling")
    key, _, (H, W), kw = case
    tab = SpatialSampling(**kw).table(golden_plan(g, key), SR.B, SR.T, H, W)
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (SR.B * SR.T, _lib.SS_ROW_WORDS) == (12, 12)
    t = tab.numpy()
    win = g[f"{key}.windows"]
    assert np.array_equal(t[:, 0], win[:, 0] * SR.T + win[:, 1]) and np.array_equal(t[:, 1:10], win[:, 2:])
    f = np.float32
    assert np.array_equal(t[:, 10].view(f), win[:, 4].astype(f) / win[:, 6].astype(f))
    assert np.array_equal(t[:, 11].view(f), win[:, 5].astype(f) / win[:, 7].astype(f))
    assert _lib.load().tad_spatial_sample_workspace_bytes(SR.B, SR.T) == t.nbytes


def _check(tab, B=SR.B, T=SR.T, H=37, W=53, S=16, n_words=None):
    lib = _lib.load()
    tab = np.ascontiguousarray(tab, dtype=np.int32)
    rc = lib.tad_spatial_sample_plan_check(tab.ctypes.data, tab.size if n_words is None else n_words, B, T, H, W, S)
    return rc, lib.tad_last_error_string().decode()


def test_plan_check_refuses_malformed_tables(golden):
    g = golden("g20_spatial_sampling")
    key = "down.37x53"
    good = SpatialSampling(**CASE[key][3]).table(golden_plan(g, key), SR.B, SR.T, 37, 53).numpy()
    assert _check(good)[0] == 0

    def broken(row, word, value):
        bad = good.copy()
        bad[row, word] = value
        return _check(bad)

    for word, value, what in ((1, 37 - 17, "not inside the 37 x 53 source"), (2, -1, "not inside"), (4, 54, "not inside"), (3, 0, "not inside"),
                              (0, 4, "has two rows"), (0, 12, "outside the B * T"), (0, -1, "outside the B * T"),
                              (7, 1, "not inside the 16 x 16 resized grid"), (8, -1, "resized grid"), (5, 15, "resized grid"),
                              (9, 2, "flip"), (10, 0, "positive and finite"), (11, np.float32(np.inf).view(np.int32), "positive and finite"),
                              (10, np.float32(np.nan).view(np.int32), "positive and finite"), (11, np.float32(-1).view(np.int32), "positive")):
        rc, msg = broken(5, word, value)
        assert rc == -1 and what in msg, (word, value, msg)
    rc, msg = _check(good, n_words=good.size - 1)
    assert rc == -1 and "words, expected" in msg
    rc, msg = _check(good[:-1], n_words=None)
    assert rc == -1 and "words, expected" in msg
    assert _check(good, S=17)[0] == -1 and _check(good, H=30)[0] == -1
    # the wrapper states the same: a window outside the source, a doubled frame, a missing frame
    ss = SpatialSampling(**CASE[key][3])
    plan = golden_plan(g, key)
    with pytest.raises(TadError, match="not inside"):
        ss.table([plan[0]._replace(j=40)] + plan[1:], SR.B, SR.T, 37, 53)
    with pytest.raises(TadError, match="one window per frame"):
        ss.table(plan + [plan[3]], SR.B, SR.T, 37, 53)
    with pytest.raises(TadError, match="one window per frame"):
        ss.table(plan[:-1], SR.B, SR.T, 37, 53)


def test_entry_point_validates_on_the_host():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.tad_spatial_sample(None, 0, None, None, None, None, 0, 1, 1, 8, 8, 4, None) == -1
    assert b"null" in lib.tad_last_error_string()
    assert lib.tad_spatial_sample(p, 0, p, None, None, p, 0, 1, 1, 8, 8, 4, None) == -1 and b"workspace of 0 bytes" in lib.tad_last_error_string()
    assert lib.tad_spatial_sample(p, 1, p, None, None, p, 48, 1, 1, 8, 8, 4, None) == -1 and b"mean and std" in lib.tad_last_error_string()
    assert lib.tad_spatial_sample(p, 0, p, None, None, p, 1 << 30, 4096, 16, 8, 8, 4, None) == -1 and b"B * T" in lib.tad_last_error_string()
    assert lib.tad_spatial_sample(p, 0, p, None, None, p, 48, 1, 1, 8, 8, 0, None) == -1 and b"S=0" in lib.tad_last_error_string()
    assert lib.tad_spatial_sample_workspace_bytes(0, 4) == 0
    with pytest.raises(TadError, match="GPU"):
        SpatialSampling(crop_size=8)(torch.zeros(1, 3, 2, 16, 16))                 # there is no CPU path


def test_what_the_reference_refuses_is_refused():
    with pytest.raises(TadError, match="spatial_idx"):
        SpatialSampling(spatial_idx=3)
    with pytest.raises(TadError, match="must be the same"):
        SpatialSampling(spatial_idx=1, min_scale=256, max_scale=320, crop_size=224)
    with pytest.raises(TadError, match="come together"):
        SpatialSampling(scale=(0.08, 1.0))
    # a jittered clip of exactly crop_size x crop_size: the reference's random_crop returns a bare tensor and its caller raises
    with pytest.raises(TadError, match="exactly 16 x 16"):
        SpatialSampling(min_scale=16, max_scale=16, crop_size=16).plan(1, 2, 20, 20)
    with pytest.raises(TadError, match="smaller than crop_size"):
        SpatialSampling(min_scale=8, max_scale=8, crop_size=16).plan(1, 2, 20, 20)


@pytest.mark.parametrize("case", SR.CASES, ids=SR.CASE_IDS)
def test_restatement_is_within_the_reference_s_own_error(golden, case):
    g = golden("g20_spatial_sampling")
    key, _, (H, W), kw = case
    want = g[f"{key}.out"]
    got = SR.sample(SR.clips(H, W), g[f"{key}.windows"], kw["crop_size"])
    err, bound = float(np.abs(got.astype(np.float64) - want).max()), SR.bound(g, key)
    differing = int((got.view(np.int32) != want.view(np.int32)).sum())
    print(f"spatial sampling {key}: max |restatement - reference| {err:.3g}, gap {float(g[f'{key}.gap']):.3g}, bound {bound:.3g}, "
          f"ratio {err / bound:.3f}, {differing} of {want.size} values differ in a bit")
    assert err <= bound
    if key in SR.EXACT_CASES:
        assert differing == 0


def test_a_flip_is_the_mirrored_result_bit_for_bit(golden):
    g = golden("g20_spatial_sampling")
    for key in ("down.37x53", "s18.37x53", "jitter.20x27"):
        _, _, (H, W), kw = CASE[key]
        win = g[f"{key}.windows"].copy()
        assert win[:, 10].any()
        got = SR.sample(SR.clips(H, W), win, kw["crop_size"])
        flipped = win[:, 10] == 1
        win[:, 10] = 0
        plain = SR.sample(SR.clips(H, W), win, kw["crop_size"])
        for row, f in zip(win, flipped):
            b, t = row[0], row[1]
            want = plain[b, :, t, :, ::-1] if f else plain[b, :, t]
            assert np.array_equal(got[b, :, t].view(np.int32), want.view(np.int32))


def test_the_uint8_twins_give_the_clips():
    """frames_to_clip's expression in numpy f32 (what the fused route applies to every tap)"""
    u8 = SR.frames(17, 19)
    x = SR.clips(17, 19)
    t = torch.from_numpy(u8).float().div(255.0).permute(0, 4, 1, 2, 3)
    want = (t - torch.tensor(SR.MEAN).view(1, 3, 1, 1, 1)) / torch.tensor(SR.STD).view(1, 3, 1, 1, 1)
    assert np.array_equal(x.view(np.int32), want.contiguous().numpy().view(np.int32))
