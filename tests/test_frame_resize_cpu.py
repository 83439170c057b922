"""The frame ingest without a GPU: the host coefficients against the numpy restatement of the contract (tests/frame_resize_recipe.py),
the restatement against an independent float64 bicubic, ``PadWideClips.plan`` against the reference's draws and generator state (golden
G23), the host's tables through ``tad_frame_resize_plan_check`` and every malformation it refuses, and the refusals that come before any
launch."""
import numpy as np
import pytest
import torch

import frame_resize_recipe as R
from simple_tad_amd import _lib
from simple_tad_amd import frame_resize as FR
from simple_tad_amd import kernels as K
from simple_tad_amd._lib import TadError

ALL_SHAPES = R.SHAPES + R.EXTRA_SHAPES
EXTENTS = sorted({(n, m) for (H, W), (Sh, Sw) in ALL_SHAPES for n, m in ((H, Sh), (W, Sw))} | {(1280, 224), (720, 224), (1, 1), (224, 720)})
G_MODES = {0: None, 1: "black", 2: "color", 3: "reflect", 4: "replicate"}


# ---------------------------------------------------------------------------------------------------- the coefficients
@pytest.mark.parametrize("n_src,n_dst", EXTENTS)
def test_cubic_coeffs_equal_the_recipe(n_src, n_dst):
    first, k = FR.cubic_coeffs(n_src, n_dst)
    taps, kk = R.axis(n_src, n_dst)
    assert first.dtype == np.int32 and k.dtype == np.int32 and first.shape == (n_dst,) and k.shape == (n_dst, 4)
    assert np.array_equal(k, kk)
    assert np.array_equal(np.clip(first[:, None] + np.arange(4), 0, n_src - 1), taps)
    assert set(k.sum(axis=1).tolist()) <= {2047, 2048, 2049}          # not renormalised
    assert np.abs(k).sum(axis=1).max() <= 2818 == _lib.FR_MAX_ABS_SUM
    assert first.min() >= -2 and first.max() <= n_src - 2             # s = first + 1 in [-1, n_src - 1]
    assert taps.min() >= 0 and taps.max() <= n_src - 1 and (np.diff(taps, axis=1) >= 0).all()   # clamped at both ends
    if n_dst >= n_src:                                                # (a strong shrink keeps its taps off the borders)
        assert first[0] < 0 and first[-1] + 3 > n_src - 1 and taps.min() == 0 and taps.max() == n_src - 1
    if n_src == n_dst:                                                # the identity: the tap at the output's own index, weight 1
        assert (k == (0, 2048, 0, 0)).all() and np.array_equal(first + 1, np.arange(n_dst))


def test_upscale_clamps_taps_at_both_borders():
    first, _ = FR.cubic_coeffs(9, 32)
    assert first[0] == -2 and first[-1] == 7                          # taps -2 .. 1 and 7 .. 10 of a source 0 .. 8
    taps, _ = R.axis(9, 32)
    assert taps[0].tolist() == [0, 0, 0, 1] and taps[-1].tolist() == [7, 8, 8, 8]
    assert (R.axis(1, 4)[0] == 0).all()                               # one source sample: every tap clamps to it


# ---------------------------------------------------------------------------------------------------- the recipe against float64 bicubic
@pytest.mark.parametrize("src,dst", R.SHAPES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in R.SHAPES])
def test_recipe_lies_within_one_grey_level_of_float64_bicubic(src, dst):
    """0.5 for the final rounding plus at most 4 * 255 * (0.5 / 2048) ~ 0.25 per pass from 11-bit coefficients: off by two is a bug.
    Measured over these inputs: at most 0.723, at most 6.2 % of the bytes off the rounded reference (70x90 -> 33x35)."""
    im = R.images(*src)
    got = R.resize(im, *dst)
    ref = R.float64_bicubic(im, *dst)
    err = float(np.abs(got.astype(np.float64) - np.clip(ref, 0, 255)).max())
    share = float((got != np.clip(np.rint(ref), 0, 255).astype(np.uint8)).mean())
    print(f"frame resize recipe {src} -> {dst}: max |byte - float64 bicubic| = {err:.3f}, {100 * share:.2f} % of bytes off the rounded reference")
    assert err <= 1.0
    assert share <= 0.10
    if src == dst:
        assert np.array_equal(got, im)


def test_the_step_image_leaves_the_byte_range_on_both_sides():
    un = R.resize_unclipped(R.images(45, 80)[2:], 28, 28)
    assert un.min() < 0 and un.max() > 255


def test_recipe_pad_modes():
    x = R.images(5, 9)[:1]
    assert R.pad_frames(x, None, 3, 3) is x
    for mode in R.MODES:
        assert np.array_equal(R.pad_frames(x, mode, 0, 0, 0.5, (1, 2, 3)), x)
        p = R.pad_frames(x, mode, 2, 3, 0.5, (1, 2, 3))
        assert p.shape == (1, 10, 9, 3) and np.array_equal(p[:, 2:7], x)                   # inside the frame: the byte itself
    assert (R.pad_frames(x, "color", 2, 3, 0.5, (1, 2, 3))[:, [0, 1, 7, 8, 9]] == (1, 2, 3)).all()
    assert not R.pad_frames(x, "black", 2, 3, 0.5, (1, 2, 3))[:, [0, 1, 7, 8, 9]].any()
    rep = R.pad_frames(x, "replicate", 2, 3)
    assert np.array_equal(rep[0, 0], x[0, 0]) and np.array_equal(rep[0, 1], x[0, 0]) and np.array_equal(rep[0, 9], x[0, 4])
    ref = R.pad_frames(x, "reflect", 2, 3, 1.0)                                            # alpha 1: the mirror image itself, edge row doubled
    assert np.array_equal(ref[0, [1, 0]], x[0, [0, 1]]) and np.array_equal(ref[0, [7, 8, 9]], x[0, [4, 3, 2]])
    half = R.pad_frames(np.full((1, 1, 1, 3), 5, np.uint8), "reflect", 1, 1, 0.5)          # 2.5 -> 2: ties to even
    assert half[0, :, 0, 0].tolist() == [2, 5, 2]


# ---------------------------------------------------------------------------------------------------- the draws of pad_wide_clips
def test_plan_reproduces_the_reference_draws_and_generator_state(golden):
    g = golden("g23_frame_ingest")
    S = int(g["crop_size"])
    seen = set()
    for seed, h, w in g["cases"].tolist():
        want = g[f"s{seed}.{h}x{w}.pads"]
        torch.manual_seed(seed)
        plan = FR.PadWideClips(S).plan(len(want), h, w)
        assert np.array_equal(torch.get_rng_state().numpy(), g[f"s{seed}.{h}x{w}.state"])
        for p, row in zip(plan, want):
            mode = G_MODES[int(row[0])]
            seen.add(mode)
            assert p.mode == mode and (p.pad_top, p.pad_bottom) == (int(row[1]), int(row[2])) and tuple(p.colour) == tuple(int(v) for v in row[4:7])
            if mode == "reflect":                                     # (the only mode whose alpha reaches cv2)
                assert p.alpha == float(row[3])
            if w <= h:
                assert p == FR.NO_PAD
    assert seen == set(G_MODES.values())


# ---------------------------------------------------------------------------------------------------- the plan check
def table_of(pads, H, W, S_h, S_w):
    return FR.pad_table([FR.Pad(*p) for p in pads], len(pads), H, W, S_h, S_w)


GOOD = [("reflect", 3, 9, 0.25, (0, 0, 0)), (None, 0, 0, 0.0, (0, 0, 0)), ("color", 9, 0, 0.0, (1, 2, 255)), ("replicate", 0, 0, 0.1, (0, 0, 0))]


def check(tab, B, nv, H, W, S_h, S_w, n_words=None):
    return _lib.load().tad_frame_resize_plan_check(tab.ctypes.data, tab.size if n_words is None else n_words, B, nv, H, W, S_h, S_w)


def test_plan_check_accepts_the_host_tables():
    for (H, W), (S_h, S_w) in ALL_SHAPES:
        pads = [(m, min(t, H), min(b, H), a, c) for m, t, b, a, c in GOOD]
        table, nv = table_of(pads, H, W, S_h, S_w)
        assert table.dtype == torch.int32 and table.numel() * 4 == _lib.load().tad_frame_resize_workspace_bytes(4, nv, S_h, S_w)
        assert nv == len({(t + b if m else 0) for m, t, b, _, _ in pads})
        assert check(table.numpy(), 4, nv, H, W, S_h, S_w) == 0
    assert _lib.load().tad_frame_resize_workspace_bytes(0, 1, 4, 4) == 0


def test_plan_check_refuses_malformed_tables():
    H, W, S_h, S_w = 9, 13, 6, 7
    table, nv = table_of(GOOD, H, W, S_h, S_w)
    good = table.numpy()
    assert nv == 3 and check(good, 4, nv, H, W, S_h, S_w) == 0
    rows, hset = 4 * _lib.FR_ROW_WORDS, 4 * _lib.FR_ROW_WORDS
    vset0 = hset + _lib.FR_SET_HEAD + 5 * S_w
    lib = _lib.load()

    def refused(tab, match, **kw):
        assert check(tab, 4, nv, H, W, S_h, S_w, **kw) != 0
        msg = lib.tad_last_error_string().decode()
        assert match in msg, msg

    refused(good, "words, expected", n_words=good.size - 1)                        # the wrong word count
    assert check(good[:-1].copy(), 4, nv, H, W, S_h, S_w) != 0
    bad = good.copy(); bad[1 * _lib.FR_ROW_WORDS] = 0
    refused(bad, "has two rows")                                                   # a sample named twice
    bad = good.copy(); bad[0] = 4
    refused(bad, "outside the batch")
    bad = good.copy(); bad[2] = H + 1
    refused(bad, "greater than H")                                                 # a pad greater than H
    bad = good.copy(); bad[2 * _lib.FR_ROW_WORDS + 3] = H + 1
    refused(bad, "greater than H")
    bad = good.copy(); bad[2] = -1
    refused(bad, "negative pad")
    bad = good.copy(); bad[1] = 4
    refused(bad, "unknown mode")
    bad = good.copy(); bad[_lib.FR_ROW_WORDS + 2] = 1
    refused(bad, "mode none with pads")
    bad = good.copy(); bad[4] = np.float32(1.5).view(np.int32)
    refused(bad, "alpha")
    bad = good.copy(); bad[6] = nv
    refused(bad, "vertical set")
    bad = good.copy(); bad[3] = 8                                                  # the row's set is stated for another virtual height
    refused(bad, "its vertical set is stated for")
    bad = good.copy(); bad[hset] = W + 1
    refused(bad, "horizontal set: input extent")
    bad = good.copy(); bad[hset + _lib.FR_SET_HEAD + S_w - 1] = W - 1              # a tap outside the (virtual) source
    refused(bad, "outside the 13 samples")
    bad = good.copy(); bad[hset + _lib.FR_SET_HEAD] = -3
    refused(bad, "outside the 13 samples")
    bad = good.copy(); bad[vset0 + _lib.FR_SET_HEAD + 2] = good[vset0] - 1
    refused(bad, "vertical set 0: output 2 has its first tap at")
    bad = good.copy(); bad[hset + _lib.FR_SET_HEAD + S_w + 4 * 3 + 1] = 2819       # |k| sums over the bound
    refused(bad, "sum |k|")
    bad = good.copy(); bad[vset0 + _lib.FR_SET_HEAD + S_h + 2] = -2819
    refused(bad, "sum |k|")
    bad = good.copy(); bad[vset0] = 3 * H + 1
    refused(bad, "virtual height")
    bad = good.copy(); bad[vset0 + 1] = S_h + 1
    refused(bad, "output extent")
    assert rows == hset and check(good, 4, nv, H, W, S_h, S_w) == 0                # (the good table is still good)


def test_host_refusals():
    with pytest.raises(TadError, match="second reflection"):
        table_of([("reflect", 10, 0, 0.1, (0, 0, 0))], 9, 13, 6, 7)
    with pytest.raises(TadError, match="second reflection"):
        table_of([("black", 0, 10, 0.1, (0, 0, 0))], 9, 13, 6, 7)
    with pytest.raises(TadError, match="unknown pad mode"):
        table_of([("wrap", 1, 1, 0.1, (0, 0, 0))], 9, 13, 6, 7)
    with pytest.raises(TadError, match="three bytes"):
        table_of([("color", 1, 1, 0.1, (0, 0, 256))], 9, 13, 6, 7)
    with pytest.raises(TadError, match="pads for"):
        FR.pad_table([FR.NO_PAD], 2, 9, 13, 6, 7)
    with pytest.raises(TadError):
        FR.cubic_coeffs(0, 4)
    with pytest.raises(TadError, match="rows for"):
        K.frame_resize_table([], (13, *FR.cubic_coeffs(13, 7)), [(9, *FR.cubic_coeffs(9, 6))], 1, 9, 13, 6, 7)
    with pytest.raises(TadError, match="a set with first"):
        K.frame_resize_table([(0, 0, 0, 0, 0.0, (0, 0, 0), 0)], (13, *FR.cubic_coeffs(13, 6)), [(9, *FR.cubic_coeffs(9, 6))], 1, 9, 13, 6, 7)


def test_null_pointers_return_before_any_launch():
    lib = _lib.load()
    assert lib.tad_frame_resize(None, None, 0, None, None, None, 0, 1, 1, 4, 4, 2, 2, 1, None) == -1
    assert b"null pointer" in lib.tad_last_error_string()
    assert lib.tad_frame_resize_plan_check(None, 0, 1, 1, 4, 4, 2, 2) == -1
    assert b"null pointer" in lib.tad_last_error_string()


def test_cpu_tensors_raise():
    x = torch.zeros((2, 3, 9, 13, 3), dtype=torch.uint8)
    with pytest.raises(TadError, match="no CPU path"):
        FR.resize_frames(x, 8)
    with pytest.raises(TadError, match="no CPU path"):
        FR.resize_frames(x[0], (6, 7))
    with pytest.raises(TadError, match="no CPU path"):
        FR.PadWideClips(8)(x)
    with pytest.raises(TadError, match="GPU tensor"):
        K.frame_resize(x, torch.zeros(8, dtype=torch.int32), 1, 8, 8)
    with pytest.raises(TadError):
        FR.resize_frames(x, 0)
    from simple_tad_amd import FrameStore
    with pytest.raises(TadError, match="no CPU path"):
        FrameStore(4, 8, 8, "cpu").append_resized(x[0])
    with pytest.raises(TypeError, match="uint8 frames"):
        FrameStore(4, 8, 8, "cpu").append_resized(x[0].float())


def test_header_and_binding_list_the_same_symbols():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tad_mi355x.h")).read()
    declared = set(re.findall(r"\b(tad_frame_resize\w*)\s*\(", header))
    assert declared == {n for n in _lib.SIGNATURES if n.startswith("tad_frame_resize")} == \
        {"tad_frame_resize", "tad_frame_resize_plan_check", "tad_frame_resize_workspace_bytes"}
    assert _lib.load().tad_abi_version() == 5
    for name, value in (("ROW_WORDS", _lib.FR_ROW_WORDS), ("SET_HEAD", _lib.FR_SET_HEAD), ("MAX_SETS", _lib.FR_MAX_SETS),
                        ("MAX_ABS_SUM", _lib.FR_MAX_ABS_SUM), ("NONE", _lib.FR_NONE), ("CONST", _lib.FR_CONST), ("REFLECT", _lib.FR_REFLECT),
                        ("REPLICATE", _lib.FR_REPLICATE)):
        assert re.search(rf"#define TAD_FR_{name} {value}\b", header), name
