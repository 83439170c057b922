"""The YUV ingest's host side without a GPU: the recipe's own fixed points (tests/yuv_recipe.py), the pinned integers of the four colour
sets and their int32 bound, the packers, the table builder (stream_bank.plan_ingest_yuv: offsets, set sharing, flags, the cache) and
``YuvFrame``'s refusals."""
import numpy as np
import pytest
import torch

import yuv_recipe as Y
from simple_tad_amd import _lib, stream_bank as SB
from simple_tad_amd._lib import TadError
from simple_tad_amd.frame_resize import cubic_coeffs

# the integers of the four sets: {y_off, cy, cvr, cug, cvg, cub}.  bt601 is the literal set; the others are the derivation's, pinned
PINNED = {"bt601": (16, 1220542, 1673527, -409993, -852492, 2116026),
          "bt709": (16, 1220945, 1879825, -223607, -558796, 2215014),
          "bt601-full": (0, 1048576, 1470104, -360853, -748826, 1858077),
          "bt709-full": (0, 1048576, 1651297, -196424, -490864, 1945738)}


def test_pinned_integers_of_the_four_colour_sets():
    assert Y.colour_sets() == PINNED, "the recipe's derivation"
    assert SB.COLOUR_SETS == PINNED, "the package's derivation (written on its own) gives the same integers"
    for name, c in PINNED.items():
        assert SB.colour_set(name) == c
        assert c[0] == (0 if name.endswith("-full") else 16) and (c[1] == 1 << 20) == name.endswith("-full")
    # the derivation for BT.601's weights is close to, and not, the literal three-digit set
    d = Y.derive(0.299, 0.114, False)
    assert d != PINNED["bt601"] and all(abs(a - b) <= 1000 for a, b in zip(d, PINNED["bt601"]))
    assert SB.derive_colour_set(0.299, 0.114, False) == d


def test_recipe_fixed_points():
    for name, c in PINNED.items():
        full = name.endswith("-full")
        black, white = (0, 255) if full else (16, 235)
        assert Y.convert_samples([black], [128], [128], c).tolist() == [[0, 0, 0]], name
        assert Y.convert_samples([white], [128], [128], c).tolist() == [[255, 255, 255]], name
        # every luma below the offset clamps to black, every luma above white to white
        below = np.arange(0, black + 1)
        assert (Y.convert_samples(below, np.full_like(below, 128), np.full_like(below, 128), c) == 0).all(), name
        above = np.arange(white, 256)
        assert (Y.convert_samples(above, np.full_like(above, 128), np.full_like(above, 128), c) == 255).all(), name
        # saturation at both ends of each channel: R follows V, B follows U, G falls with both
        mid = 128
        assert Y.convert_samples([mid], [128], [255], c)[0, 0] == 255 and Y.convert_samples([mid], [128], [0], c)[0, 0] == 0, name
        assert Y.convert_samples([mid], [255], [128], c)[0, 2] == 255 and Y.convert_samples([mid], [0], [128], c)[0, 2] == 0, name
        assert Y.convert_samples([200], [0], [0], c)[0, 1] == 255 and Y.convert_samples([60], [255], [255], c)[0, 1] == 0, name
        assert 0 < Y.convert_samples([200], [128], [128], c)[0, 1] < 255 and 0 < Y.convert_samples([60], [128], [128], c)[0, 1] < 255, name
        if full:  # full-range identity on grey
            g = np.arange(256)
            out = Y.convert_samples(g, np.full_like(g, 128), np.full_like(g, 128), c)
            assert (out == g[:, None]).all(), name
    # a value worked by hand, BT.601: Y 81, U 90, V 240 (the red of the colour bars)
    yy = (81 - 16) * 1220542
    want = [(yy + 1673527 * 112 + (1 << 19)) >> 20, (yy - 852492 * 112 - 409993 * -38 + (1 << 19)) >> 20, (yy + 2116026 * -38 + (1 << 19)) >> 20]
    assert Y.convert_samples([81], [90], [240], PINNED["bt601"]).tolist() == [[min(max(v, 0), 255) for v in want]] == [[254, 0, 0]]


def test_nearest_chroma_and_the_packers():
    for fmt in ("nv12", "nv21", "i420"):
        for (h, w) in ((1, 1), (2, 2), (5, 7), (4, 6)):
            Yp, U, V = Y.planes(h, w, 3)
            rgb = Y.convert(Yp, U, V, PINNED["bt601"])
            for (y, x) in ((0, 0), (h - 1, w - 1), (h // 2, w // 2)):
                assert rgb[y, x].tolist() == Y.convert_samples([Yp[y, x]], [U[y >> 1, x >> 1]], [V[y >> 1, x >> 1]], PINNED["bt601"])[0].tolist()
            assert np.array_equal(Y.convert(Yp, U, V, PINNED["bt601"], bgr=True), rgb[..., ::-1])
            cw = (w + 1) // 2
            step = 1 if fmt == "i420" else 2
            for yp, cp, gap, gap2 in ((None, None, 0, 0), (w + 1, cw * step + 1, 3, 5), (w + 13, cw * step + 13, 0, 1)):
                buf, lay = Y.pack(Yp, U, V, fmt, yp, cp, gap, gap2, fill=0xEE)
                back = Y.unpack(buf, lay)
                assert all(np.array_equal(a, b) for a, b in zip(back, (Yp, U, V))), (fmt, h, w, yp)
                assert buf.size == lay["nbytes"]
                live = h * w + 2 * U.size
                assert (buf != 0xEE).sum() <= live and (buf == 0xEE).sum() >= buf.size - live
            if fmt != "i420":
                assert abs(lay["u_off"] - lay["v_off"]) == 1 and (lay["u_off"] < lay["v_off"]) == (fmt == "nv12")


def test_the_int32_bound_holds_for_each_set_and_is_refused_beyond():
    for name, c in PINNED.items():
        assert Y.bound(c) == SB.colour_set_bound(c) < 2 ** 31, name
    # the largest set that passes, and the first that does not: 255 * cy + 128 * cvr + 2^19 = 2^31 - 1 and 2^31
    cy = 1 << 20
    cvr = (2 ** 31 - 1 - (1 << 19) - 255 * cy) // 128
    ok = (0, cy, cvr, 0, 0, 0)
    assert 255 * cy + 128 * cvr + (1 << 19) <= 2 ** 31 - 1 < 255 * cy + 128 * (cvr + 1) + (1 << 19)
    assert SB.colour_set(ok) == ok
    for bad in ((0, cy, cvr + 1, 0, 0, 0), (0, cy, 0, 0, 0, -(cvr + 1)), (0, cy, 0, (cvr + 1) // 2 + 1, -(cvr + 1) // 2, 0), (256, cy, 0, 0, 0, 0),
                (0, -1, 0, 0, 0, 0)):
        with pytest.raises(TadError, match="colour_set"):
            SB.colour_set(bad)
    with pytest.raises(TadError, match="unknown matrix 'bt2020'"):
        SB.colour_set("bt2020")
    with pytest.raises(TadError, match="six integers"):
        SB.colour_set((16, 1, 2))
    # the library's own check of the same bound (the Python check is bypassed: the table builder is handed the set directly)
    from simple_tad_amd import kernels as K
    hs, vs = [(2, *cubic_coeffs(2, 4))], [(2, *cubic_coeffs(2, 4))]
    row = [(0, 2, 4, 5, 2, 2, 2, 2, 0, 0, 0, 0, 0)]
    assert K.ingest_yuv_table(row, hs, vs, [ok], 8, 1, 4, 4).numel() == 16 + 2 * 24 + 8
    with pytest.raises(TadError, match=r"colour set 0: 255 \* cy \+ 128 \* max\|c\| \+ 2\^19 = 2147483648 reaches 2\^31"):
        K.ingest_yuv_table(row, hs, vs, [(0, cy, cvr + 1, 0, 0, 0)], 8, 1, 4, 4)


def _frames():
    """six frames of three layouts; frames 0 and 2 are alike in everything, frame 5 shares frame 1's height and frame 0's width"""
    mk = lambda h, w, fmt, yp=None, cp=None, m="bt601": SB.YuvFrame(np.zeros(4 * (h + 2) * ((yp or w) + 16), np.uint8), h, w, fmt, yp, cp, m)
    return [mk(5, 7, "nv12"), mk(20, 23, "i420", 24, 13, "bt709"), mk(5, 7, "nv12"), mk(16, 12, "nv21", 25), mk(1, 1, "i420"),
            mk(20, 7, "nv12", 8, 21, "bt709")]


def test_plan_offsets_set_sharing_and_flags():
    fs = _frames()
    slots = [9, 0, 4, 11, 2, 7]
    bgrs = [False, True, True, False, False, True]
    S_h, S_w = 16, 12
    table, offsets, nbytes, nh, nv, nc = SB.plan_ingest_yuv([f.layout for f in fs], slots, bgrs, S_h, S_w, 12)
    table = table.numpy()
    assert (nh, nv, nc) == (4, 4, 2), "one set per distinct w (7, 23, 12, 1), per distinct h (5, 20, 16, 1), per distinct colour set"
    R, H = _lib.YUV_ROW_WORDS, _lib.FR_SET_HEAD
    rows = table[:len(fs) * R].reshape(len(fs), R)
    at = SB._HEAD
    for k, f in enumerate(fs):
        ch, cw = (f.h + 1) // 2, (f.w + 1) // 2
        assert offsets[k] == at == rows[k, 0] and at % 4 == 0
        assert rows[k, 1] == f.y_pitch and rows[k, 4] == f.c_pitch and rows[k, 5] == f.c_step and (rows[k, 6], rows[k, 7]) == (f.h, f.w)
        c_at = at + f.h * f.y_pitch
        if f.format == "i420":
            assert (rows[k, 2], rows[k, 3]) == (c_at, c_at + ch * f.c_pitch) and f.nbytes == f.h * f.y_pitch + (2 * ch - 1) * f.c_pitch + cw
        else:
            assert (rows[k, 2], rows[k, 3]) == ((c_at, c_at + 1) if f.format == "nv12" else (c_at + 1, c_at))
            assert f.nbytes == f.h * f.y_pitch + (ch - 1) * f.c_pitch + 2 * cw
        at += (f.nbytes + 3) // 4 * 4
    assert nbytes == at
    assert rows[:, 8].tolist() == slots and rows[:, 12].tolist() == [_lib.YUV_BGR if b else 0 for b in bgrs] and not rows[:, 13:].any()
    assert rows[0, 9] == rows[2, 9] == rows[5, 9] and rows[1, 10] == rows[5, 10] and rows[0, 10] == rows[2, 10]
    assert rows[:, 11].tolist() == [0, 1, 0, 0, 0, 1]
    at = len(fs) * R
    hsets, vsets = [], []
    for n, size, out in ((nh, S_w, hsets), (nv, S_h, vsets)):
        for _ in range(n):
            out.append((table[at:at + H].tolist(), table[at + H:at + H + size], table[at + H + size:at + H + 5 * size].reshape(size, 4)))
            at += H + 5 * size
    for k, f in enumerate(fs):
        for (head, first, kk), n_in, n_out in ((hsets[rows[k, 9]], f.w, S_w), (vsets[rows[k, 10]], f.h, S_h)):
            assert head == [n_in, n_out, 0, 0]
            assert np.array_equal(first, cubic_coeffs(n_in, n_out)[0]) and np.array_equal(kk, cubic_coeffs(n_in, n_out)[1])
    csets = table[at:].reshape(nc, _lib.YUV_CSET_WORDS)
    assert tuple(csets[0, :6]) == PINNED["bt601"] and tuple(csets[1, :6]) == PINNED["bt709"] and not csets[:, 6:].any()
    assert at + nc * _lib.YUV_CSET_WORDS == table.size


def test_plan_cache_changes_the_slots_only_and_checks_them_again():
    lays = [f.layout for f in _frames()[:3]]
    bgrs = [True, False, False]
    cache = {}
    a = SB.plan_ingest_yuv(lays, [0, 5, 3], bgrs, 8, 8, 6, cache)
    b = SB.plan_ingest_yuv(lays, [1, 4, 3], bgrs, 8, 8, 6, cache)
    fresh = SB.plan_ingest_yuv(lays, [1, 4, 3], bgrs, 8, 8, 6)
    assert len(cache) == 1 and torch.equal(b[0], fresh[0]) and b[1:] == fresh[1:]
    assert (a[0] != b[0]).nonzero().flatten().tolist() == [8, _lib.YUV_ROW_WORDS + 8]
    assert a[0][8] == 0 and a[0][_lib.YUV_ROW_WORDS + 8] == 5, "the cached table is not the one handed out"
    with pytest.raises(TadError, match="row 1: slot=6 outside the store"):
        SB.plan_ingest_yuv(lays, [1, 6, 3], bgrs, 8, 8, 6, cache)
    with pytest.raises(TadError, match="slot=3 is already named by row 0"):
        SB.plan_ingest_yuv(lays, [3, 4, 3], bgrs, 8, 8, 6, cache)
    SB.plan_ingest_yuv(lays, [1, 4, 3], [False] * 3, 8, 8, 6, cache)
    assert len(cache) == 2, "other flags are another table"
    other = SB.YuvFrame(np.zeros(400, np.uint8), 5, 7, "nv12", matrix="bt709-full").layout
    SB.plan_ingest_yuv([other] + lays[1:], [1, 4, 3], [False] * 3, 8, 8, 6, cache)
    assert len(cache) == 3, "another colour set is another table"


def test_yuv_frame_refusals_and_the_bare_array():
    buf = np.zeros(4096, np.uint8)
    ok = SB.YuvFrame(buf, 6, 8)
    assert (ok.format, ok.y_pitch, ok.c_pitch, ok.c_step, ok.nbytes, ok.cset) == ("nv12", 8, 8, 2, 72, PINNED["bt601"])
    assert SB.YuvFrame(buf, 5, 7, "i420").nbytes == 35 + 2 * 3 * 4 and SB.YuvFrame(buf, 5, 7, "nv21").nbytes == 35 + 3 * 8
    assert SB.YuvFrame(buf, 5, 7, "nv12", 20, 16).nbytes == 100 + 2 * 16 + 8, "the last row stops at its last live byte"
    assert SB.YuvFrame(torch.zeros((9, 8), dtype=torch.uint8), 6, 8).nbytes == 72, "a tensor, any shape"
    for args, kw, exc, text in (((buf, 6, 8), dict(format="yuyv"), TadError, "format 'yuyv' must be one of"),
                                ((buf, 0, 8), {}, TadError, "a frame of 0 x 8 pixels"),
                                ((buf, 6, _lib.YUV_MAX_EXTENT + 1), {}, TadError, "pixels must have 1 .. 32768 per side"),
                                ((buf, 6, 8), dict(y_pitch=7), TadError, "y_pitch=7 is below the 8 bytes of a luma row"),
                                ((buf, 6, 7), dict(c_pitch=7), TadError, "c_pitch=7 is below the 8 bytes of a nv12 chroma row"),
                                ((buf, 6, 7), dict(format="i420", c_pitch=3), TadError, "c_pitch=3 is below the 4 bytes of a i420 chroma row"),
                                ((buf[:71], 6, 8), {}, TadError, r"71 bytes do not hold a nv12 frame of 6 x 8 .* \(72 bytes\)"),
                                ((buf, 6, 8), dict(matrix="rec2020"), TadError, "unknown matrix 'rec2020'"),
                                ((buf.astype(np.int8), 6, 8), {}, TypeError, "data must be a uint8 numpy array or CPU tensor"),
                                (("frame.yuv", 6, 8), {}, TypeError, "but got str")):
        with pytest.raises(exc, match=text):
            SB.YuvFrame(*args, **kw)
    # the bare array: uint8 [h * 3 / 2, w], even h and w -- a contiguous NV12 frame
    bare = SB.YuvFrame.of(np.zeros((9, 8), np.uint8), 0)
    assert (bare.h, bare.w, bare.format, bare.y_pitch, bare.c_pitch, bare.nbytes) == (6, 8, "nv12", 8, 8, 72)
    assert SB.YuvFrame.of(ok) is ok
    for bad in (np.zeros((9, 7), np.uint8), np.zeros((8, 8), np.uint8), np.zeros((9, 8, 1), np.uint8), np.zeros((9, 8), np.float32), "x"):
        with pytest.raises(TypeError, match=r"Input 3 must be a YuvFrame or a uint8 array"):
            SB.YuvFrame.of(bad, 3)
    import simple_tad_amd as T
    from simple_tad_amd import kernels
    assert T.YuvFrame is SB.YuvFrame and callable(kernels.ingest_yuv) and callable(kernels.ingest_yuv_table)
    assert callable(T.StreamBank.push_yuv)
    with pytest.raises(TadError, match="expected a GPU tensor"):
        kernels.ingest_yuv(torch.zeros(64, dtype=torch.uint8), 64, torch.zeros((1, 4, 4, 3), dtype=torch.uint8), torch.zeros(8, dtype=torch.int32), 1, 1, 1, 1)
