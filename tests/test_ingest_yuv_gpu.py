"""The YUV ingest kernel alone (tady_ingest_yuv, include/tad_mi355x_yuv.h): K pitched NV12 / NV21 / I420 frames of K sizes in one packed
buffer, one launch, each converted and resized into a slot of its own -- bit for bit over every byte against the numpy restatement of
the conversion (tests/yuv_recipe.py) followed by the numpy restatement of the resize (tests/frame_resize_recipe.py), and on the device
against ``kernels.ingest_frames`` fed the recipe-converted RGB frames.  The surfaces are laid out here, by the recipe's packers, at
offsets of every phase, with pitch padding, gaps between planes and gaps between frames; the tables go through
``kernels.ingest_yuv_table`` (the plan check).  The last test hands the raw C entry a table the plan check would refuse: the header
states what the device does with it, and that is what is checked -- inside one guarded allocation, after the well-formed cases."""
import numpy as np
import pytest
import torch

import frame_resize_recipe as R
import yuv_recipe as Y
from guarded import GuardedArena

pytestmark = pytest.mark.gpu

POISON = 0xA5
HEAD = 8
DESTS = [(16, 16), (28, 28), (35, 33)]  # (35, 33): S_h != S_w, one output past a tile edge on both axes
FORMATS = ("nv12", "nv21", "i420")
CSETS = Y.colour_sets()
# (h, w) of the sources of the mixed call: the n_src = 1 tap range on either axis, the smallest chroma plane, odd extents, an up-scale, a
# down-scale, even extents, a vertical shrink above 4 (four slots per output row), and a second frame of an earlier size
SOURCES = [(1, 1), (1, 9), (9, 1), (2, 2), (5, 7), (20, 23), (16, 12), (150, 12), (5, 7)]


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import _lib, kernels
    _lib.load()
    return kernels


def spec(h, w, i, matrix=None):
    """frame i of a call: its planes, and a layout chosen by its index -- the three formats in turn, pitches w, w + 1 and w + 13 (the
    chroma pitch likewise from its own live bytes), gaps between the planes on every second frame, B first on two of every four"""
    fmt = FORMATS[i % 3]
    step = 1 if fmt == "i420" else 2
    pad = (0, 1, 13)[(i // 3 + i) % 3]
    return dict(planes=Y.planes(h, w, i), fmt=fmt, y_pitch=w + pad, c_pitch=(w + 1) // 2 * step + pad, gap=(i % 2) * 3, gap2=(i % 2) * 5,
                matrix=matrix or ("bt601", "bt709")[i % 2], bgr=bool(i % 4 >= 2))


def lay_out(specs, slots, dst, F, fill=0x00, rng=None, end_phase=None):
    """(src uint8 numpy ending on the last live byte, table CPU tensor, src_bytes, nh, nv, nc): the surfaces one behind the other, k % 4
    dead bytes in front of frame k (so the planes start at every phase of a word), every byte that is no live sample ``fill`` or random"""
    from simple_tad_amd import kernels
    from simple_tad_amd.frame_resize import cubic_coeffs
    hsets, vsets, csets, rows, parts = {}, {}, {}, [], []
    at = HEAD
    parts.append(rng.randint(0, 256, HEAD).astype(np.uint8) if rng is not None else np.full(HEAD, fill, np.uint8))
    for k, (s, slot) in enumerate(zip(specs, slots)):
        buf, lay = Y.pack(*s["planes"], s["fmt"], s["y_pitch"], s["c_pitch"], s["gap"], s["gap2"], fill, rng)
        dead = k % 4
        if end_phase is not None and k == len(specs) - 1:
            dead = (end_phase - at - lay["nbytes"]) % 4
        parts.append(rng.randint(0, 256, dead).astype(np.uint8) if rng is not None else np.full(dead, fill, np.uint8))
        at += dead
        h, w = lay["h"], lay["w"]
        rows.append((at, lay["y_pitch"], at + lay["u_off"], at + lay["v_off"], lay["c_pitch"], lay["c_step"], h, w, slot,
                     hsets.setdefault(w, len(hsets)), vsets.setdefault(h, len(vsets)), csets.setdefault(CSETS[s["matrix"]], len(csets)),
                     1 if s["bgr"] else 0))
        parts.append(buf)
        at += lay["nbytes"]
    table = kernels.ingest_yuv_table(rows, [(w, *cubic_coeffs(w, dst[1])) for w in hsets], [(h, *cubic_coeffs(h, dst[0])) for h in vsets],
                                     list(csets), at, F, *dst)
    src = np.concatenate(parts)
    assert src.size == at
    return src, table, at, len(hsets), len(vsets), len(csets)


def on_device(src):
    """the bytes on the GPU, in an allocation that reaches the next multiple of 4 (the header's slack), the slack 0xFF"""
    n = (src.size + 3) // 4 * 4
    d = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
    d[:src.size] = torch.from_numpy(src).cuda()
    return d


def ingest(K, specs, slots, dst, F, **kw):
    src, table, nbytes, nh, nv, nc = lay_out(specs, slots, dst, F, **kw)
    store = torch.full((F, *dst, 3), POISON, dtype=torch.uint8, device="cuda")
    out = K.ingest_yuv(on_device(src), nbytes, store, table.cuda(), len(specs), nh, nv, nc)
    assert out is store
    return store.cpu().numpy()


_WANT = {}


def converted(s):
    """the recipe's conversion of one frame, in the channel order its flag asks for"""
    return Y.convert(*s["planes"], CSETS[s["matrix"]], bgr=s["bgr"])


def want(s, dst):
    """the recipe's conversion and resize of one frame, computed once and left unchanged"""
    key = (tuple(p.tobytes() for p in s["planes"]), s["planes"][0].shape, s["matrix"], s["bgr"], dst)
    if key not in _WANT:
        r = R.resize(converted(s)[None], *dst)[0]
        r.setflags(write=False)
        _WANT[key] = r
    return _WANT[key]


def expected(specs, slots, dst, F):
    e = np.full((F, *dst, 3), POISON, dtype=np.uint8)
    for s, slot in zip(specs, slots):
        e[slot] = want(s, dst)
    return e


@pytest.mark.parametrize("dst", DESTS, ids=[f"{a}x{b}" for a, b in DESTS])
def test_one_mixed_call_equals_the_recipes_and_ingest_frames(K, dst):
    from simple_tad_amd import stream_bank as SB
    specs = [spec(h, w, i) for i, (h, w) in enumerate(SOURCES)] + [spec(*dst, len(SOURCES))]   # the last one is at S_h x S_w already
    specs[8] = dict(spec(5, 7, 8), fmt=specs[4]["fmt"], c_pitch=specs[4]["c_pitch"], matrix=specs[4]["matrix"])  # frames 4 and 8 share all three sets
    n = len(specs)
    F = n + 3
    slots = [(7 * i + 2) % F for i in range(n)]                                                 # scattered, out of order (7 and F = 13 coprime)
    assert len(set(slots)) == n and slots != sorted(slots) and F % 7
    assert {s["fmt"] for s in specs} == set(FORMATS) and {s["bgr"] for s in specs} == {True, False} and {s["matrix"] for s in specs} == {"bt601", "bt709"}
    assert {s["y_pitch"] - s["planes"][0].shape[1] for s in specs} == {0, 1, 13}
    got = ingest(K, specs, slots, dst, F)
    exp = expected(specs, slots, dst, F)
    for k, s in enumerate(slots):
        assert np.array_equal(got[s], exp[s]), f"frame {k} {SOURCES[k] if k < len(SOURCES) else dst} {specs[k]['fmt']} -> {dst}, slot {s}"
    untouched = sorted(set(range(F)) - set(slots))
    assert len(untouched) == 3 and (got[untouched] == POISON).all()
    assert np.array_equal(got, exp), "every byte of the store"
    assert np.array_equal(got[slots[-1]], converted(specs[-1])), "equal extents give the converted bytes back"
    assert not np.array_equal(got[slots[4]], got[slots[8]]), "equal sizes and sets, their own bytes"
    # on the device: the RGB ingest on the frames the recipe converted (already in the stored channel order: no swap)
    rgb = [converted(s) for s in specs]
    table, offsets, nbytes, nh, nv = SB.plan_ingest([f.shape[:2] for f in rgb], slots, [False] * n, *dst, F)
    src = np.zeros(nbytes + SB._HEAD, dtype=np.uint8)
    for f, at in zip(rgb, offsets):
        src[at:at + f.size] = f.reshape(-1)
    ref = torch.full((F, *dst, 3), POISON, dtype=torch.uint8, device="cuda")
    K.ingest_frames(torch.from_numpy(src).cuda(), nbytes, ref, table.cuda(), n, nh, nv)
    assert np.array_equal(ref.cpu().numpy(), got)
    # two calls give the same bits
    assert np.array_equal(ingest(K, specs, slots, dst, F), got)


@pytest.mark.parametrize("matrix", sorted(CSETS))
def test_colour_sweep_at_equal_extents(K, matrix):
    """every Y 0 .. 255 with every (U, V) of 13 x 13 values around the ends, the offsets and the centre: 169 pairs x 64 chroma blocks of
    four luma samples = one 208 x 208 frame; at equal extents the store holds the conversion itself"""
    vals = np.asarray([0, 1, 15, 16, 17, 127, 128, 129, 239, 240, 241, 254, 255], dtype=np.uint8)
    block = np.arange(104 * 104)
    pair, q = block // 64, block % 64
    U = vals[pair // 13].reshape(104, 104)
    V = vals[pair % 13].reshape(104, 104)
    Yp = np.zeros((208, 208), dtype=np.uint8)
    base = (q * 4).reshape(104, 104)
    Yp[0::2, 0::2], Yp[0::2, 1::2], Yp[1::2, 0::2], Yp[1::2, 1::2] = base, base + 1, base + 2, base + 3
    seen = set(zip(Yp.reshape(-1).tolist(), np.repeat(np.repeat(U, 2, 0), 2, 1).reshape(-1).tolist(), np.repeat(np.repeat(V, 2, 0), 2, 1).reshape(-1).tolist()))
    assert len(seen) == 256 * 169, "every (Y, U, V) of the sweep, once"
    for i, fmt in enumerate(FORMATS if matrix == "bt601" else FORMATS[:1]):
        s = dict(planes=(Yp, U, V), fmt=fmt, y_pitch=208 + i, c_pitch=(104 if fmt == "i420" else 208) + i, gap=i, gap2=0, matrix=matrix, bgr=False)
        got = ingest(K, [s], [0], (208, 208), 1)[0]
        exp = Y.convert_samples(Yp, np.repeat(np.repeat(U, 2, 0), 2, 1), np.repeat(np.repeat(V, 2, 0), 2, 1), CSETS[matrix])
        assert np.array_equal(got, exp), (matrix, fmt)


def test_dead_bytes_and_neighbours_do_not_matter(K):
    """odd frames must come out the same whatever the pitch padding, the gaps between planes and between frames, the slack around the
    buffer and the even frames hold: zeros, 0xFF, random bytes"""
    dst = (16, 16)
    shapes = [(3, 3), (5, 7), (2, 1), (9, 1), (1, 9), (4, 6), (3, 5), (20, 23), (1, 1), (6, 3)]
    a = [dict(spec(h, w, 10 + i), y_pitch=w + 1 + i % 5, gap=1 + i % 3, gap2=2) for i, (h, w) in enumerate(shapes)]
    for s in a:
        s["c_pitch"] += 3
    flat = lambda s, v: dict(s, planes=tuple(np.full_like(p, v) for p in s["planes"]))
    b = [s if i % 2 else flat(s, 0xFF) for i, s in enumerate(a)]
    c = [s if i % 2 else flat(s, 0x00) for i, s in enumerate(a)]
    slots = list(range(len(shapes)))[::-1]
    ga = ingest(K, a, slots, dst, len(shapes), fill=0x00)
    gb = ingest(K, b, slots, dst, len(shapes), fill=0xFF)
    gc = ingest(K, c, slots, dst, len(shapes), rng=np.random.RandomState(77))
    for i in range(1, len(shapes), 2):
        assert np.array_equal(ga[slots[i]], want(a[i], dst)), i
        assert np.array_equal(gb[slots[i]], ga[slots[i]]) and np.array_equal(gc[slots[i]], ga[slots[i]]), i
    for i in range(0, len(shapes), 2):
        assert np.array_equal(gb[slots[i]], want(b[i], dst)) and np.array_equal(gc[slots[i]], want(c[i], dst)), i


def test_one_frame_and_sixty_four(K):
    dst = (4, 4)
    s = spec(3, 5, 0)
    got = ingest(K, [s], [1], dst, 2)
    assert np.array_equal(got[1], want(s, dst)) and (got[0] == POISON).all()
    sizes = [(1, 1), (2, 3), (3, 2), (4, 4), (5, 2)]
    specs = [spec(*sizes[i % 5], 100 + i) for i in range(64)]
    F = 66
    slots = [(37 * i + 11) % F for i in range(64)]
    assert len(set(slots)) == 64
    got = ingest(K, specs, slots, dst, F)
    assert np.array_equal(got, expected(specs, slots, dst, F))


@pytest.fixture(scope="module")
def arena():
    return GuardedArena(8 << 20, "cuda")


def _guarded_operands(arena, src, table, F, dst, store_offset):
    zeros = torch.zeros(16, dtype=torch.int32)
    x = arena.place(torch.from_numpy(src), name="src")
    t = arena.place(table, guard_pattern=(zeros, zeros), name="table")
    store = arena.place((F, *dst, 3), torch.uint8, role="output", name="store", fill=POISON, offset=store_offset)
    return x, t, store


GUARD_SOURCES = [(5, 7), (20, 23), (1, 9), (150, 12), (9, 5)]


@pytest.mark.parametrize("store_offset", [0, 1, 2, 3])
def test_guard_bands(K, arena, store_offset):
    """src, table and store each between two poisoned bands of one allocation (0xFF around the bytes, zero rows around the table), the
    store at every phase of a word: nothing outside the store changes, inside it only the named slots do, and the results are the
    recipes' -- they depend on no byte outside the planes.  The last frame's last plane ends on the last byte of src's body, one byte
    past a multiple of 4 + 2, so the word that holds its last sample reaches into the guard."""
    dst = (16, 16)
    specs = [spec(h, w, 40 + i) for i, (h, w) in enumerate(GUARD_SOURCES)]
    F = len(specs) + 2
    slots = [4, 0, 6, 2, 5]
    src, table, nbytes, nh, nv, nc = lay_out(specs, slots, dst, F, fill=0xFF, end_phase=3)
    assert nbytes % 4 == 3 and src.size == nbytes
    arena.reset()
    x, t, store = _guarded_operands(arena, src, table, F, dst, store_offset)
    assert store.data_ptr() % 4 == store_offset and x.data_ptr() % 4 == 0
    at = x.data_ptr() - arena.buf.data_ptr()
    slack = arena.buf[at:at + nbytes + 1]                                                   # the allocation's slack up to a multiple of 4: one guard byte
    assert slack.data_ptr() == x.data_ptr() and int(slack[-1]) == 0xFF
    K.ingest_yuv(slack, nbytes, store, t, len(specs), nh, nv, nc)
    arena.verify()
    assert np.array_equal(store.cpu().numpy(), expected(specs, slots, dst, F))


def test_a_malformed_device_table_is_never_an_address(K, arena):
    """The header's stated defence, through the raw C entry (the Python wrapper's table has passed the plan check, which refuses every
    row below): a row whose extents are below 1, whose c_step is not 1 or 2, one of whose pitches is below its live bytes or one of
    whose planes does not fit in src is ignored; a slot is clamped into the store; a set index is clamped into its sets (the taps are
    clamped to the row's own extents whatever the set says).  Every value is one for which a kernel that honours those clamps forms no
    address outside its operands, and everything lies inside one guarded allocation; the well-formed rows give the recipes' bytes."""
    from simple_tad_amd import _lib
    dst = (16, 16)
    shapes = [(5, 7), (20, 23), (9, 5), (4, 6), (7, 50), (3, 3), (6, 3), (8, 8), (6, 10), (12, 4), (5, 5)]
    specs = [spec(h, w, 60 + i) for i, (h, w) in enumerate(shapes)]
    n = len(specs)
    F = n + 3                                                                               # slots n .. n + 2 are named by no row
    slots = [3, 0, 6, 2, 5, 1, 4, 7, 8, 9, 10]
    src, table, nbytes, nh, nv, nc = lay_out(specs, slots, dst, F, fill=0xFF)
    lib = _lib.load_yuv()
    tab = table.numpy().copy()
    R_ = _lib.YUV_ROW_WORDS
    rows = tab[:n * R_].reshape(n, R_)
    rows[1, 0] = nbytes - 8                       # a 20 x 23 luma plane 8 bytes in front of the end of src: ignored
    rows[2, 8] = F + 5                            # a slot past the store: clamped to F - 1
    rows[3, 9], rows[3, 10], rows[3, 11] = 99, -7, 77  # set indices out of range: clamped to the last horizontal, the first vertical, the last colour set
    rows[5, 6] = 0                                # an extent below 1: ignored
    rows[6, 0] = -4                               # a negative luma offset: ignored
    rows[7, 5] = 3                                # a chroma step that is neither 1 nor 2: ignored
    rows[8, 4] = 1                                # a chroma pitch below the live bytes: ignored
    rows[9, 2] = nbytes - 1                       # a U plane that ends behind src: ignored
    rows[10, 3] = -1                              # a V plane in front of src: ignored
    assert rows[8, 4] < (10 + 1) // 2 * rows[8, 5]
    assert lib.tady_ingest_plan_check(tab.ctypes.data, tab.size, n, nh, nv, nc, nbytes, F, *dst) == -1
    arena.reset()
    x, t, store = _guarded_operands(arena, np.concatenate([src, np.full((-src.size) % 4, 0xFF, np.uint8)]), torch.from_numpy(tab), F, dst, 0)
    rc = lib.tady_ingest_yuv(x.data_ptr(), nbytes, store.data_ptr(), F, t.data_ptr(), t.numel(), n, nh, nv, nc, *dst,
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.tady_last_error_string()
    arena.verify()                                                                          # nothing outside the store has changed
    got = store.cpu().numpy()
    for k in (0, 4):                                                                        # the other rows' results are unchanged
        assert np.array_equal(got[slots[k]], want(specs[k], dst)), k
    assert np.array_equal(got[F - 1], want(specs[2], dst)), "the clamped slot"
    for s in [slots[k] for k in (1, 2, 5, 6, 7, 8, 9, 10)] + [n, n + 1]:                    # ignored rows, the slot row 2 named no longer, spare slots
        assert (got[s] == POISON).all(), s
    assert (got[slots[3]] != POISON).any()                                                  # row 3 wrote its own slot, with other sets' coefficients
