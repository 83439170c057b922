"""The ragged ingest kernel alone (tadb_ingest_frames, include/tad_mi355x_bank.h): K frames of K sizes in one packed buffer, one launch,
each resized into a slot of its own -- against the numpy restatement of the resize contract (tests/frame_resize_recipe.py), bit for bit
over whole stores, and on the device against ``resize_frames`` called once per frame.  One call mixes the smallest shapes at which the
kernel can go wrong; the slots are scattered and out of order in a store of a few more slots than frames, and the untouched slots must
keep their poison.  The last test hands the raw C entry a table the plan check would refuse: the header states what the device does
with it (skip the row, clamp the slot, clamp the set index), and that is what is checked -- inside one guarded allocation."""
import numpy as np
import pytest
import torch

import frame_resize_recipe as R
from guarded import GuardedArena

pytestmark = pytest.mark.gpu

POISON = 0xA5
DESTS = [(16, 16), (28, 28), (35, 33)]  # (35, 33): S_h != S_w, one output past a tile edge on both axes
# (h, w) of the sources of the mixed call.  3w mod 4: w = 1, 23, 7, 9 -> 3, 1, 1, 3; w = 6, 50 -> 2; w = 3 -> 1; w = 12 -> 0
SOURCES = [(1, 1), (1, 9), (9, 1),       # the n_src = 1 tap range on either axis
           (5, 7),                       # up-scale on both axes
           (20, 23),                     # the project's fixture; a down-scale on both axes towards 16 x 16
           (4, 6), (6, 3),               # 3w mod 4 = 2 and 1
           (40, 10), (7, 50),            # down-scale vertically and up-scale horizontally, and the other way round
           (150, 12),                    # a vertical shrink above 4: the tile's rows are held as four slots per output row
           (5, 7)]                       # a second frame of an earlier size: it shares both sets


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import _lib, kernels
    _lib.load()
    return kernels


def image(h, w, seed):
    return np.random.RandomState(7919 * seed + 31 * h + w).randint(0, 256, (h, w, 3)).astype(np.uint8)


_WANT = {}


def want(frame, dst):
    """the recipe's resize of one frame, computed once per (bytes, destination) and left unchanged"""
    key = (frame.shape, frame.tobytes(), dst)
    if key not in _WANT:
        r = R.resize(frame[None], *dst)[0]
        r.setflags(write=False)
        _WANT[key] = r
    return _WANT[key]


def pack(frames, slots, swaps, dst, F, fill=0x00):
    """(src uint8 numpy of the staged bytes, table CPU tensor, src_bytes, nh, nv): the frames back to back at plan_ingest's offsets, every
    byte that belongs to no frame (the slack in front, the gaps up to the next multiple of 4, the slack behind) set to ``fill``"""
    from simple_tad_amd import stream_bank as SB
    table, offsets, nbytes, nh, nv = SB.plan_ingest([f.shape[:2] for f in frames], slots, swaps, *dst, F)
    src = np.full(nbytes + SB._HEAD, fill, dtype=np.uint8)
    for f, at in zip(frames, offsets):
        src[at:at + f.size] = f.reshape(-1)
    return src, table, nbytes, nh, nv


def ingest(K, frames, slots, swaps, dst, F, fill=0x00):
    src, table, nbytes, nh, nv = pack(frames, slots, swaps, dst, F, fill)
    store = torch.full((F, *dst, 3), POISON, dtype=torch.uint8, device="cuda")
    out = K.ingest_frames(torch.from_numpy(src).cuda(), nbytes, store, table.cuda(), len(frames), nh, nv)
    assert out is store
    return store.cpu().numpy()


def expected(frames, slots, swaps, dst, F):
    e = np.full((F, *dst, 3), POISON, dtype=np.uint8)
    for f, s, sw in zip(frames, slots, swaps):
        e[s] = want(f, dst)[..., ::-1] if sw else want(f, dst)
    return e


@pytest.mark.parametrize("dst", DESTS, ids=[f"{a}x{b}" for a, b in DESTS])
def test_one_mixed_call_equals_the_recipe_and_resize_frames(K, dst):
    from simple_tad_amd.frame_resize import resize_frames
    frames = [image(h, w, i) for i, (h, w) in enumerate(SOURCES)] + [image(*dst, 99)]       # the last one is at S_h x S_w already
    n = len(frames)
    F = n + 3
    slots = [(7 * i + 2) % F for i in range(n)]                                             # scattered, out of order (7 and F = 15 coprime)
    assert len(set(slots)) == n and slots != sorted(slots) and F % 7
    swaps = [bool(i % 3 == 1) for i in range(n)]                                            # the channel swap on and off in one call
    swaps[-1] = False
    got = ingest(K, frames, slots, swaps, dst, F)
    exp = expected(frames, slots, swaps, dst, F)
    for k, s in enumerate(slots):
        assert np.array_equal(got[s], exp[s]), f"frame {k} {frames[k].shape[:2]} -> {dst}, slot {s}, swap {swaps[k]}"
    untouched = sorted(set(range(F)) - set(slots))
    assert len(untouched) == 3 and (got[untouched] == POISON).all()
    assert np.array_equal(got[slots[-1]], frames[-1]), "equal extents give the input bytes back"
    assert np.array_equal(got[slots[3]][..., ::-1] if swaps[3] else got[slots[3]], want(frames[3], dst))
    assert not np.array_equal(got[slots[3]], got[slots[10]][..., ::-1] if swaps[10] else got[slots[10]]), "equal sizes, their own bytes"
    # on the device: the one-size kernel, once per frame
    for k, f in enumerate(frames):
        one = resize_frames(torch.from_numpy(f[None]).cuda(), dst)[0]
        if swaps[k]:
            one = one.flip(-1)
        assert torch.equal(one.cpu(), torch.from_numpy(got[slots[k]])), k
    # two calls give the same bits
    assert np.array_equal(ingest(K, frames, slots, swaps, dst, F), got)


def test_one_frame_and_the_largest_count(K):
    from simple_tad_amd import _lib
    dst = (4, 4)
    f = image(3, 5, 0)
    got = ingest(K, [f], [1], [True], dst, 2)
    assert np.array_equal(got[1], want(f, dst)[..., ::-1]) and (got[0] == POISON).all()
    n = _lib.BANK_MAX_FRAMES
    sizes = [(1, 1), (2, 3), (3, 2), (4, 4)]
    rng = np.random.RandomState(5)
    frames = [rng.randint(0, 256, (*sizes[i % 4], 3)).astype(np.uint8) for i in range(n)]
    F = n + 2
    slots = [(1237 * i + 11) % F for i in range(n)]                                         # 1237 is prime and does not divide F = 4098
    assert len(set(slots)) == n
    swaps = [bool(i % 5 == 0) for i in range(n)]
    got = ingest(K, frames, slots, swaps, dst, F)
    exp = np.full((F, *dst, 3), POISON, dtype=np.uint8)
    for j, sz in enumerate(sizes):                                                          # the recipe, one batch per size
        ks = list(range(j, n, 4))
        r = R.resize(np.stack([frames[k] for k in ks]), *dst)
        for k, rk in zip(ks, r):
            exp[slots[k]] = rk[..., ::-1] if swaps[k] else rk
    assert np.array_equal(got, exp)
    with pytest.raises(_lib.TadError, match="1 .. 4096"):
        ingest(K, frames + [frames[0]], slots + [F - 1], swaps + [False], dst, F)


def test_bytes_of_the_neighbours_and_of_the_gaps_do_not_matter(K):
    """frames back to back, widths whose rows end at every phase of a word: the odd frames must come out the same whatever the even
    frames, the gaps between frames and the slack around them hold"""
    dst = (16, 16)
    shapes = [(3, 3), (5, 7), (2, 1), (9, 1), (1, 9), (4, 6), (3, 5), (20, 23), (1, 1), (6, 3)]
    a = [image(h, w, 10 + i) for i, (h, w) in enumerate(shapes)]
    b = [f if i % 2 else np.full_like(f, 0xFF) for i, f in enumerate(a)]
    c = [f if i % 2 else np.zeros_like(f) for i, f in enumerate(a)]
    slots = list(range(len(shapes)))[::-1]
    swaps = [False] * len(shapes)
    ga = ingest(K, a, slots, swaps, dst, len(shapes), fill=0x00)
    gb = ingest(K, b, slots, swaps, dst, len(shapes), fill=0xFF)
    gc = ingest(K, c, slots, swaps, dst, len(shapes), fill=0x5A)
    for i in range(1, len(shapes), 2):
        assert np.array_equal(ga[slots[i]], want(a[i], dst)), i
        assert np.array_equal(gb[slots[i]], ga[slots[i]]) and np.array_equal(gc[slots[i]], ga[slots[i]]), i
    for i in range(0, len(shapes), 2):
        assert (gb[slots[i]] == 0xFF).all() and (gc[slots[i]] == 0).all(), "a frame of 0 or of 255 stays what it is"


@pytest.fixture(scope="module")
def arena():
    return GuardedArena(8 << 20, "cuda")


def _guarded_operands(arena, src, table, F, dst, store_offset):
    zeros = torch.zeros(8, dtype=torch.int32)
    x = arena.place(torch.from_numpy(src), name="src")
    t = arena.place(table, guard_pattern=(zeros, zeros), name="table")
    store = arena.place((F, *dst, 3), torch.uint8, role="output", name="store", fill=POISON, offset=store_offset)
    return x, t, store


@pytest.mark.parametrize("store_offset", [0, 1, 2, 3])
def test_guard_bands(K, arena, store_offset):
    """src, table and store each between two poisoned bands of one allocation (0xFF around the bytes, zero rows around the table), the
    store at every phase of a word: nothing outside the store changes, inside it only the named slots do, and the results are the recipe's
    -- they depend on no byte outside the frames.  The last frame ends on the last byte of src's body with a width that leaves its rows
    unaligned, so the words that hold its last pixels reach into the guard."""
    dst = (16, 16)
    frames = [image(h, w, 40 + i) for i, (h, w) in enumerate([(5, 7), (20, 23), (1, 9), (150, 12), (9, 5)])]
    F = len(frames) + 2
    slots = [4, 0, 6, 2, 5]
    swaps = [False, True, False, False, True]
    src, table, nbytes, nh, nv = pack(frames, slots, swaps, dst, F, fill=0xFF)
    end = nbytes - (-frames[-1].size) % 4                                                   # the last frame's last byte + 1
    assert end % 4 == 3 and (src[end:] == 0xFF).all()
    arena.reset()
    x, t, store = _guarded_operands(arena, src[:end], table, F, dst, store_offset)
    assert store.data_ptr() % 4 == store_offset
    at = x.data_ptr() - arena.buf.data_ptr()
    slack = arena.buf[at:at + end + 1]                                                      # the allocation's slack up to a multiple of 4: one guard byte
    assert slack.data_ptr() == x.data_ptr() and int(slack[-1]) == 0xFF
    K.ingest_frames(slack, end, store, t, len(frames), nh, nv)                              # src_bytes = the body: the last frame still fits
    arena.verify()
    assert np.array_equal(store.cpu().numpy(), expected(frames, slots, swaps, dst, F))


def test_a_malformed_device_table_is_never_an_address(K, arena):
    """The header's stated defence, through the raw C entry (the Python wrapper's table has passed the plan check, which refuses every
    row below): a row whose frame does not fit in src, or whose extents are below 1, is ignored; a slot is clamped into the store; a set
    index is clamped into the sets (the taps are clamped to the row's own extents whatever the set says).  Everything lies inside one
    guarded allocation; the well-formed rows give the recipe's bytes all the same."""
    from simple_tad_amd import _lib
    dst = (16, 16)
    frames = [image(h, w, 60 + i) for i, (h, w) in enumerate([(5, 7), (20, 23), (9, 5), (4, 6), (7, 50), (3, 3), (6, 3)])]
    F = len(frames) + 3                                                                     # slots 7, 8, 9 are named by no row
    slots = [3, 0, 6, 2, 5, 1, 4]
    swaps = [False] * len(frames)
    src, table, nbytes, nh, nv = pack(frames, slots, swaps, dst, F, fill=0xFF)
    lib = _lib.load_bank()
    tab = table.numpy().copy()
    rows = tab[:len(frames) * _lib.BANK_ROW_WORDS].reshape(len(frames), _lib.BANK_ROW_WORDS)
    rows[1, 0] = nbytes - 8                       # a 20 x 23 frame 8 bytes in front of the end of src: ignored
    rows[2, 3] = F + 5                            # a slot past the store: clamped to F - 1
    rows[3, 4], rows[3, 5] = 99, -7               # set indices out of range: clamped to the last horizontal, the first vertical set
    rows[5, 1] = 0                                # an extent below 1: ignored
    rows[6, 0] = -4                               # a negative offset: ignored
    assert lib.tadb_ingest_plan_check(tab.ctypes.data, tab.size, len(frames), nh, nv, nbytes, F, *dst) == -1
    arena.reset()
    x, t, store = _guarded_operands(arena, src, torch.from_numpy(tab), F, dst, 0)
    rc = lib.tadb_ingest_frames(x.data_ptr(), nbytes, store.data_ptr(), F, t.data_ptr(), t.numel(), len(frames), nh, nv, *dst,
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.tadb_last_error_string()
    arena.verify()                                                                          # nothing outside the store has changed
    got = store.cpu().numpy()
    for k in (0, 4):                                                                        # the other rows' results are unchanged
        assert np.array_equal(got[slots[k]], want(frames[k], dst)), k
    assert np.array_equal(got[F - 1], want(frames[2], dst)), "the clamped slot"
    for s in (slots[1], slots[2], slots[5], slots[6], 7, 8):                                # ignored rows, the slot row 2 named no longer, spare slots
        assert (got[s] == POISON).all(), s
    assert (got[slots[3]] != POISON).any()                                                  # row 3 wrote its own slot, with other sets' coefficients
