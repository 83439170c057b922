"""StreamBank's host side without a GPU: the ring bookkeeping (stream_bank.StreamRings) against a plain-Python model of S deques, the
table builder (stream_bank.plan_ingest: offsets, set de-duplication, flags, the cache) and the refusals that are made before anything
could be launched."""
import collections
import random

import numpy as np
import pytest
import torch

import simple_tad_amd as T
from simple_tad_amd import _lib, stream_bank as SB
from simple_tad_amd._lib import TadError
from simple_tad_amd.frame_resize import cubic_coeffs


class DequeModel:
    """what the bank must behave like: per stream the last T frame tags in arrival order, and where each tag lives in the store"""

    def __init__(self, S, T_):
        self.S, self.T = S, T_
        self.win = [collections.deque(maxlen=T_) for _ in range(S)]
        self.store = {}  # slot -> tag

    def push(self, s, tag, slot):
        assert s * self.T <= slot < (s + 1) * self.T, "a stream writes inside its own slots"
        if len(self.win[s]) == self.T:  # the slot taken must be the one of the frame that leaves
            assert self.store[slot] == self.win[s][0], "a full ring overwrites its OLDEST frame"
        else:
            assert self.store.get(slot) not in self.win[s], "a filling ring overwrites nothing it holds"
        self.win[s].append(tag)
        self.store[slot] = tag

    def reset(self, s):
        self.win[s].clear()


@pytest.mark.parametrize("S,T_", [(1, 1), (3, 4), (5, 2), (4, 16)])
def test_rings_follow_a_model_of_deques(S, T_):
    rng = random.Random(100 * S + T_)
    rings, model = SB.StreamRings(S, T_), DequeModel(S, T_)
    tag, differed = 0, False
    for step in range(40 * T_):
        if rng.random() < 0.05:
            s = rng.randrange(S)
            rings.reset(s)
            model.reset(s)
            assert rings.count[s] == 0 and rings.start[s] == 0
        # an uneven tick: some cameras drop the frame, the order of the ids is arbitrary
        ids = [s for s in range(S) if rng.random() < 0.6]
        rng.shuffle(ids)
        slots = rings.assign(rings.check_ids(ids, "test"))
        assert len(set(slots)) == len(slots) == len(ids)
        for s, slot in zip(ids, slots):
            model.push(s, (s, tag), slot)
            tag += 1
        assert rings.ready == [s for s in range(S) if len(model.win[s]) == T_]
        ready = rings.ready
        differed |= len({rings.start[s] for s in ready}) > 1
        table = rings.window_table(ready)
        assert table.dtype == np.int32 and table.shape == (len(ready), T_)
        for row, s in zip(table, ready):  # temporal order, oldest first
            assert [model.store[int(slot)] for slot in row] == list(model.win[s]), (step, s)
    assert any(c > 2 * T_ for c in rings.count), "some ring has wrapped more than once"
    assert differed or S == 1 or T_ == 1, "ready rings sat at different phases in one table"


def test_ids_are_checked():
    rings = SB.StreamRings(3, 2)
    assert rings.check_ids(np.asarray([2, 0]), "x") == [2, 0] and rings.check_ids(torch.tensor([1]), "x") == [1] and rings.check_ids([], "x") == []
    with pytest.raises(TadError, match=r"who: stream id 3 outside \[0, 3\)"):
        rings.check_ids([0, 3], "who")
    with pytest.raises(TadError, match=r"stream id -1 outside"):
        rings.check_ids([-1], "who")
    with pytest.raises(TadError, match="stream id 1 is named twice in one call"):
        rings.check_ids([1, 2, 1], "who")
    with pytest.raises(TadError):
        SB.StreamRings(0, 4)
    with pytest.raises(TadError):
        SB.StreamRings(2, 0)


def _sets(table, K, nh, nv, S_h, S_w):
    R, H = _lib.BANK_ROW_WORDS, _lib.FR_SET_HEAD
    rows = table[:K * R].reshape(K, R)
    at, out = K * R, []
    for n, size in ((nh, S_w), (nv, S_h)):
        group = []
        for _ in range(n):
            group.append((table[at:at + H].tolist(), table[at + H:at + H + size], table[at + H + size:at + H + 5 * size].reshape(size, 4)))
            at += H + 5 * size
        out.append(group)
    assert at == table.size
    return rows, out[0], out[1]


def test_table_builder_offsets_sets_and_flags():
    extents = [(5, 7), (20, 23), (5, 7), (16, 12), (1, 1), (20, 7)]
    slots = [9, 0, 4, 11, 2, 7]
    swaps = [False, True, True, False, False, True]
    S_h, S_w = 16, 12
    table, offsets, nbytes, nh, nv = SB.plan_ingest(extents, slots, swaps, S_h, S_w, 12)
    table = table.numpy()
    assert (nh, nv) == (4, 4), "one horizontal set per distinct w (7, 23, 12, 1), one vertical per distinct h (5, 20, 16, 1)"
    rows, hsets, vsets = _sets(table, len(extents), nh, nv, S_h, S_w)
    # offsets: back to back, each on a multiple of 4, slack in front of the first, the end rounded up
    at = SB._HEAD
    for k, (h, w) in enumerate(extents):
        assert offsets[k] == at == rows[k, 0] and at % 4 == 0
        at += (h * w * 3 + 3) // 4 * 4
    assert nbytes == at and SB._HEAD % 4 == 0 and SB._HEAD >= 4
    assert rows[:, 1].tolist() == [h for h, _ in extents] and rows[:, 2].tolist() == [w for _, w in extents]
    assert rows[:, 3].tolist() == slots
    assert rows[:, 6].tolist() == [_lib.BANK_SWAP_RB if s else 0 for s in swaps] and not rows[:, 7].any()
    # frames of one width share their horizontal set, frames of one height their vertical set; each set is cubic_coeffs' own
    assert rows[0, 4] == rows[2, 4] == rows[5, 4] and rows[1, 5] == rows[5, 5] and rows[0, 5] == rows[2, 5]
    for k, (h, w) in enumerate(extents):
        head, first, kk = hsets[rows[k, 4]]
        assert head == [w, S_w, 0, 0]
        assert np.array_equal(first, cubic_coeffs(w, S_w)[0]) and np.array_equal(kk, cubic_coeffs(w, S_w)[1])
        head, first, kk = vsets[rows[k, 5]]
        assert head == [h, S_h, 0, 0]
        assert np.array_equal(first, cubic_coeffs(h, S_h)[0]) and np.array_equal(kk, cubic_coeffs(h, S_h)[1])
    # equal extents: the identity coefficients
    assert all(k.tolist() == [0, 2048, 0, 0] for k in hsets[rows[3, 4]][2]) and all(k.tolist() == [0, 2048, 0, 0] for k in vsets[rows[3, 5]][2])


def test_table_cache_changes_the_slots_only_and_checks_them_again():
    extents, swaps = [(5, 7), (9, 7), (5, 3)], [True, False, False]
    cache = {}
    a = SB.plan_ingest(extents, [0, 5, 3], swaps, 8, 8, 6, cache)
    b = SB.plan_ingest(extents, [1, 4, 3], swaps, 8, 8, 6, cache)
    fresh = SB.plan_ingest(extents, [1, 4, 3], swaps, 8, 8, 6)
    assert len(cache) == 1 and torch.equal(b[0], fresh[0]) and b[1:] == fresh[1:]
    assert (a[0] != b[0]).nonzero().flatten().tolist() == [3, _lib.BANK_ROW_WORDS + 3]
    assert a[0][3] == 0 and a[0][_lib.BANK_ROW_WORDS + 3] == 5, "the cached table is not the one handed out"
    with pytest.raises(TadError, match="row 1: slot=6 outside the store"):
        SB.plan_ingest(extents, [1, 6, 3], swaps, 8, 8, 6, cache)
    with pytest.raises(TadError, match="slot=3 is already named by row 0"):
        SB.plan_ingest(extents, [3, 4, 3], swaps, 8, 8, 6, cache)
    SB.plan_ingest(extents, [1, 4, 3], [False] * 3, 8, 8, 6, cache)
    assert len(cache) == 2, "other flags are another table"


def test_table_builder_refusals():
    with pytest.raises(TadError, match="at most 64 each"):
        SB.plan_ingest([(2, w) for w in range(1, 66)], list(range(65)), [False] * 65, 4, 4, 65)
    with pytest.raises(TadError, match=r"cubic_coeffs: 0 -> 4 samples"):  # (the coefficient builder meets the extent first)
        SB.plan_ingest([(0, 3)], [0], [False], 4, 4, 1)
    with pytest.raises(TadError, match="1 .. 4096"):
        SB.plan_ingest([], [], [], 4, 4, 1)
    with pytest.raises(TadError, match="slot=2 outside the store"):
        SB.plan_ingest([(3, 3)], [2], [False], 4, 4, 2)


def test_a_model_that_is_not_on_the_gpu_is_refused():
    model = T.VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=1, num_heads=2, all_frames=4, tubelet_size=2, num_classes=2)
    with pytest.raises(TadError, match="the model must be on a GPU"):
        T.StreamBank(model, streams=2)
    assert T.StreamBank is SB.StreamBank and T.stream_bank is SB
    from simple_tad_amd import kernels
    assert callable(kernels.ingest_frames) and callable(kernels.ingest_table)
    with pytest.raises(TadError, match="expected a GPU tensor"):
        kernels.ingest_frames(torch.zeros(64, dtype=torch.uint8), 64, torch.zeros((1, 4, 4, 3), dtype=torch.uint8), torch.zeros(8, dtype=torch.int32), 1, 1, 1)
