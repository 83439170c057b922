"""ClipPrefetcher on the CPU device (the same rotation with plain copies, no pinning) and the host side of tad_im2col_tubelets_16.
Every wait below has a timeout: a deadlock fails instead of hanging."""
import ctypes
import os
import re
import threading

import pytest
import torch

from simple_tad_amd import ClipPrefetcher, ops, prefetch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAIT_S = 10.0
CPU = torch.device("cpu")


def make_batch(i, b=2):
    """the engines' batch shape: (clip, target, name list, extra_info dict), every tensor holding the batch index"""
    return (torch.full((b, 3, 2, 4, 4), float(i)), torch.full((b,), i, dtype=torch.int64), [f"clip{i}_{j}" for j in range(b)],
            {"ttc": torch.full((b,), i + 0.5), "smoothed_labels": torch.full((b, 2), float(-i)), "fps": 30, "tag": ("v", i)})


def check_batch(out, i, b=2):
    ref = make_batch(i, b)
    assert type(out) is tuple and len(out) == 4
    assert torch.equal(out[0], ref[0]) and out[0].dtype == torch.float32
    assert torch.equal(out[1], ref[1]) and out[1].dtype == torch.int64
    assert type(out[2]) is list and out[2] == ref[2]
    assert type(out[3]) is dict and list(out[3]) == list(ref[3])
    assert torch.equal(out[3]["ttc"], ref[3]["ttc"]) and torch.equal(out[3]["smoothed_labels"], ref[3]["smoothed_labels"])
    assert out[3]["fps"] == 30 and out[3]["tag"] == ("v", i)


def live_producers():
    return [t for t in threading.enumerate() if t.name == "ClipPrefetcher" and t.is_alive()]


class ListLoader:
    """a loader with the attributes the engines and their callers read"""

    def __init__(self, batches):
        self.batches, self.sampler, self.dataset = batches, object(), object()

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_order_and_structure(depth):
    n = 3 * depth + 1
    pf = ClipPrefetcher(ListLoader([make_batch(i) for i in range(n)]), CPU, depth=depth)
    got = list(pf)
    assert len(got) == n
    for i, out in enumerate(got):
        check_batch(out, i)
    assert live_producers() == []


def test_len_and_sampler_delegate():
    loader = ListLoader([make_batch(i) for i in range(5)])
    pf = ClipPrefetcher(loader, CPU)
    assert len(pf) == 5 and pf.sampler is loader.sampler and pf.dataset is loader.dataset
    with pytest.raises(AttributeError):
        pf.batch_sampler  # the loader has none: the wrapper invents nothing
    with pytest.raises(ValueError):
        ClipPrefetcher(loader, CPU, depth=0)
    with pytest.raises(ValueError):
        ClipPrefetcher(loader, CPU, wire="bf16")


class CountingLoader:
    """counts what the producer has taken, and lets the consumer wait for a count"""

    def __init__(self, n):
        self.n, self.taken, self.cv = n, 0, threading.Condition()
        self.requested = 0      # next() calls the consumer has STARTED (written by the consumer before each call)
        self.max_ahead = 0      # max over takes of (taken - requested): at most depth if the producer respects the bound

    def __len__(self):
        return self.n

    def __iter__(self):
        for i in range(self.n):
            with self.cv:
                self.taken += 1
                self.max_ahead = max(self.max_ahead, self.taken - self.requested)
                self.cv.notify_all()
            yield make_batch(i)

    def wait_taken(self, count):
        with self.cv:
            return self.cv.wait_for(lambda: self.taken >= count, timeout=WAIT_S)


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_producer_is_never_more_than_depth_ahead(depth):
    n = 3 * depth + 4
    loader = CountingLoader(n)
    it = iter(ClipPrefetcher(loader, CPU, depth=depth))
    received = 0
    # before the first request the producer may take `depth` batches, and does (that is the prefetch)
    assert loader.wait_taken(min(n, depth)) and loader.taken == min(n, depth)
    for i in range(n):
        loader.requested += 1
        check_batch(next(it), i)
        received += 1
        assert loader.taken <= received + depth
        # ... it runs ahead as far as it may (otherwise nothing overlaps) and then stands still
        assert loader.wait_taken(min(n, received + depth)), (loader.taken, received)
        assert loader.taken == min(n, received + depth)
    with pytest.raises(StopIteration):
        next(it)
    # at the moment of a take the consumer had started `requested` calls, `requested - 1` of them answered at the least
    assert loader.max_ahead <= depth
    assert live_producers() == []


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_no_aliasing_after_slot_reuse(depth):
    """every yielded batch is intact after depth + 2 further batches: nothing yielded is a view of a staging slot"""
    n = 3 * depth + 3
    held = []
    for out in ClipPrefetcher(ListLoader([make_batch(i) for i in range(n)]), CPU, depth=depth):
        held.append(out)
        if len(held) > depth + 2:
            check_batch(held[-(depth + 3)], len(held) - (depth + 3))
    for i, out in enumerate(held):
        check_batch(out, i)
    ptrs = [o[0].data_ptr() for o in held]
    assert len(set(ptrs)) == len(ptrs)


def test_ragged_batches_shrink_and_regrow():
    sizes = [2, 2, 5, 2, 5, 1]  # larger than the first (slot regrowth), then smaller (a view of the slot), last one short
    pf = ClipPrefetcher(ListLoader([make_batch(i, b) for i, b in enumerate(sizes)]), CPU, depth=2)
    got = list(pf)
    for i, (out, b) in enumerate(zip(got, sizes)):
        check_batch(out, i, b)
        assert out[0].is_contiguous() and out[0].shape[0] == b
    assert len(got) == len(sizes)


class Boom(RuntimeError):
    pass


@pytest.mark.parametrize("k", [0, 1, 4])
def test_loader_failure_arrives_at_its_position(k):
    def gen():
        for i in range(8):
            if i == k:
                raise Boom(f"batch {i}")
            yield make_batch(i)

    class L:
        def __iter__(self):
            return gen()

    it = iter(ClipPrefetcher(L(), CPU, depth=2))
    for i in range(k):
        check_batch(next(it), i)
    with pytest.raises(Boom, match=f"batch {k}"):
        next(it)
    with pytest.raises(StopIteration):
        next(it)
    assert live_producers() == []


def test_staging_failure_arrives_at_its_position():
    # a leaf whose copy into a dense slot fails: a sparse tensor
    batches = [make_batch(0), make_batch(1), (torch.zeros(2, 2), torch.zeros(2, 2).to_sparse())]
    it = iter(ClipPrefetcher(ListLoader(batches), CPU, depth=3))
    check_batch(next(it), 0)
    check_batch(next(it), 1)
    with pytest.raises(Exception):
        next(it)
    assert live_producers() == []


def test_early_break_new_epoch_and_close():
    loader = ListLoader([make_batch(i) for i in range(9)])
    pf = ClipPrefetcher(loader, CPU, depth=2)
    for i, out in enumerate(pf):
        check_batch(out, i)
        if i == 2:
            break
    first = iter(pf)  # a second __iter__ stops the first epoch's producer and starts over from batch 0
    check_batch(next(first), 0)
    assert len(live_producers()) == 1
    second = iter(pf)
    assert len(live_producers()) == 1
    with pytest.raises(StopIteration):
        next(first)
    for i in range(9):
        check_batch(next(second), i)
    third = iter(pf)
    check_batch(next(third), 0)
    pf.close()
    assert live_producers() == []
    with pytest.raises(StopIteration):
        next(third)
    pf.close()  # idempotent


def test_dropping_the_iterator_stops_the_producer():
    pf = ClipPrefetcher(ListLoader([make_batch(i) for i in range(9)]), CPU, depth=2)
    it = iter(pf)
    check_batch(next(it), 0)
    th = pf._epoch.thread
    del it  # what an early ``break`` leaves behind: nobody holds the iterator
    th.join(WAIT_S)
    assert not th.is_alive()
    pf2 = ClipPrefetcher(ListLoader([make_batch(i) for i in range(9)]), CPU, depth=2)
    it2 = iter(pf2)
    check_batch(next(it2), 0)
    th2 = pf2._epoch.thread
    assert th2.daemon
    del pf2, it2  # garbage collection of the wrapper
    th2.join(WAIT_S)
    assert not th2.is_alive()


@pytest.fixture
def precision():
    prev = ops.get_precision()
    yield ops.set_precision
    ops.set_precision(prev)


@pytest.mark.parametrize("mode,dtype", [("fast", torch.bfloat16), ("half", torch.float16)])
def test_wire_operand_rounds_the_clip_in_the_staging_pass(precision, mode, dtype):
    precision(mode)
    g = torch.Generator().manual_seed(5)
    batches = []
    for i in range(5):
        clip = torch.randn(2, 3, 2, 4, 4, generator=g) * (10.0 ** (i - 2))
        batches.append((clip, torch.full((2,), i, dtype=torch.int64), [f"n{i}"], {"ttc": torch.randn(2, generator=g), "aux": torch.randn(2, 3, 2, 4, 4)}))
    got = list(ClipPrefetcher(ListLoader(batches), CPU, depth=2, wire="operand"))
    for out, ref in zip(got, batches):
        assert out[0].dtype == dtype and torch.equal(out[0].view(torch.int16), ref[0].to(dtype).view(torch.int16))
        assert out[1].dtype == torch.int64 and torch.equal(out[1], ref[1]) and out[2] == ref[2]
        assert out[3]["ttc"].dtype == torch.float32 and torch.equal(out[3]["ttc"], ref[3]["ttc"])
        assert out[3]["aux"].dtype == torch.float32 and torch.equal(out[3]["aux"], ref[3]["aux"])  # 5-D f32, but not the clip
    # a clip that is not 5-D f32 (the uint8 input stage's frames) keeps its dtype; clip_index picks the leaf
    u8 = [(torch.full((2, 2, 4, 4, 3), i, dtype=torch.uint8), torch.randn(2, 3, 2, 4, 4)) for i in range(3)]
    for out, ref in zip(ClipPrefetcher(ListLoader(u8), CPU, wire="operand"), u8):
        assert out[0].dtype == torch.uint8 and torch.equal(out[0], ref[0]) and out[1].dtype == torch.float32
    for out, ref in zip(ClipPrefetcher(ListLoader(u8), CPU, wire="operand", clip_index=1), u8):
        assert out[0].dtype == torch.uint8 and out[1].dtype == dtype and torch.equal(out[1].view(torch.int16), ref[1].to(dtype).view(torch.int16))


def test_wire_operand_raises_under_precise(precision):
    precision("precise")
    pf = ClipPrefetcher(ListLoader([make_batch(0)]), CPU, wire="operand")
    with pytest.raises(ValueError, match="precise"):
        iter(pf)
    assert live_producers() == []
    check_batch(next(iter(ClipPrefetcher(ListLoader([make_batch(0)]), CPU, wire="same"))), 0)


def test_no_pool_and_nothing_sized_by_the_cpu_count():
    src = open(prefetch.__file__).read()
    assert "cpu_count" not in src and "ThreadPool" not in src and "concurrent.futures" not in src


# ---------------------------------------------------------------------------------------------------- C ABI of the 16-bit clip source
@pytest.fixture(scope="module")
def lib():
    from simple_tad_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_im2col_16_is_declared_bound_and_exported(lib):
    from simple_tad_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tad_mi355x.h")).read(), flags=re.S)
    m = re.search(r"int\s+tad_im2col_tubelets_16\s*\(([^)]*)\)", header)
    assert m, "tad_im2col_tubelets_16 is not declared in include/tad_mi355x.h"
    assert re.sub(r"\s+", " ", m.group(1)).strip() == ("const uint16_t* x, uint16_t* cols, int B, int C, int T, int H, int W, int tubelet, "
                                                       "int patch, tad_stream_t stream")
    assert _lib.SIGNATURES["tad_im2col_tubelets_16"] == _lib.SIGNATURES["tad_im2col_tubelets"]
    assert hasattr(lib, "tad_im2col_tubelets_16")
    assert "tad_im2col_tubelets_16" not in _lib.F16_TWINS and not hasattr(lib, "tad_im2col_tubelets_16_f16")  # a move: one symbol
    assert len(_lib.F16_TWINS) == 23 and _lib.ABI_VERSION == 5


def test_im2col_16_host_validation(lib):
    """argument checks run before any launch: -1 and a message, on a machine without a GPU"""
    buf = ctypes.create_string_buffer(256)
    base = ctypes.addressof(buf)
    p = (base + 15) // 16 * 16  # 16-byte aligned inside the buffer
    f = lib.tad_im2col_tubelets_16
    assert f(None, p, 1, 3, 2, 8, 8, 2, 8, None) == -1 and b"null" in lib.tad_last_error_string()
    assert f(p, None, 1, 3, 2, 8, 8, 2, 8, None) == -1 and b"null" in lib.tad_last_error_string()
    assert f(p, p, 1, 3, 2, 9, 9, 2, 3, None) == -1 and b"even" in lib.tad_last_error_string()            # odd patch
    assert f(p, p, 1, 3, 3, 8, 8, 2, 8, None) == -1 and b"multiples" in lib.tad_last_error_string()       # T % tubelet
    assert f(p, p, 1, 3, 2, 8, 12, 2, 8, None) == -1 and b"multiples" in lib.tad_last_error_string()      # W % patch
    assert f(p + 8, p, 1, 3, 2, 8, 8, 2, 8, None) == -1 and b"misaligned" in lib.tad_last_error_string()  # wide: x 16 bytes
    assert f(p, p + 4, 1, 3, 2, 8, 8, 2, 8, None) == -1 and b"misaligned" in lib.tad_last_error_string()  # wide: cols 16 bytes
    assert f(p + 2, p, 1, 3, 2, 6, 6, 2, 6, None) == -1 and b"misaligned" in lib.tad_last_error_string()  # pairs: x 4 bytes
    assert f(p, p + 2, 1, 3, 2, 6, 6, 2, 6, None) == -1 and b"misaligned" in lib.tad_last_error_string()  # pairs: cols 4 bytes
