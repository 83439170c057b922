"""The guard-band arena (tests/guarded.py) proves that it can see: plain torch ops on a CPU arena stand in for a kernel, each planted
defect must make verify() or the value comparison fail, and the same stand-in without the defect must pass.  This is the evidence
that tests/test_guarded_gpu.py is not vacuous; no kernel is mutated for it."""
import types

import pytest
import torch

from guarded import GuardedArena, GuardViolation, POISON_MODES, bits, poison_bits, same_bits

ROWS, COLS = 37, 20  # nothing a multiple of anything
STRAY = -1.2345678  # 0xBF9E0652: every byte differs from both poisons'


@pytest.fixture(params=POISON_MODES)
def arena(request):
    return GuardedArena(8 << 20, "cpu", poison=request.param)


def raw(arena, t, dtype=None):
    """what a kernel holds: the whole arena as elements of t's type, and the element index of t[0] in it (a 'base pointer')"""
    p = arena.placement_of(t)
    dtype = dtype or t.dtype
    item = torch.empty((), dtype=dtype).element_size()
    head = p.start % item
    return arena.buf[head:head + (arena.buf.numel() - head) // item * item].view(dtype), (p.start - head) // item


def scale_kernel(arena, x, y, *, defect=None):
    """y = 2 x, written through a raw base pointer the way a kernel does; ``defect`` plants one addressing bug"""
    mem, y0 = raw(arena, y)
    n = x.numel()
    vals = (x.reshape(-1) * 2).to(y.dtype)
    if defect == "unwritten":
        mem[y0:y0 + n - 1] = vals[:n - 1]
        return
    mem[y0:y0 + n] = vals
    if defect == "past":
        mem[y0 + n] = STRAY
    elif defect == "before":
        mem[y0 - 1] = STRAY
    elif defect == "tile_past":  # a ragged last tile stored without its row guard: row ROWS + 255 of a 256-row tile
        mem[y0 + (ROWS + 255) * COLS:y0 + (ROWS + 256) * COLS] = STRAY
    elif defect == "input":
        xm, x0 = raw(arena, x)
        xm[x0 + 5] = STRAY


def setup(arena, dtype=torch.float32):
    torch.manual_seed(0)
    x = torch.randn(ROWS, COLS).to(dtype)
    xa = arena.place(x, role="input", name="x")
    ya = arena.place((ROWS, COLS), dtype, role="output", name="y")
    za = arena.place(torch.randn(3, 5), role="input", name="neighbour")
    return x, xa, ya, za


def test_layout_alignment_guard_width_and_poison(arena):
    x, xa, ya, za = setup(arena, torch.bfloat16)
    for t in (xa, ya, za):
        p = arena.placement_of(t)
        assert t.data_ptr() % 256 == 0
        assert p.start - p.lo >= max(64 << 10, 256 * t.shape[-1] * t.element_size()) and p.hi - p.end >= p.start - p.lo
        assert p.end - p.start == t.numel() * t.element_size()  # the guard starts at the byte after the last element
    view, pat = poison_bits(torch.bfloat16, arena.poison)
    mem, y0 = raw(arena, ya)
    assert pat == {"nan": 0x7FC0, "huge": 0x7F7F}[arena.poison]
    assert int(bits(mem[y0 - 1:y0])) == pat and int(bits(mem[y0 + ya.numel():y0 + ya.numel() + 1])) == pat
    assert torch.isnan(ya).all(), "an output body starts as NaN"
    assert same_bits(xa, x)
    wide = arena.place((5, 2048), torch.float32, role="output")
    p = arena.placement_of(wide)
    assert p.start - p.lo >= 256 * 2048 * 4, "256 rows of the row pitch"
    idx = arena.place(torch.tensor([3, 1, 2], dtype=torch.int32), index_range=7, name="idx")
    im, i0 = raw(arena, idx)
    g = torch.cat([im[i0 - 4096:i0], im[i0 + 3:i0 + 4096]])
    assert int(g.min()) >= 0 and int(g.max()) < 7 and g.unique().numel() > 1, "guards of an index tensor hold in-range indices"
    with pytest.raises(ValueError):
        arena.place(torch.tensor([1], dtype=torch.int32))
    u8 = arena.place(torch.zeros(11, dtype=torch.uint8), name="frames")
    um, u0 = raw(arena, u8)
    assert int(um[u0 - 1]) == 0xFF and int(um[u0 + 11]) == 0xFF


def test_correct_stand_in_passes(arena):
    x, xa, ya, _ = setup(arena)
    scale_kernel(arena, xa, ya)
    arena.verify()
    assert torch.equal(ya, x * 2)


@pytest.mark.parametrize("defect,where,first", [("past", "guard after y", "+0"), ("before", "guard before y", "-4"),
                                                ("tile_past", "guard after y", f"+{255 * COLS * 4}"), ("input", "body of input x", "+20")])
def test_stray_writes_are_reported_with_placement_and_offset(arena, defect, where, first):
    x, xa, ya, za = setup(arena)
    scale_kernel(arena, xa, ya, defect=defect)
    with pytest.raises(GuardViolation) as e:
        arena.verify()
    msg = str(e.value)
    assert where in msg and f"offsets {first} .." in msg, msg
    assert "neighbour" not in msg, "a write that is wrong by a whole tile still lands in the guard, not in the next tensor"
    n = {"past": 4, "before": 4, "tile_past": COLS * 4, "input": 4}[defect]
    assert f"{n} byte(s) changed" in msg, msg
    # and the same call without the defect passes
    arena.reset()
    x, xa, ya, _ = setup(arena)
    scale_kernel(arena, xa, ya)
    arena.verify()


def test_unwritten_output_element_fails_the_value_comparison(arena):
    x, xa, ya, _ = setup(arena)
    scale_kernel(arena, xa, ya, defect="unwritten")
    arena.verify()  # nothing outside was touched ...
    assert not torch.equal(ya, x * 2) and torch.isnan(ya[-1, -1]), "... but the element never written is still NaN"
    scale_kernel(arena, xa, ya)
    assert torch.equal(ya, x * 2)


def test_write_past_the_declared_workspace_size(arena):
    declared = 1000  # bytes, as a *_workspace_bytes query would return them
    ws = arena.place((declared,), torch.uint8, role="workspace", name="ws")
    assert arena.placement_of(ws).end - arena.placement_of(ws).start == declared
    wm, w0 = raw(arena, ws)
    wm[w0:w0 + declared] = 7  # all of the declared size: allowed
    arena.verify()
    wm[w0 + declared + 1] = 7
    with pytest.raises(GuardViolation, match=r"guard after ws .*offsets \+1 \.\. \+1"):
        arena.verify()


def rowsum_kernel(arena, x, rows):
    mem, x0 = raw(arena, x)
    return mem[x0:x0 + rows * COLS].reshape(rows, COLS).sum(0)


def test_reduction_over_one_row_too_many_changes_the_value(arena):
    """the weight-gradient tail: rows past M entering the sum.  Seen under BOTH poison modes"""
    x, xa, _, _ = setup(arena)
    ref = x.double().sum(0)
    good = rowsum_kernel(arena, xa, ROWS)
    assert torch.allclose(good.double(), ref, rtol=1e-5, atol=1e-5)
    bad = rowsum_kernel(arena, xa, ROWS + 1)
    assert not torch.allclose(bad.double(), ref, rtol=1e-3, atol=1e-3)
    assert (torch.isnan(bad).all() if arena.poison == "nan" else (bad > 1e37).all())
    arena.verify()  # (an over-READ changes no byte: only the value comparison can see it)


def softmax_kernel(arena, s, keys, max_keys=None):
    """row softmax over the first ``keys`` scores of a row whose pitch is ``keys`` (the row behind it, or the guard, follows);
    max_keys: how many scores enter the row maximum -- a hardware max, which returns the non-NaN operand (torch.fmax)"""
    mem, s0 = raw(arena, s)
    row = mem[s0:s0 + max(keys, max_keys or 0)]
    m = row[:max_keys or keys].clone()
    mx = m[0]
    for v in m[1:]:
        mx = torch.fmax(mx, v)
    p = torch.exp(row[:keys] - mx)
    return p / p.sum()


def test_softmax_over_one_key_too_many(arena):
    s = torch.randn(9)  # the LAST row of a score matrix: what follows it is the guard
    sa = arena.place(s, role="input", name="scores")
    ref = torch.softmax(s.double(), 0)
    assert torch.allclose(softmax_kernel(arena, sa, 9).double(), ref, atol=1e-6)
    bad = softmax_kernel(arena, sa, 10)
    assert not torch.allclose(bad[:9].double(), ref, atol=1e-3), "a stray key must change the probabilities"
    # the case that needs `huge`: the tail mask is applied to the probabilities but the row maximum covers one key too many.
    # A hardware max drops the NaN, so under `nan` the result is right and the bug invisible; under `huge` every exp underflows.
    sly = softmax_kernel(arena, sa, 9, max_keys=10)
    if arena.poison == "nan":
        assert torch.allclose(sly.double(), ref, atol=1e-6), "NaN poison alone cannot see a stray key in a hardware max"
    else:
        assert not torch.allclose(sly.double(), ref, atol=1e-3, equal_nan=False)
    arena.verify()


def test_routing_puts_a_wrappers_own_allocations_into_the_arena(arena):
    """a stand-in for simple_tad_amd.kernels: a module that allocates its output, a zeroed output, a padded operand copy and a grow-only
    workspace through its global ``torch``"""
    mod = types.SimpleNamespace(torch=torch, _workspaces={"stale": 1})

    def op(x, stray=False):
        t = mod.torch
        xp = t.nn.functional.pad(x, (0, 4))
        y = t.empty(x.shape, dtype=x.dtype, device=x.device)
        z = t.zeros((3,), dtype=t.float32, device=x.device)
        e = t.empty_like(x)
        e16 = t.empty_like(x, dtype=t.float16)  # (keywords do not leave the arena)
        ws = t.empty(100, dtype=t.uint8, device=x.device)
        mod._workspaces["k"] = ws
        host = t.empty(4)  # no device: not the arena's business
        scale_kernel(arena, x, y, defect="past" if stray else None)
        e.copy_(x)
        assert arena.contains(e16) and e16.dtype == t.float16 and not arena.contains(host)
        return xp, y, z, e, ws, host

    x, xa, _, _ = setup(arena)
    n0 = len(arena.placements)
    with arena.route(mod):
        assert not mod._workspaces, "cached workspaces are dropped on entry"
        xp, y, z, e, ws, host = op(xa)
    assert mod.torch is torch and not mod._workspaces
    roles = [p.role for p in arena.placements[n0:]]
    assert roles == ["input", "output", "output", "output", "output", "workspace"], roles
    for t in (xp, y, z, e, ws):
        arena.placement_of(t)
    with pytest.raises(KeyError):
        arena.placement_of(host)
    arena.verify()
    assert torch.equal(y, x * 2) and torch.equal(z, torch.zeros(3)) and torch.equal(xp[:, :COLS], x) and not xp[:, COLS:].any()
    with arena.route(mod):
        op(xa, stray=True)
    with pytest.raises(GuardViolation, match="guard after wrapper output"):
        arena.verify()


def test_guard_pattern_keeps_table_rows_valid(arena):
    table = torch.tensor([[10, 20, 4, 0], [30, 40, 4, 0]], dtype=torch.int64)
    ta = arena.place(table, guard_pattern=(table[0], torch.zeros(1, dtype=torch.int64)), name="table")
    mem, t0 = raw(arena, ta)
    assert torch.equal(mem[t0 - 8:t0].reshape(2, 4), table[:1].repeat(2, 1)) and not mem[t0 + 8:t0 + 64].any()
    arena.verify()


@pytest.mark.parametrize("dtype,offsets", [(torch.float32, (0, 4, 8, 12)), (torch.bfloat16, (0, 2, 6, 14)), (torch.uint8, (0, 1, 7, 15)),
                                           (torch.int64, (0, 8))])
def test_place_offset_moves_the_body_and_keeps_the_guards_tight(arena, dtype, offsets):
    """place(offset=k): the view starts k bytes behind a 256-byte boundary, the guard before it still ends immediately before its first
    byte, the guard after it still starts at the byte after its last, both at least as wide as without the offset; the next placement
    is back on the 256-byte grid; a stray write one element in front of the shifted body is reported inside the element in front of its first byte"""
    item = torch.empty((), dtype=dtype).element_size()
    kw = dict(index_range=9) if dtype == torch.int64 else {}
    for k in offsets:
        arena.reset()
        data = (torch.arange(ROWS * COLS) % 7).to(dtype).reshape(ROWS, COLS)
        t = arena.place(data, role="input", name="shifted", offset=k, **kw)
        nxt = arena.place((3, 5), torch.float32, role="output", name="next")
        p = arena.placement_of(t)
        assert t.data_ptr() % 256 == k and p.lo % 256 == arena.base % 256
        assert p.start - p.lo == GuardedArena.guard_bytes(data.shape, dtype) + k and p.hi - p.end >= GuardedArena.guard_bytes(data.shape, dtype)
        assert p.end - p.start == data.numel() * item and nxt.data_ptr() % 256 == 0
        assert same_bits(t, data)
        mem, t0 = raw(arena, t)
        if dtype in (torch.float32, torch.bfloat16):
            view, pat = poison_bits(dtype, arena.poison)
            assert int(bits(mem[t0 - 1:t0])) == pat and int(bits(mem[t0 + t.numel():t0 + t.numel() + 1])) == pat
            assert int(bits(mem[t0 - k // item - 1:t0 - k // item])) == pat, "the bytes the offset skipped are guard bytes too"
        elif dtype == torch.uint8:
            assert int(mem[t0 - 1]) == 0xFF and int(mem[t0 + t.numel()]) == 0xFF
        else:
            assert 0 <= int(mem[t0 - 1]) < 9 and 0 <= int(mem[t0 + t.numel()]) < 9
        arena.verify()
        mem[t0 - 1] = 100 if dtype != torch.uint8 else 3  # (differs from every guard value)
        with pytest.raises(GuardViolation, match=rf"guard before shifted.*offsets -[1-{item}] \.\. -\d relative to its first byte"):
            arena.verify()
    with pytest.raises(AssertionError):
        arena.place(torch.zeros(4), offset=2)  # not on the f32 element grid
