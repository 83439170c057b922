"""The pointer alignment contract on the GPU (tests/alignment_contract.py, tests/alignment_cases.py).

Control for the refusals: every case's all-aligned call, on real tensors inside the guard arena, returns 0 (the cases describe valid
calls), and the same call with one ``align = N`` pointer moved by one element is refused with every output bit-identical to its
snapshot.  A misaligned ``align = N`` pointer never reaches a kernel: it is tested through refusals only.

The `any` rows: every pointer the table marks `any` is placed at every element-aligned offset within 16 bytes -- alone, and together
with every other `any` pointer of the call shifted by a different amount -- inside the guard arena, in both poison modes, and the
outputs are compared with the all-aligned call bit for bit.  The reductions whose summation order follows the address
(tad_grad_norm_coef here; tad_sumsq_f32 and tad_grad_segnorm have their own tests, named in the table) are held to fp64 with the bound
their existing test uses (tests/test_kernels_gpu.py::test_sumsq_alignment_tails_and_grad_norm_coef: 2e-6 relative on the norm, 4e-6 on
the coefficient).  The all-aligned result is the oracle here; its own correctness is what the rest of the suite pins.
"""
import ctypes

import pytest
import torch

import alignment_cases as AL
import alignment_contract as AC
from guarded import GuardedArena, POISON_MODES, same_bits

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "u16": torch.int16, "i32": torch.int32, "i64": torch.int64, "u64": torch.int64, "u8": torch.uint8, "f64": torch.float64}
OP16 = {"bf16": torch.bfloat16, "f16": torch.float16}
poison = pytest.mark.parametrize("poison", POISON_MODES)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def arena():
    return GuardedArena(64 << 20, "cuda")


def dtype_of(p, fmt):
    return OP16[fmt] if p.dtype == "op16" else TORCH[p.dtype]


def host_data(case):
    """{position: host tensor} of every pointer argument, the same for every placement of the case"""
    g = torch.Generator().manual_seed(20240607)
    out = {}
    for i, p in case.pointers():
        dt = dtype_of(p, case.fmt)
        if p.data is not None:
            t = p.data(torch, g).to(dt).reshape(p.shape)
        elif dt.is_floating_point and p.role in ("input", "inout"):
            t = torch.randn(p.shape, generator=g).to(dt)
        elif p.role in ("input", "inout"):
            t = torch.zeros(p.shape, dtype=dt)
        else:
            t = None  # an output / workspace: born NaN (0x7F bytes for integers)
        out[i] = t
    return out


def run(lib, arena, case, data, offsets=None, mode=None, expect=0):
    """place every pointer argument (offsets: {position: bytes}), call, verify the guards; returns (rc, {name: output clone})"""
    offsets = offsets or {}
    arena.reset(mode)
    placed = {}
    for i, p in case.pointers():
        dt = dtype_of(p, case.fmt)
        kw = dict(role=p.role, name=p.name, offset=offsets.get(i, 0))
        if not dt.is_floating_point or dt == torch.float64:
            if p.index_range is not None:
                kw["index_range"] = p.index_range
            elif dt != torch.uint8:
                kw["guard_pattern"] = (torch.zeros(1, dtype=dt), torch.zeros(1, dtype=dt))
        placed[i] = arena.place(data[i], **kw) if data[i] is not None else arena.place(p.shape, dt, **kw)
        assert placed[i].data_ptr() % 256 == offsets.get(i, 0)
    before = {i: placed[i].clone() for i, p in case.pointers() if p.role != "input"}
    args = [ctypes.c_void_p(placed[i].data_ptr()) if i in placed else a for i, a in enumerate(case.args)]
    rc = getattr(lib, case.symbol)(*args)
    torch.cuda.synchronize()
    msg = lib.tad_last_error_string() if rc else b""
    assert rc == expect, f"{case}: rc = {rc} ({msg})"
    arena.verify()
    if rc:
        for i, t in before.items():
            assert same_bits(t, placed[i]), f"{case}: a refused call changed {case.args[i].name}"
    outs = {p.name: placed[i].clone() for i, p in case.pointers() if p.role in ("output", "inout")}
    return rc, outs, msg


SYMBOLS = AL.symbols()  # (names only: the cases are built inside the tests, once the library is loaded)


def gpu_cases(sym):
    return [c for c in AL.cases(sym) if c.gpu]


@pytest.mark.parametrize("sym", [s for s in SYMBOLS if AC.TWIN_OF.get(s, s) not in AL.NOT_RUN])
def test_aligned_call_runs_and_each_misaligned_pointer_is_refused_untouched(lib, arena, sym):
    built = gpu_cases(sym)
    assert built, f"{sym}: no case runs on the GPU"
    for case in built:
        control(lib, arena, case)


def control(lib, arena, case):
    data = host_data(case)
    rc, outs, _ = run(lib, arena, case, data, mode="nan")
    for name, t in outs.items():
        if t.dtype.is_floating_point and [p for _, p in case.pointers() if p.name == name][0].role == "output":
            assert not torch.isnan(t).all(), f"{case}: the aligned call left {name} unwritten"
    for i, p in case.pointers():
        need = case.required(p.name)
        item = AL.ITEM[p.dtype]
        if need is None or need <= item:
            continue
        _, _, msg = run(lib, arena, case, data, offsets={i: item}, mode="nan", expect=-1)
        assert f"{p.name} is misaligned".encode() in msg, msg


# ------------------------------------------------------------------ the `any` rows
def any_pointers(case):
    out = []
    for i, p in case.pointers():
        row = AC.CONTRACT[case.symbol][p.name]
        if isinstance(row, AC._Any) and not row.covered:
            out.append((i, p, row))
        elif isinstance(row, AC.A) and case.required(p.name) == AL.ITEM[p.dtype] and AL.ITEM[p.dtype] > 1:
            out.append((i, p, AC.ANY))  # a conditional requirement that is the element size under this case's condition
    return out


def element_offsets(p):
    item = AL.ITEM[p.dtype]
    return list(range(0, 16, item))


ANY_SYMBOLS = [s for s in SYMBOLS if any(isinstance(r, AC._Any) and not r.covered for r in AC.CONTRACT[s].values())
               and AC.TWIN_OF.get(s, s) not in AL.NOT_RUN]  # (the table alone: no library)


def placements(case):
    """offset maps: each `any` pointer alone at every non-zero offset, then all of them together, neighbours shifted by different
    amounts (every offset of every pointer occurs in one of these as well)"""
    ptrs = any_pointers(case)
    out = [{i: off} for i, p, _ in ptrs for off in element_offsets(p)[1:]]
    most = max(len(element_offsets(p)) for _, p, _ in ptrs)
    if len(ptrs) > 1:
        for r in range(1, most):
            # pointer k moves by its offset number r + k + k // len: neighbours differ, and so do pointers a whole period apart
            out.append({i: element_offsets(p)[(r + k + k // len(element_offsets(p))) % len(element_offsets(p))] for k, (i, p, _) in enumerate(ptrs)})
    return out


NORM_RTOL, COEF_RTOL = 2e-6, 4e-6  # tests/test_kernels_gpu.py::test_sumsq_alignment_tails_and_grad_norm_coef


def compare(case, data, base, got, where):
    if AC.TWIN_OF.get(case.symbol, case.symbol) == "tad_grad_norm_coef":  # the summation order follows the address: fp64, the existing bounds
        x = [data[i] for i, p in case.pointers() if p.name == "x"][0].double()
        inv, mx = case.args[2], case.args[3]
        norm = float(x.norm()) * inv
        coef = inv * min(mx / (norm + 1e-6), 1.0)
        o = got["out3"].cpu().double()
        assert abs(float(o[0]) - norm) <= NORM_RTOL * norm and abs(float(o[1]) - coef) <= COEF_RTOL * coef and float(o[2]) == 0.0, (where, o, norm, coef)
        return
    for name in base:
        assert same_bits(base[name], got[name]), f"{case} {where}: {name} differs in bits from the all-aligned call"


@poison
@pytest.mark.parametrize("sym", ANY_SYMBOLS)
def test_any_pointer_gives_the_same_bits_at_every_offset(lib, arena, sym, poison):
    built = [c for c in gpu_cases(sym) if any_pointers(c)]
    names = {p.name for c in built for _, p, _ in any_pointers(c)}
    want = {n for n, r in AC.CONTRACT[sym].items() if isinstance(r, AC._Any) and not r.covered}
    assert want <= names, f"{sym}: no GPU case moves {sorted(want - names)}"
    for case in built:
        any_offsets(lib, arena, case, poison)


def any_offsets(lib, arena, case, poison):
    data = host_data(case)
    _, base, _ = run(lib, arena, case, data, mode=poison)
    for offs in placements(case):
        names = {case.args[i].name: o for i, o in offs.items()}
        _, got, _ = run(lib, arena, case, data, offsets=offs, mode=poison)
        compare(case, data, base, got, names)
    if AC.TWIN_OF.get(case.symbol, case.symbol) == "tad_grad_norm_coef":
        compare(case, data, base, base, "aligned")


def test_every_offset_of_every_any_pointer_is_placed(lib):
    for case in [c for sym in ANY_SYMBOLS for c in gpu_cases(sym) if any_pointers(c)]:
        seen = {}
        for offs in placements(case):
            for i, o in offs.items():
                seen.setdefault(i, set()).add(o)
        for i, p, _ in any_pointers(case):
            assert seen[i] | {0} == set(element_offsets(p)), (case, p.name)


def test_ema_tables_at_every_offset(lib, arena):
    """tad_ema_update's table holds the addresses of the tensors it updates, so its call is built here, after the placements, and not
    from a case: the all-aligned call returns 0, `tensors` (int64 rows: `any`) 8 bytes further gives the same bits, and `chunks`
    (8 bytes) 4 bytes further is refused with the tensors untouched"""
    from simple_tad_amd import kernels as K
    n = _lib_chunk() + 5
    g = torch.Generator().manual_seed(5)
    e0, m0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    results = []
    for mode in POISON_MODES:
        for off in (0, 8):
            arena.reset(mode)
            e, m = arena.place(e0, role="inout", name="ema"), arena.place(m0, name="model")
            table, nt, nc = K.ema_table([(e.data_ptr(), m.data_ptr(), n)])
            row = table[:4].clone()  # (guards of an address table: rows that stay valid)
            t = arena.place(table, name="table", guard_pattern=(row, row), offset=off)
            assert t.data_ptr() % 16 == off
            rc = lib.tad_ema_update(ctypes.c_void_p(t.data_ptr()), nt, ctypes.c_void_p(t.data_ptr() + 32 * nt), nc, 0.9, 0.1, None)
            torch.cuda.synchronize()
            assert rc == 0, lib.tad_last_error_string()
            arena.verify()
            results.append(e.clone())
            assert not same_bits(results[-1], e0.cuda())
            rc = lib.tad_ema_update(ctypes.c_void_p(t.data_ptr()), nt, ctypes.c_void_p(t.data_ptr() + 32 * nt + 4), nc, 0.9, 0.1, None)
            torch.cuda.synchronize()
            assert rc == -1 and b"chunks is misaligned" in lib.tad_last_error_string()
            assert same_bits(results[-1], e), "a refused call changed the EMA tensor"
    for r in results[1:]:
        assert same_bits(results[0], r)


def _lib_chunk():
    from simple_tad_amd import _lib
    return _lib.EMA_CHUNK


# ------------------------------------------------------------------ the wrappers' face
def shifted(t, elements=1):
    """a contiguous view of a fresh buffer that starts ``elements`` behind its (256-byte aligned) first element: passes the wrappers'
    device / dtype / contiguity checks"""
    buf = torch.empty(t.numel() + elements, dtype=t.dtype, device="cuda")
    v = buf[elements:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (elements * t.element_size()) % 16 != 0
    return v


def test_wrappers_refuse_a_contiguous_offset_view():
    """one representative wrapper per source file: the refusal of the C ABI surfaces as TadError"""
    from simple_tad_amd import _lib, kernels as K
    M, N, Kd = AL.LIN_SMALL
    op = torch.bfloat16
    x, w, b = torch.randn(M, Kd, device="cuda").to(op), torch.randn(N, Kd, device="cuda").to(op), torch.randn(N, device="cuda")
    B, Nt, H, d = AL.ATT
    qkv = torch.randn(B * Nt, 3 * H * d, device="cuda").to(op)
    f32 = torch.randn(5, 12, device="cuda")
    calls = {
        "gemm.hip x": lambda: K.linear_fwd(shifted(x), w, b),
        "gemm.hip bias": lambda: K.linear_fwd(x, w, shifted(b)),
        "layernorm.hip": lambda: K.layernorm_fwd(shifted(f32), torch.ones(12, device="cuda"), torch.zeros(12, device="cuda"), 1e-6),
        "attn_fwd.hip": lambda: K.attn_fwd(shifted(qkv), B, Nt, H, d ** -0.5),
        "attn_f32.hip": lambda: K.attn_fwd_f32(shifted(qkv.float()), B, Nt, H, d ** -0.5),
        "attn_colsum.hip": lambda: K.attn_colsum(shifted(qkv), torch.zeros(B, H, Nt, device="cuda"), torch.ones(B, Nt, device="cuda"), B, Nt, H, d ** -0.5),
        "elementwise.hip": lambda: K.meanpool_fwd(shifted(torch.randn(2, 5, 12, device="cuda"))),
        "mae.hip": lambda: K.gather_rows(shifted(f32), torch.tensor([0, 3], dtype=torch.int32, device="cuda")),
        "precise.hip": lambda: K.colsum_f32(shifted(f32)),
    }
    for what, fn in calls.items():
        with pytest.raises(_lib.TadError, match="is misaligned"):
            fn()
        torch.cuda.synchronize()
    out, lse = K.attn_fwd(qkv, B, Nt, H, d ** -0.5)[:2]
    with pytest.raises(_lib.TadError, match="is misaligned"):  # attn_bwd.hip
        K.attn_bwd(qkv, out, shifted(out), lse, B, Nt, H, d ** -0.5)
