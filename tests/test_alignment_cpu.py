"""The pointer alignment contract on a machine without a GPU: the table (tests/alignment_contract.py) covers every pointer argument
of every exported symbol, and every ``align = N`` row is refused -- TAD_EINVAL, a message that names the argument and says "aligned" --
at every element-aligned offset below N, with every other argument valid (tests/alignment_cases.py).  Nothing here launches: only calls
that must be refused are made, on addresses inside one host buffer that nothing dereferences."""
import ctypes
import re

import pytest

import alignment_cases as cases_mod
import alignment_contract as AC
from simple_tad_amd import _lib


@pytest.fixture(scope="module")
def lib():
    from simple_tad_amd import build
    build.build(verbose=False)
    return _lib.load()


def test_every_pointer_argument_has_a_row():
    """a future entry point cannot be added without a contract: every symbol of _lib.SIGNATURES has a table entry whose keys are, in
    order, the names the header gives its c_void_p arguments (the stream aside); the entries are one of the three kinds"""
    protos = AC.prototypes()
    assert set(protos) == set(_lib.SIGNATURES), set(protos) ^ set(_lib.SIGNATURES)
    missing = [s for s in _lib.SIGNATURES if AC.pointer_arguments(s, protos) and s not in AC.CONTRACT]
    assert not missing, f"no alignment contract for {missing}"
    for sym in _lib.SIGNATURES:
        names = [n for _, n in AC.pointer_arguments(sym, protos)]
        if not names:
            assert sym not in AC.CONTRACT or not AC.CONTRACT[sym], f"{sym} takes no pointer"
            continue
        assert list(AC.CONTRACT[sym]) == names, f"{sym}: rows {list(AC.CONTRACT[sym])}, the header's pointer arguments {names}"
        for name, row in AC.CONTRACT[sym].items():
            assert isinstance(row, (AC.A, AC._Any, AC._Host)), (sym, name, row)
    assert set(AC.CONTRACT) <= set(_lib.SIGNATURES), set(AC.CONTRACT) - set(_lib.SIGNATURES)
    for half, bf in AC.TWIN_OF.items():
        assert AC.CONTRACT[half] is AC.CONTRACT[bf], "a twin shares its source, hence its rows"


def test_every_aligned_row_has_a_case_and_every_covered_row_its_test(lib):
    """every ``align = N`` row, each of its conditional requirements included, is exercised by a case; every `any` row either has a
    GPU case that carries the pointer, names the existing test that covers it, or is listed in alignment_cases.NOT_RUN"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for sym, table in AC.CONTRACT.items():
        built = cases_mod.cases(sym) if AC.TWIN_OF.get(sym, sym) in cases_mod.BUILDERS else []
        for name, row in table.items():
            carried = [c for c in built if any(p.name == name for _, p in c.pointers())]
            if isinstance(row, AC.A):
                assert carried, f"{sym}: no case carries {name} ({row})"
                assert {c.required(name) for c in carried} == row.allowed(), f"{sym}.{name}: the cases exercise {[c.required(name) for c in carried]} of {row}"
            elif isinstance(row, AC._Any) and row.covered:
                path, test = row.covered.split("::")
                assert re.search(rf"^def {test}\(", open(os.path.join(root, path)).read(), flags=re.M), f"{sym}.{name}: {row.covered} does not exist"
            elif isinstance(row, AC._Any):
                assert carried, f"{sym}: no case carries the `any` pointer {name}"
                if not any(c.gpu for c in carried):
                    assert name in cases_mod.NOT_RUN.get(sym, ()), f"{sym}: the `any` pointer {name} is in no GPU case and not listed as not run"


_BUF = ctypes.create_string_buffer(64 * 4096)


def fake_addresses(case):
    """a 4096-byte aligned address inside one host buffer per pointer argument, 4096 bytes apart: never dereferenced"""
    base = (ctypes.addressof(_BUF) + 4095) // 4096 * 4096
    out = {}
    for k, (i, p) in enumerate(case.pointers()):
        assert k < 62
        out[i] = base + k * 4096
    return out


def call(lib, case, addr):
    fn = getattr(lib, case.symbol)
    args = [ctypes.c_void_p(addr[i]) if i in addr else a for i, a in enumerate(case.args)]
    return fn(*args)


ALIGNED_SYMBOLS = sorted(sym for sym, table in AC.CONTRACT.items() if any(isinstance(r, AC.A) for r in table.values()))  # (the table alone: no library)


def test_every_entry_point_with_an_aligned_row_has_cases():
    assert set(ALIGNED_SYMBOLS) <= set(cases_mod.symbols()) and len(ALIGNED_SYMBOLS) >= 60


@pytest.mark.parametrize("sym", ALIGNED_SYMBOLS)
def test_misaligned_pointer_is_refused_by_name(lib, sym):
    """every case of the entry point (built here, after the library: the workspace sizes are the library's own), every ``align = N``
    pointer it carries, every element-aligned offset below N"""
    refused = 0
    for case in cases_mod.cases(sym):
        base = fake_addresses(case)
        for pos, p in case.pointers():
            need = case.required(p.name)
            if need is None:
                continue
            item = cases_mod.ITEM[p.dtype]
            offsets = list(range(item, need, item))
            assert offsets or need <= item, (case, p.name, need, item)
            pat = re.compile(rf"\b{re.escape(p.name)} is misaligned.*\b{need}-byte aligned".encode())
            for off in offsets:
                addr = dict(base)
                addr[pos] += off
                rc = call(lib, case, addr)
                msg = lib.tad_last_error_string()
                assert rc == -1, f"{case} with {p.name} + {off}: rc = {rc} ({msg})"
                assert pat.search(msg) and b"aligned" in msg, f"{case} with {p.name} + {off} was refused for another reason: {msg}"
                refused += 1
    assert refused > 0, f"{sym}: no refusal was exercised"
