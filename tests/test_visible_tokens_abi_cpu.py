"""The pre-training ABI (include/tad_mi355x_pretrain.h, tadp_*), the third surface of the library, held to the discipline
tests/test_cabi_cpu.py, tests/test_alignment_cpu.py and tests/test_iv2_abi_cpu.py impose on the other two: exports == header prototypes
== _lib.PRETRAIN_SIGNATURES, a contract row for every pointer argument, every 16-byte row refused by name at every 4-byte offset below
16, and the host-side validation message by message.  Nothing here launches: only calls that must be refused are made, on addresses
inside one host buffer that nothing dereferences."""
import ctypes
import os
import re
import subprocess

import pytest

import alignment_contract as AC
from alignment_contract import A, ANY
from simple_tad_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tad_mi355x_pretrain.h")

# the header's "Pointer alignment", as data (the classes of tests/alignment_contract.py): f32 operands move as float4, indices int by int
CONTRACT = {
    "tadp_visible_tokens_fwd": dict(x=A(16), pos=A(16), tok=ANY, out=A(16)),
    "tadp_visible_tokens_bwd": dict(g=A(16), slot=ANY, dx=A(16), dpos=A(16)),
}


def prototypes():
    """{symbol: [argument names]} as include/tad_mi355x_pretrain.h declares them"""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(tadp_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        params = m.group(2).strip()
        out[m.group(1)] = [] if params in ("", "void") else [re.findall(r"[A-Za-z_0-9]+", p)[-1] for p in params.split(",")]
    return out


@pytest.fixture(scope="module")
def lib_path():
    from simple_tad_amd import build
    return build.build(verbose=False)


@pytest.fixture(scope="module")
def lib(lib_path):
    return _lib.load()


def test_exports_header_and_binding_are_one_set(lib_path, lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (tadp_[a-z0-9_]+)", out))
    protos = prototypes()
    assert exported == set(protos) == set(_lib.PRETRAIN_SIGNATURES) == {"tadp_abi_version", "tadp_visible_tokens_fwd", "tadp_visible_tokens_bwd"}
    for name, (_, args) in _lib.PRETRAIN_SIGNATURES.items():
        assert len(args) == len(protos[name]), name
    assert lib.tadp_abi_version() == _lib.PRETRAIN_ABI_VERSION == 1
    assert "#define TADP_ABI_VERSION 1" in open(HEADER).read()
    # f32 only: compiled once, no twin
    from simple_tad_amd import build
    assert "visible_tokens.hip" in build.SOURCES and "visible_tokens.hip" not in build.F16_SOURCES
    assert any(d.endswith("tad_mi355x_pretrain.h") for d in build.EXTRA_DEPS["visible_tokens.hip"])
    assert not any(s.endswith("_f16") for s in exported)


def test_the_core_and_extension_surfaces_are_unchanged(lib_path, lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    every = set(re.findall(r" T (tad[a-z]*_[a-z0-9_]+)", out))
    core, ext, pre = ({s for s in every if s.startswith(p)} for p in ("tad_", "tadx_", "tadp_"))
    assert every == core | ext | pre, f"exports under another prefix: {every - core - ext - pre}"
    assert pre == set(_lib.PRETRAIN_SIGNATURES) and len(pre) == 3
    assert core == set(_lib.SIGNATURES) == set(AC.prototypes()) and _lib.ABI_VERSION == lib.tad_abi_version() == 5
    assert ext == set(_lib.EXT_SIGNATURES) and len(ext) == 7 and _lib.EXT_ABI_VERSION == lib.tadx_abi_version() == 1
    assert not any(s.startswith(("tadp", "tadx")) for s in _lib.SIGNATURES)
    assert not any(s.startswith("tadp") for s in (*_lib.EXT_SIGNATURES, *_lib.F16_TWINS, *_lib.F16_TWINS.values(), *_lib.VARIANT_F16_TWINS))


def test_every_pointer_argument_has_a_row():
    protos = prototypes()
    for sym, (_, args) in _lib.PRETRAIN_SIGNATURES.items():
        names = [n for a, n in zip(args, protos[sym]) if a is ctypes.c_void_p and n != "stream"]
        if not names:
            assert sym not in CONTRACT, f"{sym} takes no pointer"
            continue
        assert list(CONTRACT[sym]) == names, f"{sym}: rows {list(CONTRACT[sym])}, the header's pointer arguments {names}"
    # the header states the same rule in words
    txt = open(HEADER).read()
    assert "Alignment: x, pos, out: 16 bytes; tok: any." in txt and "Alignment: g, dx, dpos: 16 bytes; slot: any." in txt


def P(item):
    return ("ptr", item)


B, N, NV, D = 3, 5, 2, 132
CASES = {
    "tadp_visible_tokens_fwd": dict(x=P(4), pos=P(4), tok=P(4), out=P(4), B=B, N=N, Nv=NV, D=D, stream=None),
    "tadp_visible_tokens_bwd": dict(g=P(4), slot=P(4), dx=P(4), dpos=P(4), accumulate=0, B=B, N=N, Nv=NV, D=D, stream=None),
}

_BUF = ctypes.create_string_buffer(32 * 4096)
_BASE = (ctypes.addressof(_BUF) + 4095) // 4096 * 4096


def _call(lib, sym, shift=None, **override):
    values, names = CASES[sym], prototypes()[sym]
    assert list(values) == names, (sym, list(values), names)
    args = []
    for k, n in enumerate(names):
        v = override.get(n, values[n])
        if isinstance(v, tuple) and v[0] == "ptr":
            v = ctypes.c_void_p(_BASE + k * 4096 + (shift[1] if shift and shift[0] == n else 0))
        args.append(v)
    rc = getattr(lib, sym)(*args)
    return rc, lib.tad_last_error_string()


@pytest.mark.parametrize("sym", sorted(CONTRACT))
def test_misaligned_pointer_is_refused_by_name(lib, sym):
    """every 16-byte row at every 4-byte offset below 16, also with the other optional output absent; the index tables pass anywhere"""
    refused = 0
    for name, row in CONTRACT[sym].items():
        if not isinstance(row, A):
            continue
        assert row.allowed() == {16}
        pat = re.compile(rf"\b{re.escape(name)} is misaligned.*\b16-byte aligned".encode())
        for off in (4, 8, 12):
            others = [{}]
            if sym.endswith("_bwd") and name in ("dx", "dpos"):
                others.append({"dpos" if name == "dx" else "dx": None})
            for override in others:
                rc, msg = _call(lib, sym, shift=(name, off), **override)
                assert rc == -1, f"{sym} with {name} + {off}: rc = {rc} ({msg})"
                assert pat.search(msg) and msg.startswith(sym[len("tadp_"):].encode()), f"{sym} with {name} + {off} was refused for another reason: {msg}"
                refused += 1
    assert refused >= 9
    # an index table on an odd int is not what a call is refused for: with another argument broken, that argument is what is named
    idx = "tok" if sym.endswith("_fwd") else "slot"
    rc, msg = _call(lib, sym, shift=(idx, 4), D=6)
    assert rc == -1 and b"D=6 must be a multiple of 4" in msg and idx.encode() + b" is misaligned" not in msg


def test_host_validation_without_gpu(lib):
    def refused(sym, what, **override):
        rc, msg = _call(lib, sym, **override)
        assert rc == -1 and what.encode() in msg, (sym, override, rc, msg)

    for n in ("x", "pos", "tok", "out"):
        refused("tadp_visible_tokens_fwd", "visible_tokens_fwd: null pointer", **{n: None})
    for n in ("g", "slot"):
        refused("tadp_visible_tokens_bwd", "visible_tokens_bwd: null pointer", **{n: None})
    # dx and dpos are each optional, not both
    refused("tadp_visible_tokens_bwd", "visible_tokens_bwd: dx and dpos are both null", dx=None, dpos=None)
    for sym in CASES:
        who = sym[len("tadp_"):]
        for dim in ("B", "N", "Nv", "D"):
            for bad in (0, -1):
                refused(sym, f"{who}: B=", **{dim: bad})
                refused(sym, f"{dim}={bad}", **{dim: bad})
                refused(sym, "must all be positive", **{dim: bad})
        refused(sym, f"{who}: Nv=6 exceeds N=5", Nv=6)
        refused(sym, f"{who}: D=6 must be a multiple of 4", D=6)
        refused(sym, f"{who}: D=130 must be a multiple of 4", D=130)
