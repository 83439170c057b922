"""The extension ABI (include/tad_mi355x_ext.h, tadx_*) held to the discipline tests/test_cabi_cpu.py and tests/test_alignment_cpu.py impose
on the frozen core ABI: exports == header prototypes == _lib.EXT_SIGNATURES, a contract row for every pointer argument
(tests/alignment_contract_ext.py), every ``align = N`` row refused by name at every element-aligned offset below N, and the host-side
validation.  Nothing here launches: only calls that must be refused are made, on addresses inside one host buffer that nothing
dereferences."""
import ctypes
import re
import subprocess

import pytest

import alignment_contract as AC
import alignment_contract_ext as ACX
from simple_tad_amd import _lib

F32, BF16, F16 = _lib.TAD_F32, _lib.TAD_BF16, _lib.TAD_F16


@pytest.fixture(scope="module")
def lib_path():
    from simple_tad_amd import build
    return build.build(verbose=False)


@pytest.fixture(scope="module")
def lib(lib_path):
    return _lib.load()


def test_exports_header_and_binding_are_one_set(lib_path, lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (tadx_[a-z0-9_]+)", out))
    protos = ACX.prototypes()
    assert exported == set(protos) == set(_lib.EXT_SIGNATURES), (exported ^ set(protos), set(protos) ^ set(_lib.EXT_SIGNATURES))
    assert len(exported) == 7
    for name, (_, args) in _lib.EXT_SIGNATURES.items():
        assert len(args) == len(protos[name]), name
    assert lib.tadx_abi_version() == _lib.EXT_ABI_VERSION == 1
    # the core ABI is untouched: no tadx_ name in it, its version where it was, and no twin for the run-time-format entry points
    assert not any(s.startswith("tadx") for s in _lib.SIGNATURES) and _lib.ABI_VERSION == 5
    assert not any(s.startswith("tadx") for s in (*_lib.F16_TWINS, *_lib.F16_TWINS.values()))
    assert not any(s.endswith("_f16") for s in exported)


def test_every_pointer_argument_has_a_row():
    protos = ACX.prototypes()
    assert set(ACX.CONTRACT) <= set(_lib.EXT_SIGNATURES)
    for sym in _lib.EXT_SIGNATURES:
        names = [n for _, n in ACX.pointer_arguments(sym, protos)]
        if not names:
            assert sym not in ACX.CONTRACT, f"{sym} takes no pointer"
            continue
        assert list(ACX.CONTRACT[sym]) == names, f"{sym}: rows {list(ACX.CONTRACT[sym])}, the header's pointer arguments {names}"
        for name, row in ACX.CONTRACT[sym].items():
            assert isinstance(row, (AC.A, AC._Any, AC._Host)), (sym, name, row)


# One valid call per (symbol, condition): {argument name: value}; pointer arguments are given as ("ptr", item size) and get fake addresses.
# `need` overrides the requirement of the rows whose condition the case exercises.
def P(item):
    return ("ptr", item)


ROWS, D, M, A_ = 5, 132, 9, 128


def _cases(lib):
    ws_r = lib.tadx_rmsnorm_bwd_workspace_bytes(ROWS, D)
    ws_q = lib.tadx_qk_rmsnorm_bwd_workspace_bytes(M, A_)
    assert ws_r == 1 * D * 4 and ws_q == 2 * 1 * A_ * 4
    assert lib.tadx_rmsnorm_bwd_workspace_bytes(70, 768) == 3 * 768 * 4  # 32 rows per block
    assert lib.tadx_rmsnorm_bwd_workspace_bytes(5, 1792) == 1792 * 4 and lib.tadx_qk_rmsnorm_bwd_workspace_bytes(5, 1792) == 2 * 1792 * 4
    # LayerNorm's backward deals its rows the same way (csrc/rownorm.h): three quantities, 50 blocks of 32 rows for 1569 rows
    assert lib.tad_layernorm_bwd_workspace_bytes(5, 1792) == 3 * 1792 * 4 and lib.tad_layernorm_bwd_workspace_bytes(1569, 1000) == 3 * 50 * 1000 * 4
    out = []
    for ydt, yitem, need in ((F32, 4, {}), (BF16, 2, {"y": 8}), (F16, 2, {"y": 8})):
        out.append(("tadx_rmsnorm_fwd", dict(x=P(4), gamma=P(4), y=P(yitem), y_dtype=ydt, rrms=P(4), rows=ROWS, D=D, eps=1e-6, stream=None), need))
    for dyt, item, need in ((F32, 4, {}), (BF16, 2, {"dy": 8}), (F16, 2, {"dy": 8})):
        out.append(("tadx_rmsnorm_bwd", dict(dy=P(item), dy_dtype=dyt, x=P(4), gamma=P(4), rrms=P(4), dres=P(4), dx=P(4), dx16=P(2),
                                             dx16_fmt=BF16 if dyt != F16 else F16, dgamma=P(4), accumulate=0, ws=P(4), ws_bytes=ws_r,
                                             rows=ROWS, D=D, stream=None), need))
    for fmt in (BF16, F16):
        out.append(("tadx_qk_rmsnorm_fwd", dict(qkv32=P(4), gq=P(4), gk=P(4), qkv16=P(2), fmt=fmt, rr=P(4), q_out_scale=0.18, M=M, A=A_,
                                                eps=1e-6, stream=None), {}))
        out.append(("tadx_qk_rmsnorm_bwd", dict(dqkv16=P(2), fmt=fmt, qkv32=P(4), gq=P(4), gk=P(4), rr=P(4), q_out_scale=0.18, dqkv_pre16=P(2),
                                                dgq=P(4), dgk=P(4), accumulate=1, ws=P(4), ws_bytes=ws_q, M=M, A=A_, stream=None), {}))
    return out


_BUF = ctypes.create_string_buffer(32 * 4096)
_BASE = (ctypes.addressof(_BUF) + 4095) // 4096 * 4096


def _call(lib, sym, values, shift=None, **override):
    names = ACX.prototypes()[sym]
    assert list(values) == names, (sym, list(values), names)
    args = []
    for k, n in enumerate(names):
        v = override.get(n, values[n])
        if isinstance(v, tuple) and v[0] == "ptr":
            v = ctypes.c_void_p(_BASE + k * 4096 + (shift[1] if shift and shift[0] == n else 0))
        args.append(v)
    rc = getattr(lib, sym)(*args)
    return rc, lib.tad_last_error_string()


@pytest.mark.parametrize("sym", sorted(ACX.CONTRACT))
def test_misaligned_pointer_is_refused_by_name(lib, sym):
    """every case of the entry point, every ``align = N`` pointer, every element-aligned offset below N"""
    refused, seen = 0, {name: set() for name, row in ACX.CONTRACT[sym].items() if isinstance(row, AC.A)}
    for s, values, need in _cases(lib):
        if s != sym:
            continue
        for name, row in ACX.CONTRACT[sym].items():
            if not isinstance(row, AC.A):
                continue
            n = need.get(name, row.n)
            assert n in row.allowed()
            seen[name].add(n)
            item = values[name][1]
            offsets = list(range(item, n, item))
            assert offsets
            pat = re.compile(rf"\b{re.escape(name)} is misaligned.*\b{n}-byte aligned".encode())
            for off in offsets:
                rc, msg = _call(lib, sym, values, shift=(name, off))
                assert rc == -1, f"{sym} with {name} + {off}: rc = {rc} ({msg})"
                assert pat.search(msg) and msg.startswith(sym[len("tadx_"):].encode()), f"{sym} with {name} + {off} was refused for another reason: {msg}"
                refused += 1
    assert refused > 0
    for name, row in ACX.CONTRACT[sym].items():
        if isinstance(row, AC.A):
            assert seen[name] == row.allowed(), f"{sym}.{name}: the cases exercise {seen[name]} of {row}"


def test_host_validation_without_gpu(lib):
    cases = {}
    for s, values, _ in _cases(lib):
        cases.setdefault(s, values)

    def refused(sym, what, rc_want=-1, **override):
        rc, msg = _call(lib, sym, cases[sym], **override)
        assert rc == rc_want and what.encode() in msg, (sym, override, rc, msg)

    # null pointers: every required one (rrms / rr of the forwards, dres and dx16 are optional)
    required = {"tadx_rmsnorm_fwd": ("x", "gamma", "y"), "tadx_rmsnorm_bwd": ("dy", "x", "gamma", "rrms", "dx", "dgamma", "ws"),
                "tadx_qk_rmsnorm_fwd": ("qkv32", "gq", "gk", "qkv16"),
                "tadx_qk_rmsnorm_bwd": ("dqkv16", "qkv32", "gq", "gk", "rr", "dqkv_pre16", "dgq", "dgk", "ws")}
    for sym, names in required.items():
        for n in names:
            refused(sym, "null pointer", **{n: None})
    # D % 4, D > 2048 (and A alike), a row count of zero
    for sym, dim in (("tadx_rmsnorm_fwd", "D"), ("tadx_rmsnorm_bwd", "D"), ("tadx_qk_rmsnorm_fwd", "A"), ("tadx_qk_rmsnorm_bwd", "A")):
        refused(sym, f"{dim}=6 must be a multiple of 4", **{dim: 6})
        refused(sym, f"{dim}=2052 must be a multiple of 4 and <= 2048", **{dim: 2052})
        refused(sym, f"{dim}=0", **{dim: 0})
        refused(sym, "must be", **{"rows" if dim == "D" else "M": 0})
    # a bad dtype / format
    refused("tadx_rmsnorm_fwd", "bad y_dtype 3", y_dtype=3)
    refused("tadx_rmsnorm_bwd", "bad dy_dtype -1", dy_dtype=-1)
    refused("tadx_rmsnorm_bwd", "bad dx16_fmt 0", dx16_fmt=F32)
    refused("tadx_qk_rmsnorm_fwd", "bad fmt 0", fmt=F32)
    refused("tadx_qk_rmsnorm_bwd", "bad fmt 3", fmt=3)
    refused("tadx_qk_rmsnorm_fwd", "q_out_scale", q_out_scale=0.0)
    refused("tadx_qk_rmsnorm_bwd", "q_out_scale", q_out_scale=-1.0)
    # a workspace one byte short
    refused("tadx_rmsnorm_bwd", "workspace too small", rc_want=-3, ws_bytes=cases["tadx_rmsnorm_bwd"]["ws_bytes"] - 1)
    refused("tadx_qk_rmsnorm_bwd", "workspace too small", rc_want=-3, ws_bytes=cases["tadx_qk_rmsnorm_bwd"]["ws_bytes"] - 1)
