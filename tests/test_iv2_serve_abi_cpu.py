"""The serving ABI (include/tad_mi355x_serve.h, tads_*): the fourth surface, the only one in a library of its own
(simple_tad_amd/libtad_mi355x_serve.so), held to the discipline tests/test_visible_tokens_abi_cpu.py imposes on the third: exports ==
header prototypes == _lib.SERVE_SIGNATURES, no other C name exported and none of these in the first library, a contract row for every
pointer argument, every row refused by name at every misaligned offset, and the host-side validation message by message.  Nothing here
launches: only calls that must be refused are made, on addresses inside one host buffer that nothing dereferences."""
import ctypes
import os
import re
import subprocess

import pytest

from alignment_contract import A
from simple_tad_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tad_mi355x_serve.h")
NAMES = {"tads_abi_version", "tads_last_error_string", "tads_class_token_entry_fwd", "tads_class_token_entry_bwd", "tads_residual_rmsnorm_fwd"}

# the header's "Pointer alignment", as data: f32 operands move as float4, the 16-bit output four values at a time
CONTRACT = {
    "tads_class_token_entry_fwd": dict(patch=A(16), cls=A(16), pos=A(16), out=A(16)),
    "tads_class_token_entry_bwd": dict(g=A(16), dpatch=A(16), dpos=A(16), dcls=A(16)),
    "tads_residual_rmsnorm_fwd": dict(x=A(16), y=A(16), ls_gamma=A(16), norm_gamma=A(16), x_out=A(16), xn=A(8)),
}
OPTIONAL = {"tads_class_token_entry_bwd": ("dpatch", "dpos", "dcls"), "tads_residual_rmsnorm_fwd": ("ls_gamma",)}


def prototypes():
    """{symbol: [argument names]} as include/tad_mi355x_serve.h declares them"""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(tads_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        params = m.group(2).strip()
        out[m.group(1)] = [] if params in ("", "void") else [re.findall(r"[A-Za-z_0-9]+", p)[-1] for p in params.split(",")]
    return out


@pytest.fixture(scope="module")
def paths():
    from simple_tad_amd import build
    first = build.build(verbose=False)
    assert first.endswith("libtad_mi355x.so"), "build() still returns the first library's path"
    assert os.path.exists(build.SERVE_LIB) and build.SERVE_LIB == _lib.SERVE_LIB_PATH
    return first, build.SERVE_LIB


@pytest.fixture(scope="module")
def lib(paths):
    return _lib.load_serve()


def _defined(path):
    return subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout


def test_exports_header_and_binding_are_one_set(paths, lib):
    first, serve = paths
    out = _defined(serve)
    exported = set(re.findall(r" T (tads_[a-z0-9_]+)", out))
    protos = prototypes()
    assert exported == set(protos) == set(_lib.SERVE_SIGNATURES) == NAMES
    for name, (_, args) in _lib.SERVE_SIGNATURES.items():
        assert len(args) == len(protos[name]), name
    # no other C name, and no function or variable of the library's C++ (the error text, the launch check) at all: what is left are
    # the kernels' handles, which the HIP runtime looks up by their mangled names
    other = [ln.split() for ln in out.splitlines() if ln.split() and ln.split()[-1] not in NAMES]
    c_names = [s[-1] for s in other if not s[-1].startswith("_Z") and not s[-1].startswith("__hip_")]
    assert not c_names, f"other C names exported: {c_names}"
    assert not [s[-1] for s in other if s[1] in "Tt"], "only the tads_ entry points are exported functions"
    assert not any("set_error" in s[-1] or "check_launch" in s[-1] or "g_serve_err" in s[-1] for s in other)
    assert all("_kernel" in s[-1] for s in other if s[-1].startswith("_Z"))
    # the first library knows nothing of this surface
    assert not re.findall(r"\btads_[a-z0-9_]+", _defined(first))
    assert not any(s.startswith("tads") for s in (*_lib.SIGNATURES, *_lib.EXT_SIGNATURES, *_lib.PRETRAIN_SIGNATURES))
    assert lib.tads_abi_version() == _lib.SERVE_ABI_VERSION == 1
    assert "#define TADS_ABI_VERSION 1" in open(HEADER).read()


def test_the_build_keeps_the_serving_library_apart():
    from simple_tad_amd import build
    assert build.SERVE_SOURCES == ["iv2_serve.hip"]
    assert not set(build.SERVE_SOURCES) & (set(build.SOURCES) | set(build.F16_SOURCES))
    deps = build.EXTRA_DEPS["iv2_serve.hip"]
    assert "rownorm.h" in deps and any(d.endswith("tad_mi355x_serve.h") for d in deps)
    src = open(os.path.join(build.CSRC, "iv2_serve.hip")).read()
    assert '#include "rownorm.h"' in src and "tad_mi355x_serve.h" in src


def test_every_pointer_argument_has_a_row():
    protos = prototypes()
    for sym, (_, args) in _lib.SERVE_SIGNATURES.items():
        names = [n for a, n in zip(args, protos[sym]) if a is ctypes.c_void_p and n != "stream"]
        if not names:
            assert sym not in CONTRACT, f"{sym} takes no pointer"
            continue
        assert list(CONTRACT[sym]) == names, f"{sym}: rows {list(CONTRACT[sym])}, the header's pointer arguments {names}"
    txt = open(HEADER).read()
    assert "Alignment: patch, cls, pos, out: 16 bytes." in txt and "Alignment: g, dpatch, dpos, dcls: 16 bytes." in txt
    assert "Alignment: x, y, ls_gamma, norm_gamma, x_out: 16 bytes; xn: 8 bytes." in txt


def P(item):
    return ("ptr", item)


B, N, D, ROWS = 3, 5, 132, 7
CASES = {
    "tads_class_token_entry_fwd": dict(patch=P(4), cls=P(4), pos=P(4), out=P(4), B=B, N=N, D=D, stream=None),
    "tads_class_token_entry_bwd": dict(g=P(4), dpatch=P(4), dpos=P(4), dcls=P(4), accumulate=0, B=B, N=N, D=D, stream=None),
    "tads_residual_rmsnorm_fwd": dict(x=P(4), y=P(4), ls_gamma=P(4), norm_gamma=P(4), x_out=P(4), xn=P(2), xn_fmt=_lib.TAD_BF16, rows=ROWS, D=D,
                                      eps=1e-6, stream=None),
}

_BUF = ctypes.create_string_buffer(32 * 4096)
_BASE = (ctypes.addressof(_BUF) + 4095) // 4096 * 4096


def _addr(k, off=0):
    return ctypes.c_void_p(_BASE + k * 4096 + off)


def _call(lib, sym, shift=None, **override):
    values, names = CASES[sym], prototypes()[sym]
    assert list(values) == names, (sym, list(values), names)
    args = []
    for k, n in enumerate(names):
        v = override.get(n, values[n])
        if isinstance(v, tuple) and v[0] == "ptr":
            v = _addr(k, shift[1] if shift and shift[0] == n else 0)
        args.append(v)
    rc = getattr(lib, sym)(*args)
    return rc, lib.tads_last_error_string()


@pytest.mark.parametrize("sym", sorted(CONTRACT))
def test_misaligned_pointer_is_refused_by_name(lib, sym):
    """every 16-byte row at every 4-byte offset below 16 and the 8-byte row at every 2-byte offset below 8, also with each other
    optional argument absent"""
    refused = 0
    for name, row in CONTRACT[sym].items():
        need = row.n
        step = 4 if need == 16 else 2
        pat = re.compile(rf"\b{re.escape(name)} is misaligned.*\b{need}-byte aligned".encode())
        for off in range(step, need, step):
            others = [{}] + [{o: None} for o in OPTIONAL.get(sym, ()) if o != name]
            for override in others:
                rc, msg = _call(lib, sym, shift=(name, off), **override)
                assert rc == -1, f"{sym} with {name} + {off}: rc = {rc} ({msg})"
                assert pat.search(msg) and msg.startswith(sym[len("tads_"):].encode()), \
                    f"{sym} with {name} + {off} was refused for another reason: {msg}"
                refused += 1
    assert refused >= 12
    # an 8-byte offset of the 16-bit output is fine: with another argument broken, that argument is what is named
    if sym == "tads_residual_rmsnorm_fwd":
        rc, msg = _call(lib, sym, shift=("xn", 8), D=6)
        assert rc == -1 and b"D=6 must be a multiple of 4" in msg and b"xn is misaligned" not in msg


def test_host_validation_without_gpu(lib):
    def refused(sym, what, **override):
        rc, msg = _call(lib, sym, **override)
        assert rc == -1 and what.encode() in msg, (sym, override, rc, msg)

    for n in ("patch", "cls", "pos", "out"):
        refused("tads_class_token_entry_fwd", "class_token_entry_fwd: null pointer", **{n: None})
    refused("tads_class_token_entry_bwd", "class_token_entry_bwd: null pointer", g=None)
    refused("tads_class_token_entry_bwd", "class_token_entry_bwd: dpatch, dpos and dcls are all null", dpatch=None, dpos=None, dcls=None)
    for sym in ("tads_class_token_entry_fwd", "tads_class_token_entry_bwd"):
        who = sym[len("tads_"):]
        for dim in ("B", "N", "D"):
            for bad in (0, -1):
                refused(sym, f"{who}: B=", **{dim: bad})
                refused(sym, f"{dim}={bad}", **{dim: bad})
                refused(sym, "must all be positive", **{dim: bad})
        refused(sym, f"{who}: D=6 must be a multiple of 4", D=6)
        refused(sym, f"{who}: D=130 must be a multiple of 4", D=130)
    rr = "tads_residual_rmsnorm_fwd"
    for n in ("x", "y", "x_out"):
        refused(rr, "residual_rmsnorm_fwd: null pointer", **{n: None})
    for bad in (0, -1):
        refused(rr, f"residual_rmsnorm_fwd: rows={bad} must be positive", rows=bad)
    for bad in (0, -4, 6, 130, 2052, 4096):
        refused(rr, f"residual_rmsnorm_fwd: D={bad} must be a multiple of 4 and <= 2048", D=bad)
    for bad in (_lib.TAD_F32, 3, -1):
        refused(rr, f"residual_rmsnorm_fwd: bad xn_fmt {bad}", xn_fmt=bad)
    refused(rr, "residual_rmsnorm_fwd: norm_gamma without xn", xn=None)
    refused(rr, "residual_rmsnorm_fwd: xn without norm_gamma", norm_gamma=None)
    names = prototypes()[rr]
    refused(rr, "residual_rmsnorm_fwd: x_out may be x, it may not be y", x_out=_addr(names.index("y")))
    # ... while x_out == x (in place) is no reason to refuse: with that and a bad D, D is what is named
    refused(rr, "D=6 must be a multiple of 4", x_out=_addr(names.index("x")), D=6)
    # the first library's error text is its own
    first = _lib.load()
    before = first.tad_last_error_string()
    refused(rr, "null pointer", x=None)
    assert first.tad_last_error_string() == before
