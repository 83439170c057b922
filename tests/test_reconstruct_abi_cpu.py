"""The reconstruction ABI (include/tad_mi355x_recon.h, tadr_*): the fifth surface, in a library of its own
(simple_tad_amd/libtad_mi355x_recon.so), held to the discipline tests/test_iv2_serve_abi_cpu.py imposes on the fourth: exports ==
header prototypes == _lib.RECON_SIGNATURES, no other C name exported and none of these names on any older surface, a contract row for
every pointer argument, every refusal made on the host and naming its argument.  Nothing here launches: only calls that must be refused
are made, on addresses inside one host buffer that nothing dereferences."""
import ctypes
import os
import re
import subprocess

import pytest

from alignment_contract import A, ANY
from simple_tad_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tad_mi355x_recon.h")
NAMES = {"tadr_abi_version", "tadr_last_error_string", "tadr_mae_reconstruct"}

# the header's "Pointer alignment", as data: the f32 / int32 operands move one element at a time, frames may lie anywhere
CONTRACT = {"tadr_mae_reconstruct": dict(videos=A(4), pred=A(4), slot=A(4), frames=ANY, err=A(4))}


def prototypes():
    """{symbol: [argument names]} as include/tad_mi355x_recon.h declares them"""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(tadr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        params = m.group(2).strip()
        out[m.group(1)] = [] if params in ("", "void") else [re.findall(r"[A-Za-z_0-9]+", p)[-1] for p in params.split(",")]
    return out


@pytest.fixture(scope="module")
def paths():
    from simple_tad_amd import build
    first = build.build(verbose=False)
    assert first.endswith("libtad_mi355x.so"), "build() still returns the first library's path"
    assert os.path.exists(build.RECON_LIB) and build.RECON_LIB == _lib.RECON_LIB_PATH
    assert os.path.exists(build.SERVE_LIB)
    return first, build.SERVE_LIB, build.RECON_LIB


@pytest.fixture(scope="module")
def lib(paths):
    return _lib.load_recon()


def _defined(path):
    return subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout


def test_exports_header_and_binding_are_one_set(paths, lib):
    first, serve, recon = paths
    out = _defined(recon)
    exported = set(re.findall(r" T (tadr_[a-z0-9_]+)", out))
    protos = prototypes()
    assert exported == set(protos) == set(_lib.RECON_SIGNATURES) == NAMES
    for name, (_, args) in _lib.RECON_SIGNATURES.items():
        assert len(args) == len(protos[name]), name
    # no other C name, and no function or variable of the library's C++ at all: what is left are the kernels' handles
    other = [ln.split() for ln in out.splitlines() if ln.split() and ln.split()[-1] not in NAMES]
    c_names = [s[-1] for s in other if not s[-1].startswith("_Z") and not s[-1].startswith("__hip_")]
    assert not c_names, f"other C names exported: {c_names}"
    assert not [s[-1] for s in other if s[1] in "Tt"], "only the tadr_ entry points are exported functions"
    assert not any("set_error" in s[-1] or "check_launch" in s[-1] or "g_recon_err" in s[-1] for s in other)
    assert all("mae_reconstruct_kernel" in s[-1] for s in other if s[-1].startswith("_Z"))
    # none of the four older surfaces knows a tadr_ name
    assert not re.findall(r"\btadr_[a-z0-9_]+", _defined(first)) and not re.findall(r"\btadr_[a-z0-9_]+", _defined(serve))
    assert not any(s.startswith("tadr") for s in (*_lib.SIGNATURES, *_lib.EXT_SIGNATURES, *_lib.PRETRAIN_SIGNATURES, *_lib.SERVE_SIGNATURES))
    inc = os.path.dirname(HEADER)
    for h in ("tad_mi355x.h", "tad_mi355x_ext.h", "tad_mi355x_pretrain.h", "tad_mi355x_serve.h"):
        assert "tadr_" not in open(os.path.join(inc, h)).read(), h
    assert lib.tadr_abi_version() == _lib.RECON_ABI_VERSION == 1
    assert "#define TADR_ABI_VERSION 1" in open(HEADER).read()


def test_the_build_keeps_the_new_library_apart(paths):
    from simple_tad_amd import build
    assert build.SERVE_SOURCES == ["iv2_serve.hip"] and build.RECON_SOURCES == ["mae_reconstruct.hip"]
    assert not set(build.RECON_SOURCES) & (set(build.SOURCES) | set(build.F16_SOURCES) | set(build.SERVE_SOURCES))
    assert "mae.hip" in build.SOURCES, "the target kernel stays where it is"
    assert any(d.endswith("tad_mi355x_recon.h") for d in build.EXTRA_DEPS["mae_reconstruct.hip"])
    assert "tad_mi355x_recon.h" in open(os.path.join(build.CSRC, "mae_reconstruct.hip")).read()
    # an up-to-date tree: build() compiles nothing and returns the first library's path
    before = {p: os.path.getmtime(p) for p in paths}
    assert build.build(verbose=False) == paths[0]
    assert {p: os.path.getmtime(p) for p in paths} == before


def test_every_pointer_argument_has_a_row():
    protos = prototypes()
    for sym, (_, args) in _lib.RECON_SIGNATURES.items():
        names = [n for a, n in zip(args, protos[sym]) if a is ctypes.c_void_p and n != "stream"]
        if not names:
            assert sym not in CONTRACT, f"{sym} takes no pointer"
            continue
        assert list(CONTRACT[sym]) == names, f"{sym}: rows {list(CONTRACT[sym])}, the header's pointer arguments {names}"
    assert "Alignment: videos, pred, slot, err: 4 bytes; frames: any address." in open(HEADER).read()


def P(item):
    return ("ptr", item)


MEAN3 = (ctypes.c_float * 3)(0.485, 0.456, 0.406)
STD3 = (ctypes.c_float * 3)(0.229, 0.224, 0.225)
# N = 2 * 2 * 3 = 12 tokens of 2 * 16 * 16 = 512 pixels
CASE = dict(videos=P(4), pred=P(4), slot=P(4), frames=P(1), err=P(4), B=2, n_mask=9, T=4, H=32, W=48, tubelet=2, patch=16, mean3=MEAN3, std3=STD3,
            normalize_target=1, visible_gain=1.0, stream=None)

_BUF = ctypes.create_string_buffer(32 * 4096)
_BASE = (ctypes.addressof(_BUF) + 4095) // 4096 * 4096


def _addr(k, off=0):
    return ctypes.c_void_p(_BASE + k * 4096 + off)


def _call(lib, shift=None, **override):
    sym = "tadr_mae_reconstruct"
    names = prototypes()[sym]
    assert list(CASE) == names, (list(CASE), names)
    args = []
    for k, n in enumerate(names):
        v = override.get(n, CASE[n])
        if isinstance(v, tuple) and v[0] == "ptr":
            v = _addr(k, shift[1] if shift and shift[0] == n else 0)
        args.append(v)
    rc = getattr(lib, sym)(*args)
    return rc, lib.tadr_last_error_string()


def test_misaligned_pointer_is_refused_by_name(lib):
    """every 4-byte row at every offset below 4, also with each optional output absent; frames, which has no requirement, is never
    what a refusal names"""
    refused = 0
    for name, row in CONTRACT["tadr_mae_reconstruct"].items():
        if row is ANY:
            continue
        pat = re.compile(rf"\b{re.escape(name)} is misaligned.*\b{row.n}-byte aligned".encode())
        for off in (1, 2, 3):
            for override in [{}] + [{o: None} for o in ("frames", "err") if o != name]:
                rc, msg = _call(lib, shift=(name, off), **override)
                assert rc == -1, f"{name} + {off}: rc = {rc} ({msg})"
                assert pat.search(msg) and msg.startswith(b"mae_reconstruct"), f"{name} + {off} was refused for another reason: {msg}"
                refused += 1
    assert refused >= 12 * 2
    for off in (1, 2, 3):
        rc, msg = _call(lib, shift=("frames", off), B=0)
        assert rc == -1 and b"B=0" in msg and b"misaligned" not in msg


def test_host_validation_without_gpu(lib):
    def refused(what, **override):
        rc, msg = _call(lib, **override)
        assert rc == -1 and what.encode() in msg and msg.startswith(b"mae_reconstruct: "), (override, rc, msg)

    refused("T=5 must be a positive multiple of tubelet=2", T=5)
    refused("H=33 must be a positive multiple of patch=16", H=33)
    refused("W=40 must be a positive multiple of patch=16", W=40)
    refused("T=4 must be a positive multiple of tubelet=0", tubelet=0)
    refused("H=32 must be a positive multiple of patch=0", patch=0)
    refused("tubelet*patch^2 = 1 outside [2, 1024]", T=4, H=32, W=48, tubelet=1, patch=1)
    refused("tubelet*patch^2 = 2048 outside [2, 1024]", T=4, H=32, W=64, tubelet=2, patch=32)
    for bad in (0, -1):
        refused(f"B={bad} must be positive", B=bad)
    for bad in (-1, 13):
        refused(f"n_mask={bad} outside [0, N=12]", n_mask=bad)
    refused("pred is null with n_mask=9", pred=None)
    refused("frames and err are both null", frames=None, err=None)
    for bad, shown in ((-0.25, "-0.25"), (1.5, "1.5"), (float("nan"), "nan"), (float("inf"), "inf")):
        refused(f"visible_gain={shown} outside [0, 1]", visible_gain=bad)
    for c in range(3):
        for bad in (0.0, -0.5, float("nan")):
            std = (ctypes.c_float * 3)(*STD3)
            std[c] = bad
            refused(f"std3[{c}]=", std3=std)
            refused("must be positive", std3=std)
    for n in ("videos", "slot", "mean3", "std3"):
        refused(f"{n} is null", **{n: None})
    refused("more than 2^31 - 1 workgroups", B=2 ** 30, n_mask=0, pred=None)
    # pred may be NULL when nothing is masked: with that and another argument broken, the other argument is what is named
    refused("B=0 must be positive", pred=None, n_mask=0, B=0)
    # the other libraries' error texts are their own
    first, serve = _lib.load(), _lib.load_serve()
    before = (first.tad_last_error_string(), serve.tads_last_error_string())
    refused("videos is null", videos=None)
    assert (first.tad_last_error_string(), serve.tads_last_error_string()) == before
