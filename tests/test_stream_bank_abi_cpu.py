"""The stream-bank ABI (include/tad_mi355x_bank.h, tadb_*): the sixth surface, in a library of its own
(simple_tad_amd/libtad_mi355x_bank.so), held to the discipline tests/test_reconstruct_abi_cpu.py imposes on the fifth: exports ==
header prototypes == _lib.BANK_SIGNATURES, no other C name exported and none of these names on any older surface, a contract row for
every pointer argument, every refusal made on the host and naming its argument or its row.  Nothing here launches: only the host-side
plan check runs to the end, and of the launching entry point only calls that must be refused are made, on addresses inside one host
buffer that nothing dereferences."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from alignment_contract import A, ANY, HOST
from simple_tad_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tad_mi355x_bank.h")
NAMES = {"tadb_abi_version", "tadb_last_error_string", "tadb_ingest_plan_check", "tadb_ingest_frames"}

# the header's "Pointer alignment", as data: src and table move as 4-byte words, the store may lie anywhere
CONTRACT = {"tadb_ingest_plan_check": dict(table_host=HOST),
            "tadb_ingest_frames": dict(src=A(4), store=ANY, table=A(4))}


def prototypes():
    """{symbol: [argument names]} as include/tad_mi355x_bank.h declares them"""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(tadb_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        params = m.group(2).strip()
        out[m.group(1)] = [] if params in ("", "void") else [re.findall(r"[A-Za-z_0-9]+", p)[-1] for p in params.split(",")]
    return out


@pytest.fixture(scope="module")
def paths():
    from simple_tad_amd import build
    first = build.build(verbose=False)
    assert first.endswith("libtad_mi355x.so"), "build() still returns the first library's path"
    assert os.path.exists(build.BANK_LIB) and build.BANK_LIB == _lib.BANK_LIB_PATH
    assert os.path.exists(build.SERVE_LIB) and os.path.exists(build.RECON_LIB)
    return first, build.SERVE_LIB, build.RECON_LIB, build.BANK_LIB


@pytest.fixture(scope="module")
def lib(paths):
    return _lib.load_bank()


def _defined(path):
    return subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout


def test_exports_header_and_binding_are_one_set(paths, lib):
    *older, bank = paths
    out = _defined(bank)
    exported = set(re.findall(r" T (tadb_[a-z0-9_]+)", out))
    protos = prototypes()
    assert exported == set(protos) == set(_lib.BANK_SIGNATURES) == NAMES
    for name, (_, args) in _lib.BANK_SIGNATURES.items():
        assert len(args) == len(protos[name]), name
    # no other C name, and no function or variable of the library's C++ at all: what is left is the kernel's handle
    other = [ln.split() for ln in out.splitlines() if ln.split() and ln.split()[-1] not in NAMES]
    c_names = [s[-1] for s in other if not s[-1].startswith("_Z") and not s[-1].startswith("__hip_")]
    assert not c_names, f"other C names exported: {c_names}"
    assert not [s[-1] for s in other if s[1] in "TtWw"], "only the tadb_ entry points are exported functions"
    assert not any("set_error" in s[-1] or "check_launch" in s[-1] or "g_bank_err" in s[-1] for s in other)
    assert all("ingest_frames_kernel" in s[-1] for s in other if s[-1].startswith("_Z"))
    # none of the five older surfaces knows a tadb_ name
    for p in older:
        assert not re.findall(r"\btadb_[a-z0-9_]+", _defined(p)), p
    assert not any(s.startswith("tadb") for s in (*_lib.SIGNATURES, *_lib.EXT_SIGNATURES, *_lib.PRETRAIN_SIGNATURES, *_lib.SERVE_SIGNATURES,
                                                  *_lib.RECON_SIGNATURES))
    inc = os.path.dirname(HEADER)
    for h in ("tad_mi355x.h", "tad_mi355x_ext.h", "tad_mi355x_pretrain.h", "tad_mi355x_serve.h", "tad_mi355x_recon.h"):
        assert "tadb_" not in open(os.path.join(inc, h)).read(), h
    assert lib.tadb_abi_version() == _lib.BANK_ABI_VERSION == 1
    head = open(HEADER).read()
    assert "#define TADB_ABI_VERSION 1" in head
    for name, value in (("TADB_ROW_WORDS", _lib.BANK_ROW_WORDS), ("TADB_MAX_FRAMES", _lib.BANK_MAX_FRAMES), ("TADB_MAX_SETS", _lib.BANK_MAX_SETS),
                        ("TADB_MAX_EXTENT", _lib.BANK_MAX_EXTENT), ("TADB_SWAP_RB", _lib.BANK_SWAP_RB)):
        assert re.search(rf"#define {name} {value}\b", head), name
    assert _lib.BANK_MAX_SETS == _lib.FR_MAX_SETS == 64


def test_the_build_keeps_the_new_library_apart(paths):
    from simple_tad_amd import build
    assert build.SERVE_SOURCES == ["iv2_serve.hip"] and build.RECON_SOURCES == ["mae_reconstruct.hip"] and build.BANK_SOURCES == ["stream_bank.hip"]
    assert not set(build.BANK_SOURCES) & (set(build.SOURCES) | set(build.F16_SOURCES) | set(build.SERVE_SOURCES) | set(build.RECON_SOURCES))
    assert "frame_resize.hip" in build.SOURCES, "the one-size resize stays where it is"
    deps = build.EXTRA_DEPS["stream_bank.hip"]
    assert any(d.endswith("tad_mi355x_bank.h") for d in deps) and "frame_io.h" in deps
    assert "tad_mi355x_bank.h" in open(os.path.join(build.CSRC, "stream_bank.hip")).read()
    # an up-to-date tree: build() compiles nothing and returns the first library's path
    before = {p: os.path.getmtime(p) for p in paths}
    assert build.build(verbose=False) == paths[0]
    assert {p: os.path.getmtime(p) for p in paths} == before


def test_every_pointer_argument_has_a_row():
    protos = prototypes()
    for sym, (_, args) in _lib.BANK_SIGNATURES.items():
        names = [n for a, n in zip(args, protos[sym]) if a is ctypes.c_void_p and n != "stream"]
        if not names:
            assert sym not in CONTRACT, f"{sym} takes no pointer"
            continue
        assert list(CONTRACT[sym]) == names, f"{sym}: rows {list(CONTRACT[sym])}, the header's pointer arguments {names}"
    assert "Alignment: src, table: 4 bytes; store: any address; table_host: a host array." in open(HEADER).read()


# ---------------------------------------------------------------- a well-formed plan, and one broken word at a time
S_H, S_W, F = 6, 5, 9
HEAD = 8  # bytes in front of the first frame


def _coeffs(n_src, n_dst):
    from simple_tad_amd.frame_resize import cubic_coeffs
    return cubic_coeffs(n_src, n_dst)


def good_plan():
    """three frames (4 x 7, 3 x 7, 4 x 2) -> 6 x 5: two widths, two heights; returns (table int32 [n], K, nh, nv, src_bytes)"""
    frames = [(4, 7), (3, 7), (4, 2)]
    ws, hs = [7, 2], [4, 3]
    rows, at = [], HEAD
    for k, (h, w) in enumerate(frames):
        rows.append([at, h, w, (5, 0, 8)[k], ws.index(w), hs.index(h), k & 1, 0])
        at += (h * w * 3 + 3) // 4 * 4
    words = [np.asarray(rows, dtype=np.int32).reshape(-1)]
    for n_in, out in [(w, S_W) for w in ws] + [(h, S_H) for h in hs]:
        first, k = _coeffs(n_in, out)
        words += [np.asarray([n_in, out, 0, 0], dtype=np.int32), first, k.reshape(-1)]
    return np.ascontiguousarray(np.concatenate(words), dtype=np.int32), len(frames), len(ws), len(hs), at


def _check(lib, tab, K, nh, nv, src_bytes, n_words=None, F_=F, Sh=S_H, Sw=S_W):
    rc = lib.tadb_ingest_plan_check(tab.ctypes.data, tab.size if n_words is None else n_words, K, nh, nv, src_bytes, F_, Sh, Sw)
    return rc, lib.tadb_last_error_string()


def test_a_well_formed_plan_passes(lib):
    tab, K, nh, nv, nbytes = good_plan()
    rc, msg = _check(lib, tab, K, nh, nv, nbytes)
    assert rc == 0, msg
    assert tab.size == K * _lib.BANK_ROW_WORDS + nh * (_lib.FR_SET_HEAD + 5 * S_W) + nv * (_lib.FR_SET_HEAD + 5 * S_H)


def test_every_plan_check_refusal_names_its_argument_or_row(lib):
    tab0, K, nh, nv, nbytes = good_plan()
    R, HS = _lib.BANK_ROW_WORDS, K * _lib.BANK_ROW_WORDS
    VS = HS + nh * (_lib.FR_SET_HEAD + 5 * S_W)

    def refused(what, edit=None, **kw):
        tab = tab0.copy()
        if edit is not None:
            edit(tab)
        rc, msg = _check(lib, tab, kw.pop("K", K), kw.pop("nh", nh), kw.pop("nv", nv), kw.pop("src_bytes", nbytes), **kw)
        assert rc == -1 and what.encode() in msg and msg.startswith(b"ingest_plan_check: "), (what, rc, msg)

    def word(i, v):
        return lambda t: t.__setitem__(i, v)

    # the word count
    refused(f"n_words={tab0.size - 1}, expected", n_words=tab0.size - 1)
    refused(f"n_words={tab0.size + 5}, expected", n_words=tab0.size + 5)
    # extents below 1 (and above the limit)
    refused("row 1: h=0 outside", word(1 * R + 1, 0))
    refused("row 2: w=-3 outside", word(2 * R + 2, -3))
    refused(f"row 0: h={_lib.BANK_MAX_EXTENT + 1} outside", word(1, _lib.BANK_MAX_EXTENT + 1))
    # a frame not inside [0, src_bytes), a misaligned or negative offset
    refused("row 2: the frame's bytes", src_bytes=nbytes - 1)
    refused("row 0: the frame's bytes", word(0, nbytes))
    refused("row 1: src_off=94 must be a non-negative multiple of 4", word(1 * R, 94))
    refused("row 1: src_off=-4 must be a non-negative multiple of 4", word(1 * R, -4))
    # the slot
    refused(f"row 0: slot={F} outside the store", word(3, F))
    refused("row 2: slot=-1 outside the store", word(2 * R + 3, -1))
    refused("row 2: slot=5 is already named by row 0", word(2 * R + 3, 5))
    refused("row 0: slot=5 outside the store", F_=5)
    # the set indices, and a set not stated for the row's extent
    refused(f"row 0: hset={nh} outside", word(4, nh))
    refused("row 1: vset=-1 outside", word(1 * R + 5, -1))
    refused("row 2: its hset 0 is stated for 7 columns, the frame has w=2", word(2 * R + 4, 0))
    refused("row 1: its vset 0 is stated for 4 rows, the frame has h=3", word(1 * R + 5, 0))
    refused("horizontal set 1: output extent 4, expected 5", word(HS + (_lib.FR_SET_HEAD + 5 * S_W) + 1, 4))
    # first outside [-2, in - 2]
    refused("horizontal set 0: output 2 has its first tap at -3", word(HS + _lib.FR_SET_HEAD + 2, -3))
    refused("horizontal set 0: output 4 has its first tap at 6", word(HS + _lib.FR_SET_HEAD + 4, 6))
    refused("vertical set 1: output 0 has its first tap at 2", word(VS + (_lib.FR_SET_HEAD + 5 * S_H) + _lib.FR_SET_HEAD, 2))
    # sum |k| above TAD_FR_MAX_ABS_SUM: {-385, 2819 - 385 ...}: 2819 in all
    def heavy(t):
        t[VS + _lib.FR_SET_HEAD + S_H + 4:VS + _lib.FR_SET_HEAD + S_H + 8] = (-385, 1600, 834, 0)
    refused(f"vertical set 0: output 1: sum |k| = 2819 is above {_lib.FR_MAX_ABS_SUM}", heavy)
    # unknown flag bits, the spare word
    refused("row 1: flags=0x3 holds unknown bits", word(1 * R + 6, 3))
    refused("row 0: flags=0x80000000 holds unknown bits", word(6, -2 ** 31))
    refused("row 2: word 7 is 1", word(2 * R + 7, 1))
    # the scalars
    refused("K=0 must be in", K=0)
    refused(f"K={_lib.BANK_MAX_FRAMES + 1} must be in", K=_lib.BANK_MAX_FRAMES + 1)
    refused("n_hsets=0 must be in", nh=0)
    refused("n_vsets=65 must be in", nv=65)
    refused("S_h=0 must be in", Sh=0)
    refused("S_w=16385 must be in", Sw=16385)
    refused("F=0 must be in", F_=0)
    refused("src_bytes=0 must be positive", src_bytes=0)
    rc = lib.tadb_ingest_plan_check(None, 10, K, nh, nv, nbytes, F, S_H, S_W)
    assert rc == -1 and b"table_host is null" in lib.tadb_last_error_string()
    # sum |k| = 2818 itself passes
    tab = tab0.copy()
    tab[VS + _lib.FR_SET_HEAD + S_H + 4:VS + _lib.FR_SET_HEAD + S_H + 8] = (-385, 1600, 833, 0)
    assert _check(lib, tab, K, nh, nv, nbytes)[0] == 0


# ---------------------------------------------------------------- the launching entry point: refusals only
def P(item):
    return ("ptr", item)


CASE = dict(src=P(4), src_bytes=4096, store=P(1), F=F, table=P(4), n_words=3 * 8 + 2 * (4 + 5 * S_W) + 2 * (4 + 5 * S_H), K=3, n_hsets=2,
            n_vsets=2, S_h=S_H, S_w=S_W, stream=None)

_BUF = ctypes.create_string_buffer(32 * 4096)
_BASE = (ctypes.addressof(_BUF) + 4095) // 4096 * 4096


def _addr(k, off=0):
    return ctypes.c_void_p(_BASE + k * 4096 + off)


def _call(lib, shift=None, **override):
    sym = "tadb_ingest_frames"
    names = prototypes()[sym]
    assert list(CASE) == names, (list(CASE), names)
    args = []
    for k, n in enumerate(names):
        v = override.get(n, CASE[n])
        if isinstance(v, tuple) and v[0] == "ptr":
            v = _addr(k, shift[1] if shift and shift[0] == n else 0)
        args.append(v)
    rc = getattr(lib, sym)(*args)
    return rc, lib.tadb_last_error_string()


def test_misaligned_pointer_is_refused_by_name(lib):
    """every 4-byte row at every offset below 4; store, which has no requirement, is never what a refusal names"""
    refused = 0
    for name, row in CONTRACT["tadb_ingest_frames"].items():
        if row is ANY:
            continue
        pat = re.compile(rf"\b{re.escape(name)} is misaligned.*\b{row.n}-byte aligned".encode())
        for off in (1, 2, 3):
            rc, msg = _call(lib, shift=(name, off))
            assert rc == -1, f"{name} + {off}: rc = {rc} ({msg})"
            assert pat.search(msg) and msg.startswith(b"ingest_frames"), f"{name} + {off} was refused for another reason: {msg}"
            refused += 1
    assert refused == 6
    for off in (1, 2, 3):
        rc, msg = _call(lib, shift=("store", off), K=0)
        assert rc == -1 and b"K=0" in msg and b"misaligned" not in msg


def test_host_validation_without_gpu(lib):
    def refused(what, **override):
        rc, msg = _call(lib, **override)
        assert rc == -1 and what.encode() in msg and msg.startswith(b"ingest_frames: "), (override, rc, msg)

    for n in ("src", "store", "table"):
        refused(f"{n} is null", **{n: None})
    refused("K=0 must be in", K=0)
    refused(f"K={_lib.BANK_MAX_FRAMES + 1} must be in", K=_lib.BANK_MAX_FRAMES + 1)
    refused("n_hsets=0 must be in", n_hsets=0)
    refused("n_vsets=65 must be in", n_vsets=65)
    refused("S_h=-1 must be in", S_h=-1)
    refused("S_w=0 must be in", S_w=0)
    refused("F=0 must be in", F=0)
    refused("src_bytes=-8 must be positive", src_bytes=-8)
    refused(f"n_words={CASE['n_words'] + 1}, expected", n_words=CASE["n_words"] + 1)
    # the other libraries' error texts are their own
    first, serve, recon = _lib.load(), _lib.load_serve(), _lib.load_recon()
    before = (first.tad_last_error_string(), serve.tads_last_error_string(), recon.tadr_last_error_string())
    refused("src is null", src=None)
    assert (first.tad_last_error_string(), serve.tads_last_error_string(), recon.tadr_last_error_string()) == before
