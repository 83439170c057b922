"""The YUV-ingest ABI (include/tad_mi355x_yuv.h, tady_*): the seventh surface, in a library of its own
(simple_tad_amd/libtad_mi355x_yuv.so), held to the discipline tests/test_stream_bank_abi_cpu.py imposes on the sixth: exports ==
header prototypes == _lib.YUV_SIGNATURES, no other C name exported and none of these names on any older surface, a contract row for
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

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tad_mi355x_yuv.h")
NAMES = {"tady_abi_version", "tady_last_error_string", "tady_ingest_plan_check", "tady_ingest_yuv"}

# the header's "Pointer alignment", as data: src and table move as 4-byte words, the store may lie anywhere
CONTRACT = {"tady_ingest_plan_check": dict(table_host=HOST),
            "tady_ingest_yuv": dict(src=A(4), store=ANY, table=A(4))}


def prototypes():
    """{symbol: [argument names]} as include/tad_mi355x_yuv.h declares them"""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(tady_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        params = m.group(2).strip()
        out[m.group(1)] = [] if params in ("", "void") else [re.findall(r"[A-Za-z_0-9]+", p)[-1] for p in params.split(",")]
    return out


@pytest.fixture(scope="module")
def paths():
    from simple_tad_amd import build
    first = build.build(verbose=False)
    assert first.endswith("libtad_mi355x.so"), "build() still returns the first library's path"
    assert os.path.exists(build.YUV_LIB) and build.YUV_LIB == _lib.YUV_LIB_PATH
    assert os.path.exists(build.SERVE_LIB) and os.path.exists(build.RECON_LIB) and os.path.exists(build.BANK_LIB)
    return first, build.SERVE_LIB, build.RECON_LIB, build.BANK_LIB, build.YUV_LIB


@pytest.fixture(scope="module")
def lib(paths):
    return _lib.load_yuv()


def _defined(path):
    return subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout


def test_exports_header_and_binding_are_one_set(paths, lib):
    *older, yuv = paths
    out = _defined(yuv)
    exported = set(re.findall(r" T (tady_[a-z0-9_]+)", out))
    protos = prototypes()
    assert exported == set(protos) == set(_lib.YUV_SIGNATURES) == NAMES
    for name, (_, args) in _lib.YUV_SIGNATURES.items():
        assert len(args) == len(protos[name]), name
    # no other C name, and no function or variable of the library's C++ at all: what is left is the kernel's handle
    other = [ln.split() for ln in out.splitlines() if ln.split() and ln.split()[-1] not in NAMES]
    c_names = [s[-1] for s in other if not s[-1].startswith("_Z") and not s[-1].startswith("__hip_")]
    assert not c_names, f"other C names exported: {c_names}"
    assert not [s[-1] for s in other if s[1] in "TtWw"], "only the tady_ entry points are exported functions"
    assert not any("set_error" in s[-1] or "check_launch" in s[-1] or "g_yuv_err" in s[-1] for s in other)
    assert all("ingest_yuv_kernel" in s[-1] for s in other if s[-1].startswith("_Z"))
    # none of the six older surfaces knows a tady_ name
    for p in older:
        assert not re.findall(r"\btady_[a-z0-9_]+", _defined(p)), p
    assert not any(s.startswith("tady") for s in (*_lib.SIGNATURES, *_lib.EXT_SIGNATURES, *_lib.PRETRAIN_SIGNATURES, *_lib.SERVE_SIGNATURES,
                                                  *_lib.RECON_SIGNATURES, *_lib.BANK_SIGNATURES))
    inc = os.path.dirname(HEADER)
    for h in ("tad_mi355x.h", "tad_mi355x_ext.h", "tad_mi355x_pretrain.h", "tad_mi355x_serve.h", "tad_mi355x_recon.h", "tad_mi355x_bank.h"):
        assert "tady_" not in open(os.path.join(inc, h)).read(), h
    assert lib.tady_abi_version() == _lib.YUV_ABI_VERSION == 1
    head = open(HEADER).read()
    assert "#define TADY_ABI_VERSION 1" in head
    for name, value in (("TADY_ROW_WORDS", _lib.YUV_ROW_WORDS), ("TADY_CSET_WORDS", _lib.YUV_CSET_WORDS), ("TADY_MAX_FRAMES", _lib.YUV_MAX_FRAMES),
                        ("TADY_MAX_SETS", _lib.YUV_MAX_SETS), ("TADY_MAX_CSETS", _lib.YUV_MAX_CSETS), ("TADY_MAX_EXTENT", _lib.YUV_MAX_EXTENT),
                        ("TADY_BGR", _lib.YUV_BGR)):
        assert re.search(rf"#define {name} {value}\b", head), name
    assert _lib.YUV_MAX_SETS == _lib.FR_MAX_SETS == 64
    # the header says what the contract is: its own formula, not the bytes of an OpenCV build
    assert "THE CONTRACT IS THE FORMULA ABOVE AS WRITTEN HERE, not the bytes of any OpenCV" in head


def test_the_build_keeps_the_new_library_apart(paths):
    from simple_tad_amd import build
    assert build.YUV_SOURCES == ["yuv_ingest.hip"]
    assert build.SERVE_SOURCES == ["iv2_serve.hip"] and build.RECON_SOURCES == ["mae_reconstruct.hip"] and build.BANK_SOURCES == ["stream_bank.hip"]
    assert len(build.SOURCES) == 32 and len(build.F16_SOURCES) == 10 and build.SOURCES[0] == "capi.hip" and build.SOURCES[-1] == "visible_tokens.hip"
    assert not set(build.YUV_SOURCES) & (set(build.SOURCES) | set(build.F16_SOURCES) | set(build.SERVE_SOURCES) | set(build.RECON_SOURCES)
                                        | set(build.BANK_SOURCES))
    deps = build.EXTRA_DEPS["yuv_ingest.hip"]
    assert any(d.endswith("tad_mi355x_yuv.h") for d in deps) and "frame_io.h" in deps
    src = open(os.path.join(build.CSRC, "yuv_ingest.hip")).read()
    assert "tad_mi355x_yuv.h" in src and '#include "frame_io.h"' in src and "tad_mi355x_bank.h" not in src
    # an up-to-date tree: build() compiles nothing and returns the first library's path
    before = {p: os.path.getmtime(p) for p in paths}
    assert build.build(verbose=False) == paths[0]
    assert {p: os.path.getmtime(p) for p in paths} == before


def test_every_pointer_argument_has_a_row():
    protos = prototypes()
    for sym, (_, args) in _lib.YUV_SIGNATURES.items():
        names = [n for a, n in zip(args, protos[sym]) if a is ctypes.c_void_p and n != "stream"]
        if not names:
            assert sym not in CONTRACT, f"{sym} takes no pointer"
            continue
        assert list(CONTRACT[sym]) == names, f"{sym}: rows {list(CONTRACT[sym])}, the header's pointer arguments {names}"
    assert "Alignment: src, table: 4 bytes; store: any address; table_host: a host array." in open(HEADER).read()


# ---------------------------------------------------------------- a well-formed plan, and one broken word at a time
S_H, S_W, F = 6, 5, 9
HEAD = 8  # bytes in front of the first frame
BT601 = (16, 1220542, 1673527, -409993, -852492, 2116026)
BT709F = (0, 1048576, 1651297, -196424, -490864, 1945738)
SET_H, SET_V = _lib.FR_SET_HEAD + 5 * S_W, _lib.FR_SET_HEAD + 5 * S_H


def _coeffs(n_src, n_dst):
    from simple_tad_amd.frame_resize import cubic_coeffs
    return cubic_coeffs(n_src, n_dst)


def good_plan():
    """three frames -> 6 x 5: an NV12 frame 4 x 7 with pitches 8 and 9, an I420 frame 3 x 7 with pitches 7 and 4, an NV21 frame 4 x 2 with
    pitches 5 and 2; two widths, two heights, two colour sets.  Returns (table int32 [n], K, nh, nv, nc, src_bytes)"""
    ws, hs = [7, 2], [4, 3]
    rows, at = [], HEAD
    # NV12 4 x 7: luma 4 rows of 8, chroma 2 rows of 9 (8 live bytes)
    rows.append([at, 8, at + 32, at + 33, 9, 2, 4, 7, 5, 0, 0, 0, 0, 0, 0, 0])
    at += (32 + 9 + 8 + 3) // 4 * 4
    # I420 3 x 7: luma 3 rows of 7, U 2 rows of 4, V 2 rows of 4
    rows.append([at, 7, at + 21, at + 29, 4, 1, 3, 7, 0, 0, 1, 1, 1, 0, 0, 0])
    at += (21 + 8 + 8 + 3) // 4 * 4
    # NV21 4 x 2: luma 4 rows of 5 (2 live), chroma 2 rows of 2
    rows.append([at, 5, at + 18, at + 17, 2, 2, 4, 2, 8, 1, 0, 0, 0, 0, 0, 0])
    at += (17 + 4 + 3) // 4 * 4
    words = [np.asarray(rows, dtype=np.int32).reshape(-1)]
    for n_in, out in [(w, S_W) for w in ws] + [(h, S_H) for h in hs]:
        first, k = _coeffs(n_in, out)
        words += [np.asarray([n_in, out, 0, 0], dtype=np.int32), first, k.reshape(-1)]
    words += [np.asarray([*BT601, 0, 0, *BT709F, 0, 0], dtype=np.int32)]
    return np.ascontiguousarray(np.concatenate(words), dtype=np.int32), len(rows), len(ws), len(hs), 2, at


def _check(lib, tab, K, nh, nv, nc, src_bytes, n_words=None, F_=F, Sh=S_H, Sw=S_W):
    rc = lib.tady_ingest_plan_check(tab.ctypes.data, tab.size if n_words is None else n_words, K, nh, nv, nc, src_bytes, F_, Sh, Sw)
    return rc, lib.tady_last_error_string()


def test_a_well_formed_plan_passes(lib):
    tab, K, nh, nv, nc, nbytes = good_plan()
    rc, msg = _check(lib, tab, K, nh, nv, nc, nbytes)
    assert rc == 0, msg
    assert tab.size == K * _lib.YUV_ROW_WORDS + nh * SET_H + nv * SET_V + nc * _lib.YUV_CSET_WORDS
    # the last plane may end on the last byte of src: the NV21 frame's chroma ends at its offset + 17 + 2 + 2 = 21 of 24
    r = tab[2 * _lib.YUV_ROW_WORDS:3 * _lib.YUV_ROW_WORDS]
    assert _check(lib, tab, K, nh, nv, nc, int(r[0]) + 21)[0] == 0


def test_every_plan_check_refusal_names_its_argument_or_row(lib):
    tab0, K, nh, nv, nc, nbytes = good_plan()
    R, HS = _lib.YUV_ROW_WORDS, K * _lib.YUV_ROW_WORDS
    VS = HS + nh * SET_H
    CS = VS + nv * SET_V
    end2 = int(tab0[2 * R]) + 21  # one past the last live byte of the last frame

    def refused(what, edit=None, **kw):
        tab = tab0.copy()
        if edit is not None:
            edit(tab)
        rc, msg = _check(lib, tab, kw.pop("K", K), kw.pop("nh", nh), kw.pop("nv", nv), kw.pop("nc", nc), kw.pop("src_bytes", nbytes), **kw)
        assert rc == -1 and what.encode() in msg and msg.startswith(b"ingest_plan_check: "), (what, rc, msg)

    def word(i, v):
        return lambda t: t.__setitem__(i, v)

    def words(*pairs):
        def edit(t):
            for i, v in pairs:
                t[i] = v
        return edit

    # the scalars and the word count
    refused("K=0 must be in", K=0)
    refused(f"K={_lib.YUV_MAX_FRAMES + 1} must be in", K=_lib.YUV_MAX_FRAMES + 1)
    refused("n_hsets=0 must be in", nh=0)
    refused("n_vsets=65 must be in", nv=65)
    refused("n_csets=0 must be in", nc=0)
    refused(f"n_csets={_lib.YUV_MAX_CSETS + 1} must be in", nc=_lib.YUV_MAX_CSETS + 1)
    refused("S_h=0 must be in", Sh=0)
    refused("S_w=16385 must be in", Sw=16385)
    refused("F=0 must be in", F_=0)
    refused("src_bytes=0 must be positive", src_bytes=0)
    refused(f"n_words={tab0.size - 1}, expected", n_words=tab0.size - 1)
    refused(f"n_words={tab0.size + 8}, expected", n_words=tab0.size + 8)
    rc = lib.tady_ingest_plan_check(None, 10, K, nh, nv, nc, nbytes, F, S_H, S_W)
    assert rc == -1 and b"table_host is null" in lib.tady_last_error_string()
    # the extents
    refused("row 1: h=0 outside", word(1 * R + 6, 0))
    refused("row 2: w=-3 outside", word(2 * R + 7, -3))
    refused(f"row 0: h={_lib.YUV_MAX_EXTENT + 1} outside", word(6, _lib.YUV_MAX_EXTENT + 1))
    # each plane outside src
    refused("row 2: the U plane's bytes", src_bytes=end2 - 1)            # (NV21: V is the first byte of a pair, U the last byte of the frame)
    refused("row 2: the V plane's bytes", src_bytes=end2 - 1, edit=words((2 * R + 2, int(tab0[2 * R + 3])), (2 * R + 3, int(tab0[2 * R + 2]))))
    refused("row 0: the luma plane's bytes", word(0, nbytes - 20))
    refused("row 1: the luma plane's bytes", word(1 * R, -1))
    refused("row 1: the U plane's bytes", word(1 * R + 2, nbytes - 4))
    refused("row 1: the V plane's bytes", word(1 * R + 3, -8))
    refused("row 0: the U plane's bytes", words((2, nbytes), (3, nbytes + 1)))
    # a pitch below the row's live bytes
    refused("row 0: y_pitch=6 is below the 7 live bytes of a luma row", word(1, 6))
    refused("row 0: c_pitch=7 is below the 8 live bytes of a chroma row", word(4, 7))
    refused("row 1: c_pitch=3 is below the 4 live bytes of a chroma row", word(1 * R + 4, 3))
    refused("row 2: y_pitch=-5 is below", word(2 * R + 1, -5))
    # c_step
    refused("row 0: c_step=0 must be 1", word(5, 0))
    refused("row 1: c_step=3 must be 1", word(1 * R + 5, 3))
    # interleaved chroma whose halves are not next to each other
    refused("row 0: interleaved chroma (c_step=2) with u_off=40 and v_off=42 not next to each other", word(3, 42))
    refused("row 2: interleaved chroma (c_step=2) with u_off=", word(2 * R + 2, int(tab0[2 * R + 3])))
    # the slot
    refused(f"row 0: slot={F} outside the store", word(8, F))
    refused("row 2: slot=-1 outside the store", word(2 * R + 8, -1))
    refused("row 2: slot=5 is already named by row 0", word(2 * R + 8, 5))
    refused("row 0: slot=5 outside the store", F_=5)
    # the set indices, and a set not stated for the row's extent
    refused(f"row 0: hset={nh} outside", word(9, nh))
    refused("row 1: vset=-1 outside", word(1 * R + 10, -1))
    refused(f"row 1: cset={nc} outside", word(1 * R + 11, nc))
    refused("row 2: cset=-1 outside", word(2 * R + 11, -1))
    refused("row 2: its hset 0 is stated for 7 columns, the frame has w=2", word(2 * R + 9, 0))
    refused("row 1: its vset 0 is stated for 4 rows, the frame has h=3", word(1 * R + 10, 0))
    refused("horizontal set 1: output extent 4, expected 5", word(HS + SET_H + 1, 4))
    refused("horizontal set 0: output 2 has its first tap at -3", word(HS + _lib.FR_SET_HEAD + 2, -3))
    refused("vertical set 1: output 0 has its first tap at 2", word(VS + SET_V + _lib.FR_SET_HEAD, 2))

    def heavy(t):
        t[VS + _lib.FR_SET_HEAD + S_H + 4:VS + _lib.FR_SET_HEAD + S_H + 8] = (-385, 1600, 834, 0)
    refused(f"vertical set 0: output 1: sum |k| = 2819 is above {_lib.FR_MAX_ABS_SUM}", heavy)
    # unknown flag bits, the reserved words
    refused("row 1: flags=0x3 holds unknown bits", word(1 * R + 12, 3))
    refused("row 0: flags=0x80000000 holds unknown bits", word(12, -2 ** 31))
    refused("row 2: word 13 is 1", word(2 * R + 13, 1))
    refused("row 0: word 15 is -2", word(15, -2))
    refused("colour set 1: words 6 and 7 are 0 and 9", word(CS + 8 + 7, 9))
    # the colour sets: the int32 bound (255 * 2^20 + 128 * 14684160 + 2^19 = 2^31), the offset, a negative luma gain
    refused("colour set 1: 255 * cy + 128 * max|c| + 2^19 = 2147483648 reaches 2^31", word(CS + 8 + 2, 14684160))
    refused("colour set 1: 255 * cy + 128 * max|c| + 2^19 = 2147483648 reaches 2^31", word(CS + 8 + 5, -14684160))
    refused("colour set 0: 255 * cy + 128 * max|c| + 2^19 =", words((CS + 3, -(2 ** 30)), (CS + 4, 2 ** 30)))
    refused("colour set 0: y_off=256 outside [0, 255]", word(CS, 256))
    refused("colour set 0: cy=-1 is negative", word(CS + 1, -1))
    tab = tab0.copy()
    tab[CS + 8 + 2] = 14684159  # one below: 2^31 - 128 passes
    assert _check(lib, tab, K, nh, nv, nc, nbytes)[0] == 0


# ---------------------------------------------------------------- the launching entry point: refusals only
def P(item):
    return ("ptr", item)


CASE = dict(src=P(4), src_bytes=4096, store=P(1), F=F, table=P(4), n_words=3 * 16 + 2 * SET_H + 2 * SET_V + 2 * 8, K=3, n_hsets=2,
            n_vsets=2, n_csets=2, S_h=S_H, S_w=S_W, stream=None)

_BUF = ctypes.create_string_buffer(32 * 4096)
_BASE = (ctypes.addressof(_BUF) + 4095) // 4096 * 4096


def _addr(k, off=0):
    return ctypes.c_void_p(_BASE + k * 4096 + off)


def _call(lib, shift=None, **override):
    sym = "tady_ingest_yuv"
    names = prototypes()[sym]
    assert list(CASE) == names, (list(CASE), names)
    args = []
    for k, n in enumerate(names):
        v = override.get(n, CASE[n])
        if isinstance(v, tuple) and v[0] == "ptr":
            v = _addr(k, shift[1] if shift and shift[0] == n else 0)
        args.append(v)
    rc = getattr(lib, sym)(*args)
    return rc, lib.tady_last_error_string()


def test_misaligned_pointer_is_refused_by_name(lib):
    """every 4-byte row at every offset below 4; store, which has no requirement, is never what a refusal names"""
    refused = 0
    for name, row in CONTRACT["tady_ingest_yuv"].items():
        if row is ANY:
            continue
        pat = re.compile(rf"\b{re.escape(name)} is misaligned.*\b{row.n}-byte aligned".encode())
        for off in (1, 2, 3):
            rc, msg = _call(lib, shift=(name, off))
            assert rc == -1, f"{name} + {off}: rc = {rc} ({msg})"
            assert pat.search(msg) and msg.startswith(b"ingest_yuv"), f"{name} + {off} was refused for another reason: {msg}"
            refused += 1
    assert refused == 6
    for off in (1, 2, 3):
        rc, msg = _call(lib, shift=("store", off), K=0)
        assert rc == -1 and b"K=0" in msg and b"misaligned" not in msg


def test_host_validation_without_gpu(lib):
    def refused(what, **override):
        rc, msg = _call(lib, **override)
        assert rc == -1 and what.encode() in msg and msg.startswith(b"ingest_yuv: "), (override, rc, msg)

    for n in ("src", "store", "table"):
        refused(f"{n} is null", **{n: None})
    refused("K=0 must be in", K=0)
    refused(f"K={_lib.YUV_MAX_FRAMES + 1} must be in", K=_lib.YUV_MAX_FRAMES + 1)
    refused("n_hsets=0 must be in", n_hsets=0)
    refused("n_vsets=65 must be in", n_vsets=65)
    refused("n_csets=17 must be in", n_csets=17)
    refused("S_h=-1 must be in", S_h=-1)
    refused("S_w=0 must be in", S_w=0)
    refused("F=0 must be in", F=0)
    refused("src_bytes=-8 must be positive", src_bytes=-8)
    refused(f"n_words={CASE['n_words'] + 1}, expected", n_words=CASE["n_words"] + 1)
    # the other libraries' error texts are their own
    first, serve, recon, bank = _lib.load(), _lib.load_serve(), _lib.load_recon(), _lib.load_bank()
    before = (first.tad_last_error_string(), serve.tads_last_error_string(), recon.tadr_last_error_string(), bank.tadb_last_error_string())
    refused("src is null", src=None)
    assert (first.tad_last_error_string(), serve.tads_last_error_string(), recon.tadr_last_error_string(), bank.tadb_last_error_string()) == before
