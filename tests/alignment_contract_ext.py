"""The pointer alignment contract of the extension ABI (include/tad_mi355x_ext.h, "Pointer alignment"), as data.  No GPU use.

The rows use the classes of tests/alignment_contract.py (A / ANY / HOST) and follow its rules: one row per entry point of
simple_tad_amd._lib.EXT_SIGNATURES and per ``c_void_p`` argument except the stream, named as the header's prototype names it.
tests/test_iv2_abi_cpu.py fails when a symbol or a pointer argument has no row here, and refuses every A(n) row at every
element-aligned offset below n.
"""
import ctypes
import os
import re

from alignment_contract import A, ANY
from simple_tad_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tad_mi355x_ext.h")

CONTRACT = {
    # ---- csrc/rmsnorm.hip: float4 rows, gammas, gamma gradients and partials; 8-byte pieces of 16-bit rows; the row statistics one float at a time
    "tadx_rmsnorm_fwd": dict(x=A(16), gamma=A(16), y=A(16, **{"16-bit y_dtype": 8}), rrms=ANY),
    "tadx_rmsnorm_bwd": dict(dy=A(16, **{"16-bit dy_dtype": 8}), x=A(16), gamma=A(16), rrms=ANY, dres=A(16), dx=A(16), dx16=A(8), dgamma=A(16),
                             ws=A(16)),
    "tadx_qk_rmsnorm_fwd": dict(qkv32=A(16), gq=A(16), gk=A(16), qkv16=A(8), rr=ANY),
    "tadx_qk_rmsnorm_bwd": dict(dqkv16=A(8), qkv32=A(16), gq=A(16), gk=A(16), rr=ANY, dqkv_pre16=A(8), dgq=A(16), dgk=A(16), ws=A(16)),
}


def prototypes():
    """{symbol: [argument names]} as include/tad_mi355x_ext.h declares them"""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(tadx_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        params = m.group(2).strip()
        out[m.group(1)] = [] if params in ("", "void") else [re.findall(r"[A-Za-z_0-9]+", p)[-1] for p in params.split(",")]
    return out


def pointer_arguments(symbol, protos=None):
    """[(position, name)] of the ``c_void_p`` arguments of ``symbol`` except the stream"""
    names = (protos or prototypes())[symbol]
    args = _lib.EXT_SIGNATURES[symbol][1]
    assert len(names) == len(args), f"{symbol}: the header declares {len(names)} arguments, the binding {len(args)}"
    return [(i, names[i]) for i, a in enumerate(args) if a is ctypes.c_void_p and names[i] != "stream"]
