"""Argument validation of the pooled-tail entry points (tad_colsum_segments, tad_gelu_grad_bcast): the checks run before any launch,
so they are testable without a GPU.  Every refusal is TAD_EINVAL (-1) with a message that names the entry point."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from simple_tad_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _ptr(offset=0):
    buf = ctypes.create_string_buffer(4096 + 64)
    base = ctypes.addressof(buf)
    return buf, ctypes.c_void_p((base + 63) // 64 * 64 + offset)


def _refused(lib, rc, word, entry):
    msg = lib.tad_last_error_string()
    assert rc == -1 and msg and entry in msg and word in msg, (rc, msg)


def test_colsum_segments_validation(lib):
    from simple_tad_amd._lib import TAD_BF16, TAD_F16
    keep, p = _ptr()
    keep2, odd = _ptr(2)
    call = lib.tad_colsum_segments
    e = b"colsum_segments"
    for args in ((None, TAD_BF16, p, p, 1 << 20, 2, 4, 64, None), (p, TAD_BF16, None, p, 1 << 20, 2, 4, 64, None),
                 (p, TAD_F16, p, None, 1 << 20, 2, 4, 64, None)):
        _refused(lib, call(*args), b"null", e)
    for K in (4, 60, 66):
        _refused(lib, call(p, TAD_BF16, p, p, 1 << 20, 2, 4, K, None), b"multiple of 8", e)
    for B, N in ((0, 4), (-1, 4), (2, 0), (2, -3)):
        _refused(lib, call(p, TAD_F16, p, p, 1 << 20, B, N, 64, None), b"bad shape", e)
    for args in ((odd, TAD_BF16, p, p, 1 << 20, 2, 4, 64, None), (p, TAD_BF16, odd, p, 1 << 20, 2, 4, 64, None),
                 (p, TAD_BF16, p, odd, 1 << 20, 2, 4, 64, None)):
        _refused(lib, call(*args), b"misaligned", e)
    _refused(lib, call(p, 0, p, p, 1 << 20, 2, 4, 64, None), b"op_dtype", e)  # TAD_F32 is not a 16-bit operand format
    assert call(p, TAD_BF16, p, p, 2 * 8 * 64 * 4 - 1, 2, 4, 64, None) == -3 and b"workspace" in lib.tad_last_error_string()


def test_gelu_grad_bcast_validation(lib):
    from simple_tad_amd._lib import TAD_BF16, TAD_F16
    keep, p = _ptr()
    keep2, odd = _ptr(8)
    call = lib.tad_gelu_grad_bcast
    e = b"gelu_grad_bcast"
    for args in ((None, p, p, TAD_BF16, 2, 4, 64, None), (p, None, p, TAD_BF16, 2, 4, 64, None), (p, p, None, TAD_F16, 2, 4, 64, None)):
        _refused(lib, call(*args), b"null", e)
    for K in (4, 60, 66):
        _refused(lib, call(p, p, p, TAD_F16, 2, 4, K, None), b"multiple of 8", e)
    for B, N in ((0, 4), (-1, 4), (2, 0), (2, -3)):
        _refused(lib, call(p, p, p, TAD_BF16, B, N, 64, None), b"bad shape", e)
    for args in ((odd, p, p, TAD_BF16, 2, 4, 64, None), (p, odd, p, TAD_BF16, 2, 4, 64, None), (p, p, odd, TAD_BF16, 2, 4, 64, None)):
        _refused(lib, call(*args), b"misaligned", e)
    _refused(lib, call(p, p, p, 0, 2, 4, 64, None), b"op_dtype", e)


def test_pooled_linear_validation(lib):
    from simple_tad_amd._lib import TAD_BF16, TAD_F16
    keep, p = _ptr()
    keep1, q = _ptr()
    keep2, odd = _ptr(8)
    call = lib.tad_pooled_linear
    e = b"pooled_linear"
    for args in ((None, p, TAD_BF16, p, p, p, q, 2, 4, 16, 64, None), (p, None, TAD_BF16, p, p, p, q, 2, 4, 16, 64, None),
                 (p, p, TAD_F16, p, p, None, q, 2, 4, 16, 64, None), (p, p, TAD_F16, p, p, p, None, 2, 4, 16, 64, None)):
        _refused(lib, call(*args), b"null", e)
    for K in (4, 60, 66):
        _refused(lib, call(p, p, TAD_F16, None, None, p, q, 2, 4, 16, K, None), b"multiple of 8", e)
    for B, N, D in ((0, 4, 16), (2, 0, 16), (2, -3, 16), (2, 4, 0)):
        _refused(lib, call(p, p, TAD_BF16, None, None, p, q, B, N, D, 64, None), b"bad shape", e)
    for args in ((odd, p, TAD_BF16, None, None, p, q, 2, 4, 16, 64, None), (p, odd, TAD_BF16, None, None, p, q, 2, 4, 16, 64, None)):
        _refused(lib, call(*args), b"misaligned", e)
    _refused(lib, call(p, p, 0, None, None, p, q, 2, 4, 16, 64, None), b"op_dtype", e)
    _refused(lib, call(p, p, TAD_BF16, None, None, p, p, 2, 4, 16, 64, None), b"alias", e)


def test_switch_and_shape_gate():
    from simple_tad_amd import kernels as K, ops
    assert K.colsum_segments_ok(3072) and not K.colsum_segments_ok(3076)
    old = ops.get_pooled_tail()
    try:
        ops.set_pooled_tail(False)
        assert ops.get_pooled_tail() is False
        ops.set_pooled_tail(True)
        assert ops.get_pooled_tail() is True
    finally:
        ops.set_pooled_tail(old)
