"""Host side of the stochastic-depth fill (the clip_scale argument of tad_attn_fwd / tad_attn_bwd, tad_attn_tuning "drop_skip"): argument
checks and the kernel selection run before any launch, so they are testable without a GPU."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from simple_tad_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_clip_scale_is_an_argument_and_leaves_no_state_behind(lib):
    """The scale used to be parked in thread-local state by a call of its own, with a rows_per_scale that had to equal N; the "rows_per_scale
    must be N" check went with that parameter -- a [B] operand has no second way to be shaped.  What remains to pin down: every entry point
    takes the argument in front of its usual validation, and a call with a scale changes nothing for the call behind it."""
    from simple_tad_amd import kernels as K
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    # all four entry points accept a non-null clip_scale and still refuse head_dim 32 first
    for fwd in (lib.tad_attn_fwd, lib.tad_attn_fwd_f16):
        assert fwd(p, p, 1, None, None, p, 1, 8, 1, 32, 0.125, 1, 0.0, 0, None) == -1
        assert b"head_dim" in lib.tad_last_error_string()
    for bwd in (lib.tad_attn_bwd, lib.tad_attn_bwd_f16):
        assert bwd(p, p, None, p, p, p, p, p, 1, 8, 1, 32, 0.125, 1, 0.0, 0, None) == -1
        assert b"head_dim" in lib.tad_last_error_string()
    # stateless: a call with a scale selects the fill kernels, the next one without a scale does not ...
    contract = dict(d=64, out_16bit=True, q_prescaled=True)
    for backward in (False, True):
        assert all(r["skip"] == 1 for r in K.attn_plan(2, 8, 1, backward=backward, rowscale=True, **contract))
        assert all(r["skip"] == 0 for r in K.attn_plan(2, 8, 1, backward=backward, rowscale=False, **contract))
    # ... and the next entry-point call without one fails for its own reason
    assert lib.tad_attn_fwd(p, p, 1, None, None, None, 1, 8, 1, 32, 0.125, 1, 0.0, 0, None) == -1
    assert b"head_dim" in lib.tad_last_error_string()


def test_drop_skip_knob(lib):
    v = ctypes.c_int(-1)
    assert lib.tad_attn_tuning_get(b"drop_skip", ctypes.byref(v)) == 0
    found = v.value
    try:
        assert lib.tad_attn_tuning(b"drop_skip", 2) == -1 and b"drop_skip" in lib.tad_last_error_string()
        assert lib.tad_attn_tuning(b"drop_skip", 0) == 0
        assert lib.tad_attn_tuning_get(b"drop_skip", ctypes.byref(v)) == 0 and v.value == 0
        assert lib.tad_attn_tuning(b"drop_skip", 1) == 0
        assert lib.tad_attn_tuning_get(b"drop_skip", ctypes.byref(v)) == 0 and v.value == 1
        assert lib.tad_attn_tuning_get(b"no_such_knob", ctypes.byref(v)) == -1 and b"unknown key" in lib.tad_last_error_string()
    finally:
        assert lib.tad_attn_tuning(b"drop_skip", found) == 0
