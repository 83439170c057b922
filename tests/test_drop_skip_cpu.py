"""Host side of the stochastic-depth fill (tad_attn_drop_scale, tad_attn_tuning "drop_skip"): argument checks run before any launch, so
they are testable without a GPU."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from simple_tad_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_drop_scale_is_per_clip_and_consumed_by_the_next_attention_call(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.tad_attn_drop_scale(p, 0) == -1 and b"rows_per_scale" in lib.tad_last_error_string()
    # one scale per clip: rows_per_scale must be the sequence length of the call that takes it
    assert lib.tad_attn_drop_scale(p, 5) == 0
    assert lib.tad_attn_fwd(p, p, 1, None, None, 1, 8, 1, 64, 0.125, 1, 0.0, 0, None) == -1
    assert b"rows_per_scale must be N=8" in lib.tad_last_error_string()
    # ... and that call consumed it: the next one fails for its own reason (head_dim), not for a scale left behind
    assert lib.tad_attn_fwd(p, p, 1, None, None, 1, 8, 1, 32, 0.125, 1, 0.0, 0, None) == -1
    assert b"head_dim" in lib.tad_last_error_string()
    assert lib.tad_attn_drop_scale(p, 5) == 0
    assert lib.tad_attn_bwd_f16(p, p, None, p, p, p, p, 1, 8, 1, 64, 0.125, 1, 0.0, 0, None) == -1
    assert b"rows_per_scale must be N=8" in lib.tad_last_error_string()
    assert lib.tad_attn_bwd(p, p, None, p, p, p, p, 1, 8, 1, 32, 0.125, 1, 0.0, 0, None) == -1
    assert b"head_dim" in lib.tad_last_error_string()
    # NULL clears a pending setting
    assert lib.tad_attn_drop_scale(p, 5) == 0 and lib.tad_attn_drop_scale(None, 0) == 0
    assert lib.tad_attn_fwd(p, p, 1, None, None, 1, 8, 1, 32, 0.125, 1, 0.0, 0, None) == -1
    assert b"head_dim" in lib.tad_last_error_string()


def test_drop_skip_knob(lib):
    assert lib.tad_attn_tuning(b"drop_skip", 2) == -1 and b"drop_skip" in lib.tad_last_error_string()
    assert lib.tad_attn_tuning(b"drop_skip", 0) == 0
    assert lib.tad_attn_tuning(b"drop_skip", 1) == 0
