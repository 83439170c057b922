"""The launch selector of the 16-bit attention kernels (csrc/attn_plan.hip; tad_attn_plan, kernels.attn_plan): which kernel instantiation a
tad_attn_fwd / tad_attn_bwd call runs is a pure host function of the call's contract and the knobs, so every combination is checked here
without a GPU against the rule as include/tad_mi355x.h words it (restated in expected_fwd / expected_bwd below)."""
import ctypes
import itertools

import pytest

KNOBS = ("dma_mode", "fwd_q64", "drop_skip")


@pytest.fixture(scope="module")
def K():
    from simple_tad_amd import _lib, build, kernels
    build.build(verbose=False)
    _lib.load()
    return kernels


@pytest.fixture
def knobs(K):
    """knobs(**kv): tad_attn_tuning; what was found is put back afterwards"""
    found = {k: K.attn_tuning_get(k) for k in KNOBS}
    yield lambda **kv: K.attn_tuning(**kv)
    K.attn_tuning(**found)


def grid_of(B, N, H):
    return -(-N // 128) * H * B


def expected_fwd(B, N, H, d, out16, qs, drop, clip, lo, drop_skip, fwd_q64):
    from simple_tad_amd._lib import ATTN_FWD, ATTN_FWD_Q64
    contract = d == 64 and qs and not drop and out16  # the production contract of the training step
    if fwd_q64 and contract:  # taken before the fill route; ignores the clip scale
        return dict(kernel=ATTN_FWD_Q64, hd=64, out16=1, qs=1, drop=0, dma_mode=0, skip=0, has_lo=int(lo), grid=grid_of(B, N, H), block=128)
    skip = bool(clip and drop_skip and contract)
    return dict(kernel=ATTN_FWD, hd=d, out16=int(out16), qs=int(qs), drop=int(drop), dma_mode=0, skip=int(skip), has_lo=0, grid=grid_of(B, N, H), block=256)


def expected_bwd(B, N, H, d, qs, drop, clip, drop_skip):
    from simple_tad_amd._lib import ATTN_BWD_DKV, ATTN_BWD_DQ
    skip = bool(clip and drop_skip and d == 64 and qs and not drop)  # the forward's conditions except the output type; fwd_q64 plays no part
    row = dict(hd=d, out16=1, qs=int(qs), drop=int(drop), dma_mode=0, skip=int(skip), has_lo=0, grid=grid_of(B, N, H), block=256)
    return [dict(kernel=ATTN_BWD_DQ, **row), dict(kernel=ATTN_BWD_DKV, **row)]


CONTRACTS = list(itertools.product((64, 80), (False, True), (False, True), (0.0, 0.1), (False, True), (False, True)))  # d, out16, qs, dropout, clip, out_lo


@pytest.mark.parametrize("drop_skip,fwd_q64", list(itertools.product((0, 1), (0, 1))))
def test_every_contract_plans_the_record_the_rule_gives(K, knobs, drop_skip, fwd_q64):
    from simple_tad_amd import _lib
    knobs(drop_skip=drop_skip, fwd_q64=fwd_q64)
    B, H = 2, 3
    seen = set()
    for (d, out16, qs, p, clip, lo), N in itertools.product(CONTRACTS, (1, 128, 129)):
        call = dict(d=d, out_16bit=out16, q_prescaled=qs, drop_p=p, rowscale=clip, out_lo=lo)
        if lo and not out16:  # the rounding residual goes with a 16-bit output: refused as by tad_attn_fwd
            with pytest.raises(_lib.TadError, match="out_lo"):
                K.attn_plan(B, N, H, **call)
        else:
            rows = K.attn_plan(B, N, H, **call)
            assert rows == [expected_fwd(B, N, H, d, out16, qs, p > 0, clip, lo, drop_skip, fwd_q64)], call
            seen.add((rows[0]["kernel"], rows[0]["skip"]))
        rows = K.attn_plan(B, N, H, backward=True, **call)
        assert rows == expected_bwd(B, N, H, d, qs, p > 0, clip, drop_skip), call
        assert len(rows) == 2 and all(rows[0][f] == rows[1][f] for f in ("hd", "qs", "drop", "skip"))
    assert seen == {(_lib.ATTN_FWD, 0)} | ({(_lib.ATTN_FWD_Q64, 0)} if fwd_q64 else {(_lib.ATTN_FWD, 1)} if drop_skip else set())
    assert (K.attn_tuning_get("drop_skip"), K.attn_tuning_get("fwd_q64"), K.attn_tuning_get("dma_mode")) == (drop_skip, fwd_q64, 0)  # planning sets nothing


def test_plan_rows_follow_the_enospace_protocol(K):
    from simple_tad_amd import _lib
    lib = _lib.load()
    assert len(_lib.ATTN_PLAN_FIELDS) == 10
    buf = (ctypes.c_int32 * 20)()
    assert lib.tad_attn_plan(0, 1, 8, 1, 64, 1, 1, 0.0, 0, 0, buf, 1) == 1
    assert lib.tad_attn_plan(1, 1, 8, 1, 64, 1, 1, 0.0, 0, 0, buf, 1) == -3 and b"room for 1" in lib.tad_last_error_string()
    assert lib.tad_attn_plan(1, 1, 8, 1, 64, 1, 1, 0.0, 0, 0, buf, 2) == 2
    assert lib.tad_attn_plan(1, 1, 8, 1, 64, 1, 1, 0.0, 0, 0, None, 2) == -1 and b"null" in lib.tad_last_error_string()


def test_ablation_modes_are_refused_by_a_production_build(K, knobs):
    from simple_tad_amd import _lib
    for mode in (1, 2, 3):
        with pytest.raises(_lib.TadError, match="dma_mode"):
            knobs(dma_mode=mode)
    knobs(dma_mode=0)
    assert K.attn_tuning_get("dma_mode") == 0
    with pytest.raises(_lib.TadError, match="fwd_q64"):
        knobs(fwd_q64=2)
    with pytest.raises(_lib.TadError, match="unknown key"):
        knobs(no_such_knob=1)


def test_limits_are_refused_with_the_entry_points_messages(K):
    from simple_tad_amd import _lib

    def refused(match, *shape, **call):
        with pytest.raises(_lib.TadError, match=match):
            K.attn_plan(*shape, **call)
    for backward in (False, True):
        refused("head_dim", 1, 8, 1, d=32, backward=backward)
        refused("bad shape", 65536, 8, 1, backward=backward)
        refused("bad shape", 1, 8, 65536, backward=backward)
        refused("bad shape", 1, 0, 1, backward=backward)
        refused(r"outside \[0, 1\)", 1, 8, 1, drop_p=1.0, backward=backward)
        # 1024 clips of 4096 tokens x 16 heads: 24 GiB of qkv behind one buffer descriptor
        refused("4 GiB buffer descriptor", 1024, 4096, 16, backward=backward)
    # 65535 x 65535 x 2 rows do not fit the 32-bit row index of the dropout mask (without dropout the same shape fails on its size)
    refused("dropout mask's row index", 65535, 2, 65535, drop_p=0.1)
    refused("4 GiB buffer descriptor", 65535, 2, 65535)
    refused("row-constant descriptor", 65535, 1, 65535, backward=True)
    # the same refusals reach the entry points themselves (no launch: they come first)
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.tad_attn_fwd(p, p, 1, None, None, None, 1024, 4096, 16, 64, 0.125, 1, 0.0, 0, None) == -1
    assert b"4 GiB buffer descriptor" in lib.tad_last_error_string()
    assert lib.tad_attn_bwd(p, p, None, p, p, None, p, p, 65535, 1, 65535, 64, 0.125, 1, 0.0, 0, None) == -1
    assert b"row-constant descriptor" in lib.tad_last_error_string()
