"""The entry kernels of the InternVideo2 encoder (csrc/iv2_serve.hip: tads_class_token_entry_fwd / _bwd) at every shape where they can go
wrong: one float4 per row (D 4), widths that are no multiple of 256 (252, 260), more than one block, one and several clips, one patch
token.  Forward: the bits of ``cat`` + add.  Backward: dpatch the bits of g[:, 1:]; dpos / dcls the bits of the f32 loop over the clips
(tests/iv2_serve_ref.py) and within (B - 1) 2^-24 sum_b |g| of the fp64 sum per element -- B - 1 additions, each rounding a partial sum
whose magnitude sum_b |g| bounds."""
import pytest
import torch

import guarded
import iv2_serve_ref as S

pytestmark = pytest.mark.gpu

BS = [1, 2, 3, 5]
NS = [1, 2, 8, 257]
DS = [4, 128, 252, 256, 260, 1280, 1408]


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import _lib, kernels
    _lib.load()
    return kernels


def operands(B, N, D):
    g = torch.Generator().manual_seed(1000 * B + 10 * N + D)
    return tuple(torch.randn(s, generator=g).cuda() for s in ((B, N, D), (D,), (N + 1, D), (B, N + 1, D)))


@pytest.mark.parametrize("D", DS)
def test_forward_and_backward_at_every_shape(K, D):
    for B in BS:
        for N in NS:
            patch, cls, pos, go = operands(B, N, D)
            what = f"B {B} N {N} D {D}"
            out = K.class_token_entry_fwd(patch, cls, pos)
            assert out.shape == (B, N + 1, D) and out.dtype == torch.float32
            assert torch.equal(out, torch.cat((cls.reshape(1, 1, D).expand(B, -1, -1), patch), 1) + pos), what
            assert guarded.same_bits(out, S.entry_fwd(patch, cls, pos)), what
            assert guarded.same_bits(K.class_token_entry_fwd(patch, cls, pos), out), f"{what}: not reproducible"
            dpatch, dpos, dcls = K.class_token_entry_bwd(go)
            r_patch, r_pos, r_cls = S.entry_bwd(go)
            assert guarded.same_bits(dpatch, go[:, 1:].contiguous()) and guarded.same_bits(dpatch, r_patch), what
            assert guarded.same_bits(dpos, r_pos) and guarded.same_bits(dcls, r_cls), f"{what}: not the f32 loop over the clips"
            s64 = go.double().sum(0)
            lim = (B - 1) * 2.0 ** -24 * go.double().abs().sum(0)
            assert ((dpos.double() - s64).abs() <= lim).all() and ((dcls.double() - s64[0]).abs() <= lim[0]).all(), what
            again = K.class_token_entry_bwd(go)
            assert all(guarded.same_bits(a, b) for a, b in zip(again, (dpatch, dpos, dcls))), f"{what}: not reproducible"


@pytest.mark.parametrize("B,N,D", [(1, 1, 4), (3, 8, 260), (5, 257, 128)])
def test_nullable_outputs_and_accumulation(K, B, N, D):
    _, _, _, go = operands(B, N, D)
    dpatch, dpos, dcls = K.class_token_entry_bwd(go)
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True), (False, True, True)):
        got = K.class_token_entry_bwd(go, want_dpatch=want[0], want_dpos=want[1], want_dcls=want[2])
        for w, a, b in zip(want, got, (dpatch, dpos, dcls)):
            assert (a is None) if not w else guarded.same_bits(a, b), want
    # accumulate adds the finished sums into the sinks (flat views, as the optimizer's buffers are), one more add each
    seed_p, seed_c = torch.linspace(-1, 1, (N + 1) * D).cuda(), torch.linspace(2, 3, D).cuda()
    sp, sc = seed_p.clone(), seed_c.clone()
    got = K.class_token_entry_bwd(go, into_pos=sp, into_cls=sc)
    assert got[1] is sp and got[2] is sc and guarded.same_bits(got[0], dpatch)
    assert guarded.same_bits(sp, seed_p + dpos.reshape(-1)) and guarded.same_bits(sc, seed_c + dcls)
    sp = seed_p.clone()
    got = K.class_token_entry_bwd(go, want_dpatch=False, want_dcls=False, into_pos=sp)
    assert got[0] is None and got[2] is None and guarded.same_bits(sp, seed_p + dpos.reshape(-1))
    sc = seed_c.clone()
    got = K.class_token_entry_bwd(go, want_dpatch=False, want_dpos=False, into_cls=sc)
    assert got[0] is None and got[1] is None and guarded.same_bits(sc, seed_c + dcls)
    from simple_tad_amd._lib import TadError
    with pytest.raises(TadError, match="both a sink or neither"):
        K.class_token_entry_bwd(go, into_pos=seed_p.clone())
    with pytest.raises(TadError, match="all null"):
        K.class_token_entry_bwd(go, want_dpatch=False, want_dpos=False, want_dcls=False)


@pytest.mark.parametrize("poison", guarded.POISON_MODES)
@pytest.mark.parametrize("B,N,D", [(1, 1, 4), (3, 8, 260), (2, 257, 1408)])
def test_inside_poisoned_guard_bands(K, poison, B, N, D):
    patch, cls, pos, go = operands(B, N, D)
    out = K.class_token_entry_fwd(patch, cls, pos)
    dpatch, dpos, dcls = K.class_token_entry_bwd(go)
    seed_p, seed_c = torch.linspace(-1, 1, (N + 1) * D).cuda(), torch.linspace(2, 3, D).cuda()
    arena = guarded.GuardedArena(64 << 20, "cuda", poison=poison)
    pa, ca, sa, ga = (arena.place(t, role="input") for t in (patch, cls, pos, go))
    sink_p, sink_c = arena.place(seed_p, role="inout"), arena.place(seed_c, role="inout")
    with arena.route(K):
        g_out = K.class_token_entry_fwd(pa, ca, sa)
        g_all = K.class_token_entry_bwd(ga)
        g_patch_only = K.class_token_entry_bwd(ga, want_dpos=False, want_dcls=False)[0]
        g_cls_only = K.class_token_entry_bwd(ga, want_dpatch=False, want_dpos=False)[2]
        K.class_token_entry_bwd(ga, want_dpatch=False, into_pos=sink_p, into_cls=sink_c)
    arena.verify()
    for got, want in ((g_out, out), (g_all[0], dpatch), (g_all[1], dpos), (g_all[2], dcls), (g_patch_only, dpatch), (g_cls_only, dcls),
                      (sink_p, seed_p + dpos.reshape(-1)), (sink_c, seed_c + dcls)):
        assert arena.contains(got) and guarded.same_bits(got, want)
