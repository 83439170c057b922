"""tad_im2col_tubelets_16: the patch matrix of a clip that already is in a 16-bit operand format -- a move of 16-bit words.

Reference: a torch restatement of the layout, x.view(B,C,T',tub,H',p,W',p).permute(0,2,4,6,1,3,5,7) with zero padding up to ldk, compared
as int16 views, bit for bit.  The clip cycles through all 65 536 bit patterns (NaN payloads, infinities and subnormals of both formats
must arrive unchanged); cols is pre-filled with a non-zero pattern so that an unwritten padding column shows.

Shapes: the smallest that reach each path (C = 3): one wide item per patch row (p = 8) at one and at three clips; 16-pixel patches; the
smallest pairs case; p = 14 (K = 1176 -> ldk = 1216: padded columns exactly zero); and 2 x 16 x 224^2, whose 602 112 wide items exceed
the 524 288 threads of the capped grid (the grid-stride loop runs a second time for some threads only)."""
import pytest
import torch

from guarded import GuardedArena, same_bits

pytestmark = pytest.mark.gpu

FMTS = {"bf16": torch.bfloat16, "f16": torch.float16}
#        patch tub T   H    W   B
SHAPES = [(8, 2, 4, 8, 16, 1), (8, 2, 4, 8, 16, 3), (16, 2, 4, 32, 32, 1), (2, 1, 1, 2, 4, 2), (14, 2, 2, 14, 28, 2), (16, 2, 16, 224, 224, 2)]
IDS = ["wide8-B1", "wide8-B3", "wide16", "pairs2", "pairs14", "gridstride"]
FILL = 0x5A5A


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import _lib, kernels
    _lib.load()
    return kernels


@pytest.fixture(scope="module")
def arena():
    return GuardedArena(64 << 20, "cuda")


def pattern_clip(B, T, H, W, dtype, nan=True):
    """[B,3,T,H,W] of ``dtype`` whose words walk through all 65 536 bit patterns (257 is odd), starting at the largest finite bf16 so
    that even the 48-word case holds infinities and NaNs; ``nan=False``: the NaN patterns of the format are replaced by finite ones"""
    n = B * 3 * T * H * W
    w = (torch.arange(n, dtype=torch.int64) * 257 + 0x7F7F) & 0xFFFF
    x = (w - ((w >= 0x8000).to(torch.int64) << 16)).to(torch.int16).view(dtype)  # (as a signed word)
    if not nan:
        x = torch.where(torch.isnan(x), torch.ones_like(x), x)
    return x.view(B, 3, T, H, W)


def layout_reference(x, tub, p, ldk):
    """the patch matrix as int16 [B*N, ldk] (the one statement of the layout: csrc/im2col.hip PatchGrid)"""
    B, C, T, H, W = x.shape
    cols = x.view(torch.int16).view(B, C, T // tub, tub, H // p, p, W // p, p).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(-1, C * tub * p * p)
    return torch.nn.functional.pad(cols, (0, ldk - cols.shape[1]))


@pytest.fixture(scope="module")
def references():
    """one reference per (shape, format), computed once on the host and left unchanged"""
    cache = {}

    def get(K, shape, fmt):
        if (shape, fmt) not in cache:
            p, tub, T, H, W, B = shape
            x = pattern_clip(B, T, H, W, FMTS[fmt])
            cache[(shape, fmt)] = (x, layout_reference(x, tub, p, K.patch_embed_ldk(3, tub, p)))
        return cache[(shape, fmt)]
    return get


@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_moves_every_bit_pattern(K, references, shape, fmt):
    """the C entry point on a cols pre-filled with 0x5A5A: every word of cols is written -- the clip's, or zero in the padding"""
    from simple_tad_amd import _lib
    p, tub, T, H, W, B = shape
    x, ref = references(K, shape, fmt)
    assert ref.shape[1] == {14: 1216, 2: 64}.get(p, 3 * tub * p * p)  # ldk: K rounded up to the GEMM's K-tile; K itself for p % 8 == 0
    xd = x.cuda()
    cols = torch.full(ref.shape, FILL, dtype=torch.int16, device="cuda")
    _lib.check(_lib.load().tad_im2col_tubelets_16(xd.data_ptr(), cols.data_ptr(), B, 3, T, H, W, tub, p, torch.cuda.current_stream().cuda_stream),
               "tad_im2col_tubelets_16")
    got = cols.cpu()
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {ref.numel()} words differ"
    if p == 14:
        assert not got[:, 1176:].any() and bool((ref[:, :1176] != 0).any())
    # the wrapper: the same matrix, in the clip's format
    out = K.im2col_tubelets_16(xd, tub, p)
    assert out.dtype == FMTS[fmt] and torch.equal(out.view(torch.int16).cpu(), ref)


@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_guard_bands(K, arena, references, shape, fmt, poison):
    """clip and patch matrix between poisoned guard bands in one allocation: no store outside cols (verify), and no word of the result
    depends on bytes outside x (cols is born NaN, the guards hold NaN / the largest finite value: the reference holds neither by chance,
    it is compared bit for bit)"""
    p, tub, T, H, W, B = shape
    x, ref = references(K, shape, fmt)
    arena.reset(poison)
    xa = arena.place(x, name="x")
    with arena.route(K):
        cols = K.im2col_tubelets_16(xa, tub, p)
    arena.verify()
    assert arena.contains(cols), "the wrapper allocated cols outside the arena"
    assert torch.equal(cols.view(torch.int16).cpu(), ref)


@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("shape", SHAPES[:5], ids=IDS[:5])
def test_same_bits_as_the_f32_route(K, shape, fmt):
    """the kernel this route replaces as a second reference: K.im2col_tubelets on the upcast clip, rounding back to the same format.
    Input: every bit pattern that is not a NaN -- the upcast of a 16-bit value to f32 is exact (infinities and subnormals included) and
    rounding an exactly representable value returns it, so the two routes must agree in every bit; a NaN may come back quieted from
    the two conversions (IEEE 754 allows it), which is the one thing the move does differently and test_moves_every_bit_pattern pins."""
    p, tub, T, H, W, B = shape
    op = FMTS[fmt]
    x = pattern_clip(B, T, H, W, op, nan=False).cuda()
    got = K.im2col_tubelets_16(x, tub, p)
    old = K.im2col_tubelets(x.float(), tub, p, dtype=op)
    assert same_bits(got, old), f"{int((got.view(torch.int16) != old.view(torch.int16)).sum())} words differ"


def test_misaligned_view_returns_none(K):
    """a view whose address the loads cannot take: the wrapper answers None (the caller falls back), it does not raise"""
    n = 2 * 3 * 2 * 16 * 16
    buf = torch.zeros(n + 16, dtype=torch.bfloat16, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = lambda off, H, W: buf[off:off + 2 * 3 * 2 * H * W].view(2, 3, 2, H, W)
    assert K.im2col_tubelets_16(view(1, 16, 16), 2, 8) is None     # 2 bytes off: neither decomposition
    assert K.im2col_tubelets_16(view(1, 12, 12), 2, 6) is None
    assert K.im2col_tubelets_16(view(4, 16, 16), 2, 8) is None     # 8 bytes off: not the 16-byte loads of wide items
    x = pattern_clip(2, 2, 12, 12, torch.bfloat16)
    v = view(4, 12, 12)
    v.copy_(x)
    got = K.im2col_tubelets_16(v, 2, 6)                            # ... but the 4-byte loads of pairs
    assert got is not None and torch.equal(got.view(torch.int16).cpu(), layout_reference(x, 2, 6, K.patch_embed_ldk(3, 2, 6)))
    assert K.im2col_tubelets_16(view(0, 16, 16), 2, 8) is not None
