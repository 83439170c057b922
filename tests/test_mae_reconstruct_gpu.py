"""tadr_mae_reconstruct (csrc/mae_reconstruct.hip; include/tad_mi355x_recon.h) at the smallest shapes at which the lane passes, the
ragged tail and the grid arithmetic can go wrong, against the fp64 restatement of tests/reconstruct_ref.py (oracle.vit_oracle.mae_target
and its algebraic inverse).  Nothing outside the repository is read.

  (tub, p, T, H, W)      why
  (2, 16, 4, 32, 48)     Hp != Wp, 12 tokens, 512 pixels (the NPIX = 8 instance)
  (1, 14, 2, 28, 42)     196 pixels: three full lane passes plus four lanes; 42-byte rows that start at every address mod 4
  (1,  2, 2,  4,  6)     4 pixels: one partial pass; 6-byte rows
  (1, 32, 1, 32, 64)     1024 pixels: the limit (NPIX = 16)
  (2, 16, 2, 16, 16)     one token, n_mask in {0, 1}
B in {1, 3}; masks differ per clip at equal count, n_mask in {1, 3N/4, N-1, N}; both normalize_target settings; sources: random uint8,
two adjacent grey levels, constant patches, each through the frames_to_clip formula (u / 255 - mean) / std.  A case (its source, clip,
mask, slot table, random prediction and fp64 reference) is built once per module and never written."""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch

import reconstruct_ref as RR
from edge_cases import ulp32
from guarded import GuardedArena, same_bits

pytestmark = pytest.mark.gpu

SHAPES = [(2, 16, 4, 32, 48), (1, 14, 2, 28, 42), (1, 2, 2, 4, 6), (1, 32, 1, 32, 64), (2, 16, 2, 16, 16)]
KINDS = ("random", "two_grey", "constant")
MEAN, STD = RR.MEAN, RR.STD


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import _lib, kernels
    _lib.load()
    return kernels


def n_tokens(shape):
    tub, p, T, H, W = shape
    return (T // tub) * (H // p) * (W // p)


def mask_counts(N):
    return [0, 1] if N == 1 else sorted({1, max(1, (3 * N) // 4), N - 1, N})


@functools.lru_cache(maxsize=None)
def case(shape, B, n_mask, kind):
    """source frames, the clip, a mask per clip, the slot table and a random prediction ~ N(0, 1): host tensors, built once"""
    tub, p, T, H, W = shape
    N = n_tokens(shape)
    g = torch.Generator().manual_seed(1000 * sum(shape) + 100 * B + 10 * n_mask + KINDS.index(kind))
    u8 = RR.source(kind, B, tub, p, T, H, W, g)
    mask = RR.random_masks(B, N, n_mask, g)
    pred = torch.randn(B, n_mask, tub * p * p * 3, generator=g) if n_mask else None
    if B > 1 and 0 < n_mask < N and N > 2:
        assert not torch.equal(mask[0], mask[1]), "masks differ per clip"
    mask_tok = torch.stack([mask[b].nonzero().flatten() for b in range(B)]).to(torch.int32)  # ascending: token_indices' order
    return SimpleNamespace(shape=shape, B=B, N=N, n_mask=n_mask, kind=kind, u8=u8, videos=RR.frames_to_clip_formula(u8), mask=mask,
                           slot=RR.slot_of(mask), mask_tok=mask_tok, pred=pred)


def cases(shape):
    N = n_tokens(shape)
    return [case(shape, B, n, kind) for B in (1, 3) for n in mask_counts(N) for kind in KINDS]


@functools.lru_cache(maxsize=None)
def ref64(shape, B, n_mask, kind, norm):
    c = case(shape, B, n_mask, kind)
    tub, p = shape[:2]
    return RR.reconstruct_ref(c.videos.double(), c.pred, c.slot, tub, p, normalize_target=norm)


def run(K, c, pred, norm, slot=None, **kw):
    tub, p = c.shape[:2]
    frames, err = K.mae_reconstruct(c.videos.cuda(), None if pred is None else pred.cuda(), (c.slot if slot is None else slot).cuda(),
                                    tub, p, MEAN, STD, norm, **kw)
    return (None if frames is None else frames.cpu()), (None if err is None else err.cpu())


# =============================================================================================== 1. the round trip, exact
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_round_trip_gives_the_source_back_byte_for_byte(K, shape):
    """pred = kernels.mae_target(...) of the masked tokens and visible_gain = 1: frames equal the source uint8 in EVERY byte, masked and
    visible; err is exactly 0 at visible tokens and at most 1e-10 at masked ones.  Derivation: the composition of the target and its
    inverse is off by a few f32 ulps of a value in [0, 1] (6e-8 each), the rounding margin is 0.5 / 255 = 2e-3; a constant patch
    has s = 1e-6 and labels of exactly 0, so r = m.  Measured on MI355X: no byte differs in any case."""
    tub, p = shape[:2]
    for c in cases(shape):
        for norm in (True, False):
            pred = None
            if c.n_mask:
                pred = K.mae_target(c.videos.cuda(), c.mask_tok.cuda().reshape(-1), tub, p, MEAN, STD, norm)
            frames, err = run(K, c, pred, norm)
            bad = int((frames != c.u8).sum())
            assert frames.shape == c.u8.shape and bad == 0, (shape, c.B, c.n_mask, c.kind, norm, f"{bad} bytes differ")
            assert err.shape == (c.B, c.N) and not bool(err[~c.mask].any()), "err is exactly 0 at visible tokens"
            worst = float(err[c.mask].max()) if c.n_mask else 0.0
            assert worst <= 1e-10, (shape, c.B, c.n_mask, c.kind, norm, worst)


# =============================================================================================== 2. bytes of a random prediction
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_random_prediction_bytes_against_fp64(K, shape):
    """pred ~ N(0, 1): a byte equals the fp64 byte unless the fp64 value X = 255 r lies within
    delta = 255 * 8 * 2^-24 * (|pred| (s + 1e-6) + |m| + 1) of a half-integer (s, m: the patch's deviation and mean; s + 1e-6 = 1, m = 0
    without normalize_target; at a visible token the value is 255 v and |v| stands for the first two terms); inside that band it may
    differ by 1; a difference of more than 1 fails anywhere; the share of elements inside the band is at most 2e-3 over the cases of a
    shape (the band is a property of the fp64 values alone: 1.5e-4 to 4.4e-4 of these inputs lie inside it; on MI355X at most 2 bytes per
    shape actually differ)."""
    tub, p, T, H, W = shape
    in_band, total, differ = 0, 0, 0
    for c in cases(shape):
        for norm in (True, False):
            frames, _ = run(K, c, c.pred, norm)
            ref = ref64(shape, c.B, c.n_mask, c.kind, norm)
            mag = torch.where(ref.masked[:, :, None, None], ref.rows.abs() * ref.scale + ref.centre.abs(), ref.v.abs())
            delta = RR.tokens_to_frames(255.0 * 8.0 * 2.0 ** -24 * (mag + 1.0), tub, p, T, H, W)
            X = ref.value
            band = (X - torch.floor(X) - 0.5).abs() <= delta
            diff = (frames.to(torch.int16) - RR.to_byte(X).to(torch.int16)).abs()
            assert int(diff.max()) <= 1, (shape, c.B, c.n_mask, c.kind, norm, "a byte is off by more than 1")
            outside = int((diff[~band] != 0).sum())
            assert outside == 0, (shape, c.B, c.n_mask, c.kind, norm, f"{outside} bytes differ outside the rounding band")
            in_band, total, differ = in_band + int(band.sum()), total + band.numel(), differ + int((diff != 0).sum())
    print(f"\nmae_reconstruct {shape}: {in_band} of {total} elements inside the band ({in_band / total:.2e}), {differ} bytes differ by 1")
    assert in_band <= 2e-3 * total, (shape, in_band, total)


# =============================================================================================== 3. the error map
KAPPA = 8.0   # two-grey-level bound: relative error of a standardised value in units of 2^-23 (below)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_error_map_against_fp64(K, shape):
    """err per masked token against fp64.  The project's yardstick: |err - ref| <= 4 x max(the error of torch's own f32 evaluation of the
    same expression on the same device, 8 f32 ulps of ref).

    On the two-grey-level source under normalize_target torch's one-float mean makes its own error meaningless as a yardstick (DESIGN.md
    section 4), so the kernel is held to fp64 directly there, by a first-order bound: a standardised value t = (v - m) / (s + 1e-6) of
    a two-level patch carries at most KAPPA = 8 roundings of 2^-23 max|t| (the residual against the refined two-float mean: about two
    ulps of the level gap, i.e. up to 6 x 2^-23 of a value of half the gap; the variance, the root, the sum with 1e-6, the division
    and the product one each of 2^-24), so |err - ref| <= 2 KAPPA 2^-23 mean|pred - t| max|t|; to that come the sum's own roundings --
    a chain of at most 16 additions per lane, 6 butterfly steps, 2 across the channels, the division, the square and the difference:
    fewer than 32, each at most 2^-24 of the total.

    mean(err over the masked tokens) against tad_mse_loss on kernels.mae_target's labels: within (B n_mask + tub p p 3) 2^-24 relative --
    both are fixed-order f32 sums of that many terms.  Visible tokens: exactly 0.

    Measured on MI355X (printed per shape): worst |err - ref| / max(torch f32 error, 8 ulp) 0.321, 0.316, 0.312, 0.254, 0.169 over the five
    shapes (bound 4); two grey levels, worst |err - ref| / direct bound 0.050, 0.056, 0.037, 0.048, 0.022 (bound 1)."""
    tub, p = shape[:2]
    nent = tub * p * p * 3
    worst_ratio, worst_direct = 0.0, 0.0
    for c in cases(shape):
        if not c.n_mask:
            continue
        for norm in (True, False):
            _, err = run(K, c, c.pred, norm)
            ref = ref64(shape, c.B, c.n_mask, c.kind, norm)
            assert not bool(err[~c.mask].any())
            got, want = err.double()[c.mask], ref.err[c.mask]
            e = (got - want).abs()
            if c.kind == "two_grey" and norm:
                target = (ref.v - ref.centre) / ref.scale
                mean_d = (ref.rows - target).abs().mean(dim=(2, 3))[c.mask]
                bound = 2.0 * KAPPA * 2.0 ** -23 * mean_d * target.abs().amax(dim=(2, 3))[c.mask] + 32.0 * 2.0 ** -24 * want
                worst_direct = max(worst_direct, float((e / bound).max()))
            else:
                t32 = RR.reconstruct_ref(c.videos.cuda(), c.pred.cuda(), c.slot.cuda(), tub, p, normalize_target=norm).err.cpu()
                assert t32.dtype == torch.float32
                bound = 4.0 * torch.maximum((t32.double()[c.mask] - want).abs(), 8.0 * ulp32(want))
                worst_ratio = max(worst_ratio, float((e / (bound / 4.0)).max()))
            assert bool((e <= bound).all()), (shape, c.B, c.n_mask, c.kind, norm, float((e / bound).max()))
            # the loss of the same batch
            labels = K.mae_target(c.videos.cuda(), c.mask_tok.cuda().reshape(-1), tub, p, MEAN, STD, norm)
            loss, _ = K.mse_loss(c.pred.cuda().reshape(-1, nent).contiguous(), labels.reshape(-1, nent), want_grad=False)
            a, b = float(got.mean()), float(loss.double())
            assert abs(a - b) <= (c.B * c.n_mask + nent) * 2.0 ** -24 * abs(b), (shape, c.B, c.n_mask, c.kind, norm, a, b)
    print(f"\nmae_reconstruct err {shape}: worst |err - ref| / max(torch f32 error, 8 ulp) = {worst_ratio:.3f} (bound 4); "
          f"two grey levels, worst |err - ref| / direct bound = {worst_direct:.3f} (bound 1)")


# =============================================================================================== 4. written once, nothing else touched
def _c_call(lib_mod, videos, pred, slot, frames, err, c, norm, gain=1.0):
    tub, p, T, H, W = c.shape
    f3 = lambda v: (ctypes.c_float * 3)(*v)  # noqa: E731
    rc = lib_mod.load_recon().tadr_mae_reconstruct(videos.data_ptr(), None if pred is None else pred.data_ptr(), slot.data_ptr(),
                                                    None if frames is None else frames.data_ptr(), None if err is None else err.data_ptr(),
                                                    c.B, c.n_mask, T, H, W, tub, p, f3(MEAN), f3(STD), int(norm), gain,
                                                    torch.cuda.current_stream().cuda_stream)
    lib_mod.check_recon(rc, "tadr_mae_reconstruct")


@pytest.mark.parametrize("shape", SHAPES[:4], ids=str)
def test_every_output_element_is_written_once_and_nothing_else(K, shape):
    """frames pre-filled with 0xA5 (then 0x5A) and err with NaN come back fully overwritten: the two pre-fills give the same bits, equal
    to the plain call's.  The operands sit in the guard-band arena: no byte outside frames and err changes, under NaN and under huge
    poison, with frames at every address mod 4 (the word / byte split of a row follows the address; the bytes do not).  Two runs give the
    same bits."""
    from simple_tad_amd import _lib
    N = n_tokens(shape)
    c = case(shape, 3, max(1, (3 * N) // 4), "random")
    arena = GuardedArena(32 << 20, "cuda")
    for norm in (True, False):
        plain = run(K, c, c.pred, norm)
        again = run(K, c, c.pred, norm)
        assert torch.equal(plain[0], again[0]) and same_bits(plain[1], again[1]), "two runs, the same bits"
        for poison in ("nan", "huge"):
            for off, fill in ((0, 0xA5), (1, 0x5A), (2, 0xA5), (3, 0x5A)):
                arena.reset(poison)
                videos = arena.place(c.videos, role="input", name="videos")
                pred = arena.place(c.pred, role="input", name="pred")
                slot = arena.place(c.slot, role="input", name="slot", index_range=c.n_mask)
                frames = arena.place(tuple(c.u8.shape), torch.uint8, role="output", name="frames", fill=fill, offset=off)
                err = arena.place((c.B, c.N), torch.float32, role="output", name="err")
                assert bool(torch.isnan(err).all()) and frames.data_ptr() % 4 == off
                _c_call(_lib, videos, pred, slot, frames, err, c, norm)
                arena.verify()
                assert torch.equal(frames.cpu(), plain[0]), (shape, norm, poison, off)
                assert same_bits(err.cpu(), plain[1]), (shape, norm, poison, off)


# =============================================================================================== 5. / 6. clips and slots
def test_a_clip_reads_only_its_own_rows_of_pred(K):
    """B = 3: NaN in clip 1's prediction leaves clips 0 and 2 identical in frames and err; clip 1's masked bytes are 0 (NaN -> 0), its
    masked errors NaN, its visible bytes and zeros what they were"""
    shape = SHAPES[0]
    c = case(shape, 3, 9, "random")
    tub, p, T, H, W = shape
    for norm in (True, False):
        base_f, base_e = run(K, c, c.pred, norm)
        pred = c.pred.clone()
        pred[1] = float("nan")
        f, e = run(K, c, pred, norm)
        for b in (0, 2):
            assert torch.equal(f[b], base_f[b]) and same_bits(e[b], base_e[b]), (norm, b)
        tok_masked = RR.tokens_to_frames(c.mask[:, :, None, None].expand(3, c.N, tub * p * p, 3).contiguous(), tub, p, T, H, W)[1]
        assert not bool(f[1][tok_masked].any()), "NaN gives byte 0"
        assert torch.equal(f[1][~tok_masked], base_f[1][~tok_masked])
        assert bool(torch.isnan(e[1][c.mask[1]]).all()) and not bool(e[1][~c.mask[1]].any())
    # +inf -> 255, -inf -> 0 (normalize_target off: r = pred)
    pred = c.pred.clone()
    pred[1, :, 0::2], pred[1, :, 1::2] = float("inf"), float("-inf")
    f, _ = run(K, c, pred, False)
    want = RR.to_byte(RR.reconstruct_ref(c.videos.double(), pred, c.slot, tub, p, normalize_target=False).value)
    assert torch.equal(f[1], want[1]) and set(f[1][tok_masked].unique().tolist()) == {0, 255}
    assert torch.equal(f[0], base_f[0]) and torch.equal(f[2], base_f[2])


def test_a_slot_outside_the_range_counts_as_visible(K):
    """slot = n_mask + 5 and slot = -7 (B = 3): those tokens come back as visible ones -- the source's bytes, err 0 -- and every other
    token is what it was"""
    shape = SHAPES[0]
    c = case(shape, 3, 9, "random")
    tub, p, T, H, W = shape
    slot = c.slot.clone()
    t1, t2 = int(c.mask[1].nonzero()[0]), int(c.mask[2].nonzero()[-1])
    slot[1, t1], slot[2, t2] = c.n_mask + 5, -7
    for norm in (True, False):
        base_f, base_e = run(K, c, c.pred, norm)
        f, e = run(K, c, c.pred, norm, slot=slot)
        changed = torch.zeros(3, c.N, dtype=torch.bool)
        changed[1, t1] = changed[2, t2] = True
        px = RR.tokens_to_frames(changed[:, :, None, None].expand(3, c.N, tub * p * p, 3).contiguous(), tub, p, T, H, W)
        assert torch.equal(f[px], c.u8[px]) and torch.equal(f[~px], base_f[~px])
        assert not bool(e[changed].any()) and same_bits(e[~changed], base_e[~changed])
        want = RR.reconstruct_ref(c.videos.double(), c.pred, slot, tub, p, normalize_target=norm)
        assert torch.equal(want.masked, c.mask & ~changed)


# =============================================================================================== 7. visible_gain
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1]], ids=str)
def test_visible_gain_dims_the_visible_patches_only(K, shape):
    """visible_gain = 0.5: a visible byte is rint(0.5 * 255 * v) by the f32 formula -- v = fma(videos, std, mean), one product with
    127.5, halves to even: for an odd source level the product sits ON a half-integer up to v's last bits, so this holds the kernel
    to its stated arithmetic bit for bit -- and the masked bytes are the ones of visible_gain = 1"""
    tub, p, T, H, W = shape
    for kind in ("random", "two_grey"):
        c = case(shape, 3, 9, kind)
        v = RR.tokens_to_frames(RR.patchify(RR.unnormalise_fused_f32(c.videos), tub, p), tub, p, T, H, W)
        assert v.dtype == torch.float32
        want = RR.to_byte(torch.tensor(127.5, dtype=torch.float32) * v)
        px = RR.tokens_to_frames(c.mask[:, :, None, None].expand(3, c.N, tub * p * p, 3).contiguous(), tub, p, T, H, W)
        for norm in (True, False):
            full, e1 = run(K, c, c.pred, norm)
            half, e2 = run(K, c, c.pred, norm, visible_gain=0.5)
            assert torch.equal(half[~px], want[~px]), (shape, kind, norm, int((half[~px] != want[~px]).sum()))
            assert torch.equal(half[px], full[px]) and same_bits(e1, e2)
    from simple_tad_amd._lib import TadError
    with pytest.raises(TadError, match=r"visible_gain=1.25 outside \[0, 1\]"):
        run(K, c, c.pred, True, visible_gain=1.25)


# =============================================================================================== 8. nullable outputs
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_frames_only_and_err_only_give_the_same_bits(K, shape):
    N = n_tokens(shape)
    for n_mask in mask_counts(N):
        c = case(shape, 3, n_mask, "random")
        for norm in (True, False):
            f, e = run(K, c, c.pred, norm)
            f_only, none_e = run(K, c, c.pred, norm, want_err=False)
            none_f, e_only = run(K, c, c.pred, norm, want_frames=False)
            assert none_e is None and none_f is None
            assert torch.equal(f, f_only) and same_bits(e, e_only), (shape, n_mask, norm)
    from simple_tad_amd._lib import TadError
    with pytest.raises(TadError, match="neither frames nor err"):
        run(K, c, c.pred, True, want_frames=False, want_err=False)
