"""MAE reconstruction without a GPU: the fp64 restatement the GPU tests measure against (tests/reconstruct_ref.py) is the algebraic
inverse of oracle.vit_oracle.mae_target -- which tests/test_pretrain.py pins to the reference's recorded labels -- the slot table is the
inverse of token_indices, and the Python layer refuses a model that is not on the device with the family's own message."""
from functools import partial

import pytest
import torch

import reconstruct_ref as RR
from oracle import vit_oracle as O

SHAPES = [(2, 16, 4, 32, 48), (1, 14, 2, 28, 42), (1, 2, 2, 4, 6), (1, 32, 1, 32, 64), (2, 16, 2, 16, 16)]  # (tub, p, T, H, W)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("kind", ["random", "two_grey"])
def test_the_restatement_inverts_the_oracle_target(shape, kind):
    """pred = O.mae_target(...) in fp64: 255 r is 255 v to 1e-9 at every pixel, masked or visible, and the error map is 0 -- with and
    without normalize_target, for masks that differ per clip.  (Constant patches are left to the kernel's tests: in fp64 their labels
    are rounding noise over 1e-6, and so is the inverse.)"""
    tub, p, T, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    B = 3
    N = (T // tub) * (H // p) * (W // p)
    u8 = RR.source(kind, B, tub, p, T, H, W, g)
    videos = RR.frames_to_clip_formula(u8).double()
    for n_mask in sorted({1, max(1, (3 * N) // 4), max(1, N - 1), N}):
        mask = RR.random_masks(B, N, n_mask, g)
        slot = RR.slot_of(mask)
        for norm in (True, False):
            pred = O.mae_target(videos, mask, tubelet=tub, patch=p, normalize_target=norm)
            ref = RR.reconstruct_ref(videos, pred, slot, tub, p, normalize_target=norm)
            want = 255.0 * RR.tokens_to_frames(RR.patchify(RR.unnormalise(videos), tub, p), tub, p, T, H, W)
            assert ref.value.shape == (B, T, H, W, 3) and float((ref.value - want).abs().max()) <= 1e-9, (shape, kind, n_mask, norm)
            assert float(ref.err.abs().max()) <= 1e-20 and torch.equal(ref.masked, mask)
            assert torch.equal(RR.to_byte(ref.value), u8), "the fp64 bytes are the source's"


def test_layout_helpers_are_inverse_and_follow_the_oracle_cut():
    tub, p, T, H, W = 2, 4, 4, 8, 12
    x = torch.arange(2 * 3 * T * H * W, dtype=torch.float64).reshape(2, 3, T, H, W)
    tok = RR.patchify(x, tub, p)
    every = torch.ones(2, tok.shape[1], dtype=torch.bool)
    raw = O.mae_target(x, every, tubelet=tub, patch=p, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), normalize_target=False)
    assert torch.equal(tok.reshape(2, tok.shape[1], -1), raw)
    assert torch.equal(RR.tokens_to_frames(tok, tub, p, T, H, W), x.permute(0, 2, 3, 4, 1))


def test_the_byte_rule():
    x = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.4, 0.5, 1.5, 2.5, 254.5, 255.5, 300.0, 127.49999])
    assert RR.to_byte(x).tolist() == [0, 255, 0, 0, 0, 2, 2, 254, 255, 255, 127]


def test_slot_table_is_the_inverse_of_token_indices():
    """slot[b, mask_tok[b, j]] == j, -1 at every visible token, int32, for bool and float masks, with the count given or read"""
    from simple_tad_amd.modeling_pretrain import slot_table, token_indices
    g = torch.Generator().manual_seed(5)
    for B, N, n_mask in ((1, 1, 1), (3, 12, 9), (2, 12, 1), (2, 12, 11), (2, 7, 7)):
        mask = RR.random_masks(B, N, n_mask, g)
        for m in (mask, mask.float()):
            for given in (n_mask, None):
                slot, mask_tok = slot_table(m, given)
                vis_tok, want_tok = token_indices(m, given)
                assert slot.dtype == torch.int32 and slot.shape == (B, N) and torch.equal(mask_tok, want_tok)
                assert torch.equal(slot, RR.slot_of(mask))
                for b in range(B):
                    assert slot[b, mask_tok[b].long()].tolist() == list(range(n_mask))
                    assert bool((slot[b, vis_tok[b].long()] == -1).all())


def test_reconstruct_refuses_a_cpu_model_with_the_familys_message():
    import simple_tad_amd as T
    import simple_tad_amd.internvideo2_pretrain as IVP
    import simple_tad_amd.modeling_pretrain as MP
    import iv2_pretrain_recipe as PR
    from simple_tad_amd._lib import TadError
    norm = partial(torch.nn.LayerNorm, eps=1e-6)
    vmae = MP.PretrainVisionTransformer(img_size=32, patch_size=16, encoder_embed_dim=128, encoder_depth=1, encoder_num_heads=2,
                                        decoder_num_classes=1536, decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=1, norm_layer=norm)
    iv2 = IVP.PretrainVideoMAEInternVideo2(norm_layer=norm, **PR.TINY)
    from simple_tad_amd.reconstruct import model_patch_geometry
    assert model_patch_geometry(vmae) == (16, 2) and model_patch_geometry(iv2) == (14, 1)
    for m, x, who in ((vmae, torch.zeros(2, 3, 16, 32, 32), "PretrainVisionTransformer"), (iv2, PR.clip(), "PretrainVideoMAEInternVideo2")):
        N = m.encoder.patch_embed.num_patches
        mask = RR.random_masks(2, N, (3 * N) // 4, torch.Generator().manual_seed(1))
        m.train()
        with pytest.raises(TadError, match=rf"{who}: input is on cpu; the MI355X path runs HIP kernels only"):
            T.reconstruct(m, x, mask)
        assert m.training, "the mode is put back when the call fails, too"
        with pytest.raises(ValueError, match=r"reconstruct: the clips of this batch mask different numbers of tokens"):
            bad = mask.clone()
            bad[1] = False
            T.reconstruct(m, x, bad)
        with pytest.raises(ValueError, match=r"reconstruct: the mask has \d+ tokens per clip"):
            T.reconstruct(m, x, torch.cat([mask, torch.zeros(2, 1, dtype=torch.bool)], dim=1))


def test_public_surface():
    import inspect
    import simple_tad_amd as T
    from simple_tad_amd import engine_pretrain as EP, explain, kernels
    assert {"reconstruct", "error_to_frames", "evaluate_one_epoch"} <= set(T.__all__)
    assert T.evaluate_one_epoch is EP.evaluate_one_epoch
    assert list(inspect.signature(EP.evaluate_one_epoch).parameters) == ["model", "data_loader", "device", "patch_size", "normlize_target",
                                                                         "tubelet_size", "augment_fn"]
    sig = inspect.signature(T.reconstruct)
    assert list(sig.parameters) == ["model", "clips", "mask", "normlize_target", "visible_gain", "mean", "std"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[3:])
    assert list(inspect.signature(kernels.mae_reconstruct).parameters) == ["videos", "pred", "slot", "tubelet", "patch", "mean", "std",
                                                                           "normalize_target", "visible_gain", "want_frames", "want_err"]
    e = torch.arange(24.0).reshape(1, 2, 3, 4)
    assert torch.equal(T.error_to_frames(e, (4, 6, 8)), explain.saliency_to_frames(e, (4, 6, 8)))
    assert torch.equal(T.error_to_frames(e, (4, 6, 8), "bilinear"), explain.saliency_to_frames(e, (4, 6, 8), "bilinear"))
