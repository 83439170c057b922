"""simple_tad_amd.reconstruct and engine_pretrain.evaluate_one_epoch on the tiny VideoMAE pre-training model of tests/test_pretrain.py
and the tiny InternVideo2 one of tests/iv2_pretrain_recipe.py: the dict is what its parts are when they are computed one by one --
the model's own prediction, the training step's loss, the clip's own bytes where a patch is visible and the kernel's bytes where it is
masked -- bit for bit, and the held-out pass is the mean of its batches' losses and touches no parameter."""
from functools import partial

import pytest
import torch

import iv2_pretrain_recipe as PR
import iv2_recipe as IR
import reconstruct_ref as RR
import simple_tad_amd as T
from guarded import same_bits

pytestmark = pytest.mark.gpu


def videomae(golden):
    from test_pretrain import setup
    _, _, m, P, _, mask = setup(golden)
    m.load_state_dict(P)
    return m.cuda(), mask, (16, 32, 32), 16, 2


def internvideo2(golden):
    import simple_tad_amd.internvideo2_pretrain as IVP
    torch.manual_seed(0)
    m = IVP.PretrainVideoMAEInternVideo2(norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), **PR.TINY)
    IR.perturb_(m.named_parameters())
    return m.cuda(), PR.mask(), (4, 28, 28), 14, 1


FAMILIES = {"videomae": videomae, "internvideo2": internvideo2}


def clips_for(size, B, seed):
    """uint8 frames [B,T,H,W,3] and the normalised f32 clip a loader makes of them"""
    u8 = torch.randint(0, 256, (B, *size, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return u8, RR.frames_to_clip_formula(u8)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_reconstruct_is_its_parts_bit_for_bit(golden, family):
    from simple_tad_amd import kernels as K, ops
    from simple_tad_amd.engine_pretrain import reconstruction_target
    m, mask, size, patch, tub = FAMILIES[family](golden)
    u8, x = clips_for(size, mask.shape[0], 3)
    x = x.cuda()
    grid = (size[0] // tub, size[1] // patch, size[2] // patch)
    for training in (True, False):
        m.train(training)
        out = T.reconstruct(m, x, mask)
        assert m.training is training, "the model's mode is put back"
        assert set(out) == {"frames", "error", "pred", "loss", "mask_grid"}
        m.eval()
        with torch.no_grad():
            pred = m(x, mask.cuda())
            loss = ops.MseLossFn.apply(pred, reconstruction_target(x, mask.cuda(), patch, tub, True))
        assert same_bits(out["pred"], pred) and not out["pred"].requires_grad
        assert same_bits(out["loss"], loss), (float(out["loss"]), float(loss))
        assert out["mask_grid"].dtype == torch.bool and torch.equal(out["mask_grid"].cpu(), mask.reshape(-1, *grid))
        frames, err = K.mae_reconstruct(x, pred, RR.slot_of(mask).cuda(), tub, patch, RR.MEAN, RR.STD, True)
        assert out["frames"].dtype == torch.uint8 and out["frames"].shape == u8.shape and torch.equal(out["frames"], frames)
        assert out["error"].shape == (mask.shape[0], *grid) and same_bits(out["error"].reshape(err.shape), err)
        px = RR.tokens_to_frames(mask[:, :, None, None].expand(*mask.shape, tub * patch * patch, 3).contiguous(), tub, patch, *size)
        got = out["frames"].cpu()
        assert torch.equal(got[~px], u8[~px]), "visible patches are the source's bytes"
        assert not torch.equal(got[px], u8[px]), "masked patches are the prediction, not the source"
        assert not bool(out["error"].cpu()[~out["mask_grid"].cpu()].any()) and bool((out["error"].cpu()[out["mask_grid"].cpu()] > 0).all())
        # the error map as a heat map on the frames
        heat = T.error_to_frames(out["error"], size)
        assert heat.shape == (mask.shape[0], *size)
    # the training loss of the same batch (train mode, gradients on) has the same bits: these models carry no dropout
    m.train()
    loss_train = ops.MseLossFn.apply(m(x, mask.cuda()), reconstruction_target(x, mask.cuda(), patch, tub, True))
    assert same_bits(loss_train.detach(), out["loss"])
    # without normlize_target the frames are the raw prediction and the loss the raw loss
    raw = T.reconstruct(m, x, mask, normlize_target=False, visible_gain=0.5)
    with torch.no_grad():
        want = ops.MseLossFn.apply(raw["pred"], reconstruction_target(x, mask.cuda(), patch, tub, False))
    assert same_bits(raw["loss"], want) and same_bits(raw["pred"], pred)
    frames, _ = K.mae_reconstruct(x, pred, RR.slot_of(mask).cuda(), tub, patch, RR.MEAN, RR.STD, False, visible_gain=0.5)
    assert torch.equal(raw["frames"], frames)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_evaluate_one_epoch_is_the_mean_of_its_batches_and_touches_nothing(golden, family):
    from simple_tad_amd import engine_pretrain as EP, kernels as K, ops
    m, mask, size, patch, tub = FAMILIES[family](golden)
    B = mask.shape[0]
    grid = (size[0] // tub, size[1] // patch, size[2] // patch)
    mask2 = mask.flip(0).contiguous()
    loader = [(clips_for(size, B, 5)[1], mask.reshape(B, *grid)), (clips_for(size, B, 6)[1].cuda(), mask2)]   # host and device batches
    m.train()
    before = {k: (p.detach().clone(), p._version) for k, p in m.named_parameters()}
    stats = EP.evaluate_one_epoch(m, loader, torch.device("cuda"), patch_size=patch, tubelet_size=tub)
    assert m.training and set(stats) == {"loss", "error_grid"}
    for k, p in m.named_parameters():
        assert p._version == before[k][1] and same_bits(p.detach(), before[k][0]) and p.grad is None, k
    m.eval()
    losses, esum, cnt = [], 0, 0
    with torch.no_grad():
        for x, mk in loader:
            x, mk = x.cuda(), mk.reshape(B, -1).cuda()
            pred = m(x, mk)
            losses.append(ops.MseLossFn.apply(pred, EP.reconstruction_target(x, mk, patch, tub, True)))
            _, err = K.mae_reconstruct(x, pred, RR.slot_of(mk.cpu()).cuda(), tub, patch, RR.MEAN, RR.STD, True, want_frames=False)
            esum, cnt = esum + err.sum(0), cnt + mk.sum(0).float()
    assert stats["loss"] == (losses[0] + losses[1]).item() / 2, (stats["loss"], [float(v) for v in losses])
    want = (esum / cnt.clamp_min(1.0)).reshape(grid).cpu()
    assert stats["error_grid"].shape == grid and stats["error_grid"].device.type == "cpu"
    assert torch.allclose(stats["error_grid"], want, rtol=1e-6, atol=0)
    assert bool((stats["error_grid"][(cnt > 0).reshape(grid).cpu()] > 0).all())
    with pytest.raises(ValueError, match="evaluate_one_epoch: the clips of this batch mask different numbers of tokens"):
        bad = mask.clone()
        bad[0, bad[0].nonzero()[0]] = False
        EP.evaluate_one_epoch(m, [(loader[0][0], bad)], torch.device("cuda"), patch_size=patch, tubelet_size=tub)
    assert not m.training
