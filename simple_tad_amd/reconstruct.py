"""MAE reconstruction on the device: what a pre-trained model makes of a masked clip, as frames and as an error map.

The reference means to offer this (its ``vis.sh`` calls a ``run_videomae_vis.py`` it does not ship); pre-training was the one part of
this package whose only output was a scalar loss.  ``reconstruct`` runs a ``PretrainVisionTransformer`` or a
``PretrainVideoMAEInternVideo2`` on a clip and its mask and turns the prediction [B, N_mask, tub*p*p*3] back into pixels with the inverse
of the target arithmetic (engine_for_pretraining.py:51-66): one HIP launch (``kernels.mae_reconstruct``, include/tad_mi355x_recon.h)
writes the uint8 frames -- visible patches from the clip, masked patches from the prediction, de-standardised with the patch's own
statistics under ``normlize_target`` -- and the per-token error.  A wrong mask order, patch layout or target inverse shows in the
frames; with the labels themselves as prediction the clip comes back byte for byte.
"""
from __future__ import annotations

import torch

from . import kernels as K
from . import ops
from .engine_pretrain import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, masked_count
from .explain import saliency_to_frames
from .modeling_pretrain import slot_table

__all__ = ["reconstruct", "error_to_frames", "model_patch_geometry"]


def model_patch_geometry(model):
    """(patch, tubelet) of a pre-training model, read off its encoder's patch embedding"""
    pe = model.encoder.patch_embed
    patch = pe.patch_size
    if isinstance(patch, (tuple, list)):
        if patch[0] != patch[1]:
            raise ValueError(f"reconstruct: patches must be square, got {tuple(patch)}")
        patch = patch[0]
    return int(patch), int(pe.tubelet_size)


def reconstruct(model, clips: torch.Tensor, mask: torch.Tensor, *, normlize_target: bool = True, visible_gain: float = 1.0,
                mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD) -> dict:
    """clips [B,3,T,H,W] normalised f32, mask [B,N] or [B,T',H',W'] (True = masked; the same count in every clip) ->
      frames     uint8 [B,T,H,W,3]: visible patches are the clip's pixels (times ``visible_gain``, to dim them), masked patches the
                 model's prediction, un-standardised per (patch, channel) under ``normlize_target``
      error      f32 [B,T',H',W']: per token the mean (pred - target)^2, 0 where the token is visible
      pred       f32 [B,N_mask,tub*p*p*3]: ``model(clips, mask)`` in eval mode
      loss       the MSE of pred against the reconstruction target: the launch the training engine makes, the same bits
      mask_grid  bool [B,T',H',W']
    Runs under ``no_grad`` in eval mode; the model's mode is put back afterwards."""
    patch, tub = model_patch_geometry(model)
    if clips.dim() != 5:
        raise ValueError(f"reconstruct: clips must be [B,3,T,H,W], got {tuple(clips.shape)}")
    B, _, T, H, W = clips.shape
    grid = (T // tub, H // patch, W // patch)
    num_masked = masked_count(mask, "reconstruct")
    mask = torch.as_tensor(mask).to(clips.device, non_blocking=True).flatten(1).to(torch.bool)
    if mask.shape[1] != grid[0] * grid[1] * grid[2]:
        raise ValueError(f"reconstruct: the mask has {mask.shape[1]} tokens per clip, the clip {grid[0]} x {grid[1]} x {grid[2]}")
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            pred = model(clips, mask, num_masked=num_masked)
            videos = clips.float().contiguous()
            slot, mask_tok = slot_table(mask, num_masked)
            labels = K.mae_target(videos, mask_tok.reshape(-1), tub, patch, mean, std, normlize_target)
            loss = ops.MseLossFn.apply(pred, labels)
            frames, err = K.mae_reconstruct(videos, pred.float().contiguous(), slot, tub, patch, mean, std, normlize_target, visible_gain)
    finally:
        model.train(was_training)
    return {"frames": frames, "error": err.view(B, *grid), "pred": pred, "loss": loss, "mask_grid": mask.view(B, *grid)}


def error_to_frames(error, size, mode: str = "nearest"):
    """error [B,T',H',W'] -> [B,T,H,W] with size = (T, H, W): ``explain.saliency_to_frames`` under its MAE name"""
    return saliency_to_frames(error, size, mode)
