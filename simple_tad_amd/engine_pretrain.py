"""Counterpart of ``engine_for_pretraining.train_one_epoch`` (engine_for_pretraining.py:16-152) for the MAE pre-training path
(SURVEY 8f-2): per step -- lr / weight-decay assignment (:39-45), reconstruction target from the clip (:51-66, one HIP kernel on
the masked tokens only), model forward, ``nn.MSELoss`` (:68-70, fused loss + gradient kernel), ``loss.item()``, scaler step with
``clip_grad=max_norm`` (:79-81), the per-head gradient-norm diagnostics over the encoder (:30-33, 84-91, 134-147; one device-side
collect per step, ``train_one_epoch_with_grad_norms``), synchronise.  ``train_one_epoch_double`` (:155-307) is the same step over two
loaders at once, their batches joined.  Left out: the ``gc.collect()/empty_cache()`` per step (:36-37), tensorboard
logging."""
from __future__ import annotations

import math
import sys
from typing import Iterable

import torch

from . import kernels as K
from . import ops
from .modeling_pretrain import slot_table, token_indices
from .parallel import DataParallel

IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)  # timm.data.constants, engine_for_pretraining.py:10
IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)


def reconstruction_target(videos: torch.Tensor, bool_masked_pos: torch.Tensor, patch_size: int = 16, tubelet_size: int = 2,
                          normlize_target: bool = True, num_masked=None) -> torch.Tensor:
    """labels [B, N_mask, tub*p*p*3] (engine_for_pretraining.py:51-66)"""
    _, mask_tok = token_indices(bool_masked_pos.flatten(1), num_masked)
    return K.mae_target(videos.float().contiguous(), mask_tok.reshape(-1), tubelet_size, patch_size, IMAGENET_DEFAULT_MEAN,
                        IMAGENET_DEFAULT_STD, normlize_target)


def train_one_epoch(model: torch.nn.Module, data_loader: Iterable, optimizer, device: torch.device, epoch: int, loss_scaler,
                    max_norm: float = 0, patch_size: int = 16, normlize_target: bool = True, start_steps=0, lr_schedule_values=None,
                    wd_schedule_values=None, tubelet_size: int = 2, log=None, augment_fn=None):
    """augment_fn: applied to ``batch[0]`` right after it has reached the device (uint8 frames [B,T,Hs,Ws,3] ->
    ``transforms.DataAugmentationForVideoMAE``); where it returns a pair, the second item replaces ``batch[1]``, the masks."""
    return _train_one_epoch(model, data_loader, optimizer, device, epoch, loss_scaler, max_norm, patch_size, normlize_target, start_steps,
                            lr_schedule_values, wd_schedule_values, tubelet_size, log, augment_fn, None)


def train_one_epoch_with_grad_norms(model: torch.nn.Module, data_loader: Iterable, optimizer, device: torch.device, epoch: int, loss_scaler,
                                    grad_norms, max_norm: float = 0, patch_size: int = 16, normlize_target: bool = True, start_steps=0,
                                    lr_schedule_values=None, wd_schedule_values=None, tubelet_size: int = 2, log=None, augment_fn=None):
    """``train_one_epoch`` with the per-head gradient-norm diagnostics of engine_for_pretraining.py:30-33, 84-91, 134-147 switched on.
    ``grad_norms``: a ``grad_norms.GradNormCollector`` over this model (it collects over ``model.encoder``) and optimizer: one device-side
    collect after every scaler call with the scaler's coefficient, no host sync per step; ``stats["grad_norms"]`` = the epoch
    averages {"qkv", "proj", "patch_embed"}, read back once.  An entry point of its own, not a keyword of ``train_one_epoch`` as in
    ``engine.train_one_epoch``: that function's parameter list is fixed (tests/test_multiscale_crop_cpu.py pins it name by name)."""
    if grad_norms is None:
        raise ValueError("train_one_epoch_with_grad_norms: no collector (grad_norms.GradNormCollector(model, optimizer))")
    return _train_one_epoch(model, data_loader, optimizer, device, epoch, loss_scaler, max_norm, patch_size, normlize_target, start_steps,
                            lr_schedule_values, wd_schedule_values, tubelet_size, log, augment_fn, grad_norms)


def train_one_epoch_double(model: torch.nn.Module, data_loader1: Iterable, data_loader2: Iterable, optimizer, device: torch.device,
                           epoch: int, loss_scaler, max_norm: float = 0, patch_size: int = 16, normlize_target: bool = True, start_steps=0,
                           lr_schedule_values=None, wd_schedule_values=None, tubelet_size: int = 2, log=None, augment_fn=None):
    """Counterpart of ``engine_for_pretraining.train_one_epoch_double`` (engine_for_pretraining.py:155-307), the step of domain-adaptive
    pre-training on two datasets at once: it walks ``zip(data_loader1, data_loader2)`` (so it stops with the shorter loader), joins the
    clips and the masks of the two batches along the batch dimension, loader 1's first (:196-199), and runs the step of
    ``train_one_epoch`` on the joined batch.  Host batches are joined on the host and move to the device as one tensor; batches a
    ``prefetch.ClipPrefetcher`` already delivered to the device are joined there.  Every clip of the JOINED batch must mask the same
    number of tokens: another count in loader 2's batch is refused before any kernel runs.

    Returns the ``stats`` dict of ``train_one_epoch``.  The reference returns a pair whose second item, the gradient-norm diagnostics,
    is always ``None``: its collect call is commented out (:234-235, with ``with_grad_norms`` left False by its caller).  There is no
    ``grad_norms`` argument here for that reason."""
    return _train_one_epoch(model, _joined_batches(data_loader1, data_loader2, device), optimizer, device, epoch, loss_scaler, max_norm,
                            patch_size, normlize_target, start_steps, lr_schedule_values, wd_schedule_values, tubelet_size, log, augment_fn,
                            None, who="train_one_epoch_double")


def _join(a, b, device):
    """two batches' tensors as one, a's rows first: where both already are where the other is they are joined there (host with host,
    device with device); a host half beside a device half follows it to the device first"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.device != b.device:
        a, b = a.to(device, non_blocking=True), b.to(device, non_blocking=True)
    return torch.cat([a, b], dim=0)


def _joined_batches(data_loader1, data_loader2, device):
    """the step iterator of ``train_one_epoch_double``: (clips, masks) of loader 1's batch followed by loader 2's.  Masks are flattened
    per clip before they are joined, so that the two loaders may deliver them as [B, T, H, W] or [B, N] alike; a pair of batches
    without masks (an ``augment_fn`` draws them) yields the clips alone.  Masks from one loader only are refused: dropping them would
    hide the mismatch behind a later message, or behind masks an ``augment_fn`` draws anew."""
    for step, (batch1, batch2) in enumerate(zip(data_loader1, data_loader2)):
        has1, has2 = len(batch1) > 1, len(batch2) > 1
        if has1 != has2:
            raise ValueError(f"train_one_epoch_double: step {step}: data_loader{1 if has1 else 2} delivers masks and "
                             f"data_loader{2 if has1 else 1} does not; both loaders must deliver (clips, masks), or both the clips alone")
        videos = _join(batch1[0], batch2[0], device)
        if has1:
            yield videos, _join(torch.as_tensor(batch1[1]).flatten(1), torch.as_tensor(batch2[1]).flatten(1), device)
        else:
            yield (videos,)


def masked_count(bool_masked_pos, who) -> int:
    """the number of tokens every clip of the batch masks; another count in any clip is refused, naming the counts"""
    # host-side counts (the mask comes from the loader's generator): one read of all clips' counts where clip 0's was read before
    counts = torch.as_tensor(bool_masked_pos).flatten(1).to(torch.bool).sum(1).tolist()
    num_masked = int(counts[0])
    if any(c != num_masked for c in counts):
        # token_indices splits every clip at clip 0's count: masked tokens of another clip would land among the visible ones
        # (the reference's x[~mask].reshape(B, -1, C) usually raises here)
        raise ValueError(f"{who}: the clips of this batch mask different numbers of tokens {counts}; "
                         "every clip of a batch must mask the same number")
    return num_masked


def _step_inputs(batch, device, augment_fn, who):
    """(clips on the device, bool masks [B,N] on the device, masked tokens per clip) of one (clips, masks) or (clips,) batch"""
    videos = batch[0].to(device, non_blocking=True)
    bool_masked_pos = batch[1] if len(batch) > 1 else None
    if augment_fn is not None:
        augmented = augment_fn(videos)
        videos, bool_masked_pos = augmented if isinstance(augmented, (tuple, list)) else (augmented, bool_masked_pos)
    if bool_masked_pos is None:
        raise ValueError(f"{who}: no masks for this step: the batch holds one item and augment_fn "
                         + ("returned the clips alone" if augment_fn is not None else "is None")
                         + " (pass (clips, masks) batches, or an augment_fn that returns (clips, masks))")
    num_masked = masked_count(bool_masked_pos, who)
    bool_masked_pos = torch.as_tensor(bool_masked_pos).to(device, non_blocking=True).flatten(1).to(torch.bool)
    return videos, bool_masked_pos, num_masked


def _train_one_epoch(model, data_loader, optimizer, device, epoch, loss_scaler, max_norm, patch_size, normlize_target, start_steps,
                     lr_schedule_values, wd_schedule_values, tubelet_size, log, augment_fn, grad_norms, who="train_one_epoch"):
    """``data_loader``: the step iterator -- anything that yields (clips, masks) or (clips,) batches, one per step"""
    model.train()
    dp = model if isinstance(model, DataParallel) else None
    inner = dp.module if dp is not None else model
    zero = dp.zero_grad if dp is not None else (lambda: optimizer.zero_grad(set_to_none=False))
    params = [p for p in model.parameters() if p.requires_grad]
    names = ("loss", "grad_norm", "lr", "min_lr", "loss_scale", "weight_decay")  # fixed list: every rank packs the same rows
    stats = {k: [] for k in names}
    for step, batch in enumerate(data_loader):
        it = start_steps + step
        if lr_schedule_values is not None or wd_schedule_values is not None:
            for group in optimizer.param_groups:
                if lr_schedule_values is not None:
                    group["lr"] = lr_schedule_values[it] * group.get("lr_scale", 1.0)
                if wd_schedule_values is not None and group["weight_decay"] > 0:
                    group["weight_decay"] = wd_schedule_values[it]
        videos, bool_masked_pos, num_masked = _step_inputs(batch, device, augment_fn, who)
        with torch.no_grad():
            labels = reconstruction_target(videos, bool_masked_pos, patch_size, tubelet_size, normlize_target, num_masked)
        outputs = inner(videos, bool_masked_pos, num_masked=num_masked) if dp is None else dp(videos, bool_masked_pos, num_masked=num_masked)
        loss = ops.MseLossFn.apply(outputs, labels)
        loss_value = loss.item()
        if not math.isfinite(loss_value):
            print("Loss is {}, stopping training".format(loss_value))
            sys.exit(1)
        zero()
        grad_norm = loss_scaler(loss, optimizer, clip_grad=max_norm if max_norm else None, parameters=params)
        if grad_norms is not None:
            # the reference collects right behind its scaler (:81-86), which has unscaled and clipped p.grad in place: the coefficient
            grad_norms.collect(getattr(loss_scaler, "last_coef", None))
        if device.type == "cuda":
            torch.cuda.synchronize()
        stats["loss"].append(loss_value)
        stats["grad_norm"].append(None if grad_norm is None else float(grad_norm))
        stats["loss_scale"].append(loss_scaler.state_dict()["scale"])
        stats["lr"].append(max(g["lr"] for g in optimizer.param_groups))
        stats["min_lr"].append(min(g["lr"] for g in optimizer.param_groups))
        stats["weight_decay"].append(next((g["weight_decay"] for g in optimizer.param_groups if g["weight_decay"] > 0), None))
        if log is not None:
            log(epoch, step, stats)
    # engine_for_pretraining.py:149-152: metric_logger.synchronize_between_processes() -> {k: meter.global_avg}
    from .engine import synchronize_meters
    stats["averaged"] = synchronize_meters(stats, device, group=dp.pg if dp is not None else None, names=names)
    if grad_norms is not None:
        stats["grad_norms"] = grad_norms.result(len(data_loader))
    return stats


def evaluate_one_epoch(model: torch.nn.Module, data_loader: Iterable, device: torch.device, patch_size: int = 16, normlize_target: bool = True,
                       tubelet_size: int = 2, augment_fn=None):
    """The held-out pass of MAE pre-training (the reference has none): the batches go through the batch handling and the mask-count check
    of the training step, the model runs in eval mode under ``no_grad``, and no optimizer is involved.  Per batch the loss is the
    training step's (``reconstruction_target`` and the ``tad_mse_loss`` launch) and the per-token error comes from the reconstruction
    kernel (``kernels.mae_reconstruct``, err only).  The running sums stay on the device; they are read back once, at the end.

    Returns {"loss": the mean of the batches' losses, "error_grid": f32 [T/tub, H/p, W/p] on the host: per grid position the mean error
    over the clips that masked it (0 where no clip did)}.  The model's mode is put back afterwards."""
    inner = model.module if isinstance(model, DataParallel) else model
    was_training = inner.training
    inner.eval()
    sums, steps = None, 0
    try:
        with torch.no_grad():
            for batch in data_loader:
                videos, bool_masked_pos, num_masked = _step_inputs(batch, device, augment_fn, "evaluate_one_epoch")
                labels = reconstruction_target(videos, bool_masked_pos, patch_size, tubelet_size, normlize_target, num_masked)
                outputs = inner(videos, bool_masked_pos, num_masked=num_masked)
                loss = ops.MseLossFn.apply(outputs, labels)
                slot, _ = slot_table(bool_masked_pos, num_masked)
                _, err = K.mae_reconstruct(videos.float().contiguous(), outputs.float().contiguous(), slot, tubelet_size, patch_size,
                                           IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, normlize_target, want_frames=False)
                # one row of running sums: [loss, err per position ..., masked clips per position ...]
                row = torch.cat([loss.reshape(1), err.sum(0), bool_masked_pos.sum(0).float()])
                sums = row if sums is None else sums + row
                steps += 1
                grid = (videos.shape[2] // tubelet_size, videos.shape[3] // patch_size, videos.shape[4] // patch_size)
    finally:
        inner.train(was_training)
    if sums is None:
        raise ValueError("evaluate_one_epoch: the loader delivered no batch")
    host = sums.cpu()
    n = (host.numel() - 1) // 2
    return {"loss": host[0].item() / steps, "error_grid": (host[1:1 + n] / host[1 + n:].clamp_min(1.0)).reshape(grid)}
