"""Thin counterparts of the training-runtime pieces the fine-tune hot loop needs
(reference: engine_for_finetuning.py:24-140, utils.py:386-447, optim_factory.py:24-127).

Same step ordering as ``engine_for_finetuning.train_one_epoch``: per-step lr/wd assignment from the
schedule tables, forward, loss, ``loss.item()`` finiteness check, backward, gradient norm / clipping,
optimizer step, ``zero_grad``, device synchronise, meters.  Differences, by design: loss scaling is live only
for IEEE-half operands (``set_precision("half")``, the reference's own autocast dtype); the bfloat16 kernels need
none and the scaler then reports ``scale == 1.0``; the gradient all-reduce is the bucketed RCCL exchange of
``parallel.DataParallel``.

Evaluation: ``validation_one_epoch`` and ``final_test`` (engine_for_frame_finetuning.py:282-383, 385-545; the latter writes the
reference's ``predictions.csv`` and stats file).  Both take clip tensors or ``frame_store.FrameWindows`` as ``batch[0]``.
"""
from __future__ import annotations

import json
import math
import os
import sys
from typing import Iterable, Optional

import numpy as np
import torch

from . import kernels as K
from . import ops
from .parallel import DataParallel


def cosine_scheduler(base_value, final_value, epochs, niter_per_ep, warmup_epochs=0, start_warmup_value=0, warmup_steps=-1):
    """utils.cosine_scheduler (utils.py:430-447): linear warm-up then half-cosine, one value per iteration."""
    warmup_iters = warmup_steps if warmup_steps > 0 else warmup_epochs * niter_per_ep
    warm = np.linspace(start_warmup_value, base_value, warmup_iters) if warmup_epochs > 0 else np.array([])
    n = epochs * niter_per_ep - warmup_iters
    cos = np.array([final_value + 0.5 * (base_value - final_value) * (1 + math.cos(math.pi * i / n)) for i in range(n)])
    schedule = np.concatenate((warm, cos))
    assert len(schedule) == epochs * niter_per_ep
    return schedule


def get_num_layer_for_vit(var_name, num_max_layer):
    """optim_factory.py:24-35"""
    if var_name in ("cls_token", "mask_token", "pos_embed") or var_name.startswith("patch_embed"):
        return 0
    if var_name.startswith("rel_pos_bias"):
        return num_max_layer - 1
    if var_name.startswith("blocks"):
        return int(var_name.split('.')[1]) + 1
    return num_max_layer - 1


class LayerDecayValueAssigner:
    """optim_factory.py:38-46; values = [decay ** (L + 1 - i) for i in range(L + 2)] (run_class_finetuning.py:430-434)"""

    def __init__(self, values):
        self.values = values

    @classmethod
    def from_decay(cls, layer_decay: float, num_layers: int):
        return cls([layer_decay ** (num_layers + 1 - i) for i in range(num_layers + 2)])

    def get_scale(self, layer_id):
        return self.values[layer_id]

    def get_layer_id(self, var_name):
        return get_num_layer_for_vit(var_name, len(self.values))


def get_parameter_groups(model, weight_decay=1e-5, skip_list=(), get_num_layer=None, get_layer_scale=None, verbose=False):
    """The grouping rule of optim_factory.get_parameter_groups (optim_factory.py:49-88): a parameter is undecayed when it is 1-D,
    a ``.bias`` or skip-listed; with layer-wise lr decay every (layer, decayed?) pair is a group of its own carrying ``lr_scale``.
    Groups come out in order of first appearance in ``model.named_parameters()`` -- the order the reference hands to AdamW, and what
    golden G12 pins (group names, member order, weight decay, lr_scale)."""
    skip = frozenset(skip_list)
    trainable = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    # key of a parameter = (layer id | None, decayed?)
    keys = [(None if get_num_layer is None else get_num_layer(n), not (p.dim() == 1 or n.endswith(".bias") or n in skip)) for n, p in trainable]
    groups, members = {}, {}
    for key, (name, param) in zip(keys, trainable):
        if key not in groups:
            layer, decayed = key
            groups[key] = {"weight_decay": weight_decay if decayed else 0., "params": [],
                           "lr_scale": 1. if get_layer_scale is None else get_layer_scale(layer)}
            members[key] = []
        groups[key]["params"].append(param)
        members[key].append(name)
    if verbose:
        def label(key):
            kind = "decay" if key[1] else "no_decay"
            return kind if key[0] is None else "layer_%d_%s" % (key[0], kind)
        print("Param groups = %s" % json.dumps({label(k): dict(groups[k], params=members[k]) for k in groups}, indent=2))
    return list(groups.values())


def create_optimizer(model, lr, weight_decay=0.05, betas=(0.9, 0.999), eps=1e-8, layer_decay: Optional[float] = None,
                     skip_list=None, fused_kernel: Optional[bool] = None):
    """AdamW over the reference's parameter groups (optim_factory.create_optimizer with opt='adamw',
    optim_factory.py:91-127); the rest of the reference's optimizer zoo is out of scope.  On the GPU this is
    optim.FusedAdamW (one HIP launch per step over the flat layout it shares with DataParallel); ``fused_kernel=False`` or
    CPU parameters give torch.optim.AdamW over the same groups."""
    inner = model.module if isinstance(model, DataParallel) else model
    skip = set(skip_list) if skip_list is not None else (inner.no_weight_decay() if hasattr(inner, "no_weight_decay") else set())
    assigner = LayerDecayValueAssigner.from_decay(layer_decay, inner.get_num_layers()) if layer_decay and layer_decay < 1.0 else None
    groups = get_parameter_groups(inner, weight_decay, skip, assigner.get_layer_id if assigner else None,
                                  assigner.get_scale if assigner else None)
    on_gpu = all(p.is_cuda for g in groups for p in g["params"])
    if fused_kernel is None:
        fused_kernel = on_gpu
    if fused_kernel:
        from .optim import FusedAdamW
        return FusedAdamW(groups, lr=lr, betas=betas, eps=eps, weight_decay=0.0,
                          space=model.space if isinstance(model, DataParallel) else None)
    return torch.optim.AdamW(groups, lr=lr, betas=betas, eps=eps, weight_decay=0.0, fused=on_gpu)


def freeze_layers(model, spec) -> int:
    """``--freeze_layers`` of the reference's fine-tuning scripts (run_frame_finetuning.py:143, 465-485), its rule restated with its
    substring tests: for ``spec`` starting with ``"first N blocks"``, N = int(spec.split(";")[1]) and, per named parameter,
      * ``"blocks"`` in the name: layer = int(name.split(".")[1]); below N it is frozen unless ``"norm"`` is in the name, from N on
        it is trainable;
      * else ``"patch_embed"`` in the name: frozen;
      * everything else (fc_norm, norm, head, ...): trainable.
    So the eight Linear tensors, q_bias / v_bias and gamma_1 / gamma_2 of the first N blocks and the patch projection are frozen, and
    the norms of the frozen blocks keep training.  Any other ``spec`` changes nothing (as in the reference) and warns once.  Returns
    the number of parameters the rule froze.  Takes a bare model or a DataParallel wrapper; call it before ``create_optimizer`` (and
    before wrapping, so that the flat gradient layout holds the trainable parameters only): ``get_parameter_groups`` drops frozen
    parameters, and the 16-bit Functions then launch no weight gradient for them and keep no operand for one (ops.set_skip_frozen)."""
    inner = model.module if isinstance(model, DataParallel) else model
    if not (isinstance(spec, str) and spec.startswith("first N blocks")):
        import warnings
        warnings.warn(f"freeze_layers: {spec!r} is not of the form 'first N blocks;N'; nothing is frozen")
        return 0
    n_blocks = int(spec.split(";")[1])
    frozen = 0
    for name, param in inner.named_parameters():
        if "blocks" in name:
            param.requires_grad = not (int(name.split(".")[1]) < n_blocks and "norm" not in name)
        elif "patch_embed" in name:
            param.requires_grad = False
        else:
            param.requires_grad = True
        frozen += not param.requires_grad
    return frozen


def get_grad_norm_(parameters, norm_type: float = 2.0) -> torch.Tensor:
    """utils.get_grad_norm_ (utils.py:415-427) for norm_type 2: norm(stack(norm(g))) == sqrt(sum ||g||^2).
    On GPU the sum of squares runs through tad_sumsq_f32 (one pass over the gradients)."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.)
    assert float(norm_type) == 2.0, "only the L2 norm is used by the reference's engines"
    if grads[0].is_cuda:
        acc = torch.zeros(1, dtype=torch.float32, device=grads[0].device)
        for g in grads:
            K.sumsq(g.detach().reshape(-1) if g.is_contiguous() else g.detach().contiguous().reshape(-1), acc)
        return acc.sqrt()[0]
    return torch.norm(torch.stack([torch.norm(g.detach(), 2.0) for g in grads]), 2.0)


class NativeScalerWithGradNormCount:
    """utils.NativeScalerWithGradNormCount (utils.py:386-412): backward -> (all-reduce wait) -> unscale -> clip or norm -> optimizer
    step -> scale update.  The reference wraps ``torch.cuda.amp.GradScaler()`` because its autocast arithmetic is float16; here loss
    scaling is live exactly when the kernels run on IEEE-half operands (``set_precision("half")``) and a no-op (scale 1.0) for the
    bfloat16 and precise modes, whose range is f32's.  GradScaler's defaults and rules: scale 65536, halved after a step whose
    gradients held an inf / NaN (that step is skipped), doubled after 2000 consecutive good steps.  The scale is removed inside the
    fused AdamW (its ``grad_scale`` operand, together with the clipping coefficient), so no extra pass touches the gradients.
    GradScaler.step reads "found inf" on the host before it calls the optimizer -- a host sync between backward and the optimizer that
    leaves the GPU idle while the host queues the next launches.  With the fused AdamW the decision is taken ON THE DEVICE instead
    (``*grad_scale == 0`` skips the update inside the kernel) and the host reads the flag one step late, at the start of the next
    call -- before the scale is used again, so scale, skipped steps and the optimizer's step counts end up exactly as GradScaler's."""
    state_dict_key = "amp_scaler"

    def __init__(self, model: Optional[torch.nn.Module] = None, enabled: Optional[bool] = None, init_scale: float = 65536.0,
                 growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000):
        self.model = model
        self.enabled = enabled  # None: follow the precision mode at call time
        self.scale = float(init_scale)
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self.growth_tracker = 0
        self.skipped_steps = 0
        self._pending = None  # (found-inf flag in pinned host memory, the event behind its copy, optimizer) of the last fused step, not yet read
        self._flag_host = None
        # the device coefficient (f32 [1]: unscale and clip; 0 = skipped on the device) the last fused step multiplied into the gradients,
        # None when it applied none -- what grad_norms.GradNormCollector.collect takes to see the gradients the reference sees
        self.last_coef = None

    def _settle(self):
        """read the previous fused step's found-inf flag and bring the scale and, after a skipped step, the optimizer's step counts up
        to date.  The flag travelled to pinned host memory by an asynchronous copy issued right behind the norm kernel, and an event
        recorded there is what the host waits for -- NOT the stream: by the time this runs the forward of the next step is already
        queued, so the GPU keeps working through the wait.  (Round 4 read the flag with ``.item()``: a copy queued BEHIND that forward,
        i.e. a full stream drain in front of every backward pass -- 0.5-1.0 ms of idle GPU per step in the kernel trace,
        profiles/r05_kernel_stats_half.txt.)"""
        if self._pending is None:
            return
        flag, event, optimizer, scaled = self._pending
        self._pending = None
        if event is not None:
            event.synchronize()
        found_inf = bool(flag[0].item() != 0)  # (pinned host memory behind its event, or a CPU tensor: no device round trip)
        if scaled:
            self._update_scale(found_inf)
        elif found_inf:
            self.skipped_steps += 1  # (clipping without loss scaling: the step was skipped on the device, the scale is not in play)
        if found_inf:
            optimizer.rollback_step()

    def scaling(self) -> bool:
        return (ops.get_precision() == "half") if self.enabled is None else bool(self.enabled)

    def _update_scale(self, found_inf: bool):
        if found_inf:
            self.scale *= self.backoff_factor
            self.growth_tracker = 0
            self.skipped_steps += 1
        else:
            self.growth_tracker += 1
            if self.growth_tracker >= self.growth_interval:
                self.scale *= self.growth_factor
                self.growth_tracker = 0

    def __call__(self, loss, optimizer, clip_grad=None, parameters=None, create_graph=False, update_grad=True):
        dp = self.model if isinstance(self.model, DataParallel) else None
        if dp is not None:
            dp.require_sync = bool(update_grad)  # gradient accumulation: exchange only on the last micro-step
        scaling = self.scaling()
        self._settle()
        (loss * self.scale if scaling else loss).backward(create_graph=create_graph)
        if not update_grad:
            return None
        if dp is not None:
            dp.finish()
        from .optim import FusedAdamW
        inv = 1.0 / self.scale if scaling else 1.0
        self.last_coef = None
        if isinstance(optimizer, FusedAdamW):
            # the norm of utils.get_grad_norm_ comes out of the optimizer's own pass over the gradients; with clipping or loss scaling
            # the coefficient (1 / scale) * min(1, max_norm / (norm + 1e-6)) of GradScaler.unscale_ + clip_grad_norm_ stays on the device
            clip = clip_grad is not None and clip_grad > 0
            if clip or scaling:
                # ONE pass over the flat gradients + a one-thread finish: norm, coefficient (0 = overflow: the kernel skips the step)
                # and the found-inf flag, all on the device (tad_grad_norm_coef)
                # A NON-FINITE norm makes the coefficient 0 in EVERY mode (tad_grad_norm_coef), i.e. the update is skipped on the device.
                # Under loss scaling that is GradScaler's rule.  Under clipping WITHOUT scaling (bf16 / precise) it is a deliberate
                # difference from the reference, whose clip_grad_norm_ would multiply the gradients by NaN and write NaN into every weight
                # (utils.py:401-404): here the weights survive, and the skip is accounted for like a scaled one -- counted in
                # `skipped_steps`, the optimizer's step counts rolled back -- when the flag is read at the next call.
                nc = K.grad_norm_coef(optimizer.flat_grad, inv, clip_grad if clip else 0.0)
                norm = nc[0]
                # the flag is read at the next call, from pinned host memory behind an event (see _settle)
                if self._flag_host is None:
                    self._flag_host = torch.zeros(1, dtype=torch.float32).pin_memory()
                self._flag_host.copy_(nc[2:3], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                self._pending = (self._flag_host, ev, optimizer, scaling)
                self.last_coef = nc[1:2]
                optimizer.step(grad_scale=nc[1:2])
            else:
                norm = optimizer.step(want_sumsq=True).sqrt()
            return norm
        if scaling:  # any other optimizer: unscale in place (GradScaler.unscale_), then the reference's order
            if parameters is None:
                raise ValueError("NativeScalerWithGradNormCount: loss scaling with an optimizer other than FusedAdamW needs `parameters` "
                                 "(the gradients are unscaled and checked here before the step)")
            grads = [p.grad for p in parameters if p.grad is not None]
            found = torch.zeros((), dtype=torch.float32, device=grads[0].device) if grads else None
            for g in grads:  # one reduction per tensor on the device, ONE host read for all of them
                g.mul_(inv)
                found += (~torch.isfinite(g)).any().float()
            found_inf = bool(grads) and bool(found.item() > 0)
            self._update_scale(found_inf)
            if found_inf:
                return torch.tensor(float("inf"))
        if clip_grad is not None and clip_grad > 0:
            assert parameters is not None
            norm = torch.nn.utils.clip_grad_norm_(parameters, clip_grad)
        else:
            if dp is not None and not scaling:
                acc = torch.zeros(1, dtype=torch.float32, device=dp.flat_grad.device)
                norm = (K.sumsq(dp.flat_grad, acc).sqrt()[0] if dp.flat_grad.is_cuda else dp.flat_grad.norm())
            else:
                norm = get_grad_norm_(parameters)
        optimizer.step()
        ops.invalidate_weight_cache(keep_static=True)  # fused optimizers do not bump Parameter._version (see ops._cached)
        return norm

    def state_dict(self):
        """GradScaler.state_dict()'s keys.  ``scale`` reads 1.0 while no scaling is applied -- the engines log it as loss_scale each step
        (engine_for_finetuning.py:100) -- and the scale this object carries travels beside it as ``_scale`` so that a checkpoint
        written in one precision mode resumes correctly in another (the 65536 of a half-mode run used to be dropped when
        the precision was set after the load, and a bf16-mode checkpoint installed scale 1.0 in a half-mode run)."""
        self._settle()
        return {"scale": self.scale if self.scaling() else 1.0, "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": self.growth_tracker, "_scale": self.scale}

    def load_state_dict(self, state_dict):
        """restores the carried scale whatever the precision mode is at this moment; a checkpoint without ``_scale`` (the reference's
        GradScaler, or an older run of this package) provides ``scale``, which is ignored when it is the 1.0 placeholder of a run that
        applied no scaling"""
        if "_scale" in state_dict:
            self.scale = float(state_dict["_scale"])
        elif "scale" in state_dict and float(state_dict["scale"]) != 1.0:
            self.scale = float(state_dict["scale"])
        elif "scale" in state_dict and self.scaling():
            import warnings
            warnings.warn("NativeScalerWithGradNormCount.load_state_dict: the checkpoint carries loss scale 1.0 (written without loss scaling); "
                          f"keeping this run's scale {self.scale:g} for the IEEE-half mode")
        self.growth_tracker = int(state_dict.get("_growth_tracker", self.growth_tracker))


METER_NAMES = ("loss", "class_acc", "grad_norm", "lr", "min_lr", "loss_scale")


def synchronize_meters(stats: dict, device=None, group=None, names=None) -> dict:
    """C4 of SURVEY 2.3 -- ``MetricLogger.synchronize_between_processes`` (utils.py:71-82, called at engine_for_finetuning.py:138):
    every meter's (count, total) summed over the ranks, returned as ``{name: global_avg}`` (engine_for_finetuning.py:140), so every
    rank logs the same epoch averages.  The reference issues one barrier + one fp64 all-reduce PER meter; here all meters travel in
    ONE fp64 all-reduce of a [n_meters, 2] tensor over ``group`` (the process group of the gradient exchange; default group if
    None).  ``names`` fixes the meter list: every rank must pack the same rows in the same order, so the engines pass their full
    list and a meter a rank never updated travels as (0, 0) -- a per-rank list derived from the dict would make the collective's
    shape differ across ranks and hang.  Single process: the local averages.  ``None`` entries are skipped as MetricLogger.update
    does (utils.py:121-122)."""
    import torch.distributed as dist
    if names is None:
        names = sorted(k for k, v in stats.items() if isinstance(v, list))
    names = list(names)
    packed = torch.zeros((len(names), 2), dtype=torch.float64)
    for i, k in enumerate(names):
        vals = [float(v) for v in stats.get(k, ()) if v is not None]
        packed[i, 0], packed[i, 1] = len(vals), sum(vals)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        if dist.get_backend(group) == "nccl":
            packed = packed.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
        dist.all_reduce(packed, group=group)
        packed = packed.cpu()
    return {k: (packed[i, 1] / packed[i, 0]).item() for i, k in enumerate(names) if packed[i, 0] > 0}


def train_class_batch(model, samples, target, criterion):
    """engine_for_finetuning.py:13-16"""
    outputs = model(samples)
    loss = criterion(outputs, target)
    return loss, outputs


def train_class_batch_ttc(model, samples, target, ttc, criterion):
    """engine_for_frame_finetuning.py:33-36"""
    outputs = model(samples)
    loss = criterion(outputs, target, ttc)
    return loss, outputs


def _loss_inputs(batch, targets, device, with_ttc, smoothed_labels_for_loss):
    """engine_for_frame_finetuning.py:114-120: (targets of the loss, ttc or None) from ``extra_info = batch[3]``"""
    targets_loss = batch[3]["smoothed_labels"].to(device, non_blocking=True) if smoothed_labels_for_loss else targets
    ttc = batch[3]["ttc"].to(device, non_blocking=True) if with_ttc else None
    return targets_loss, ttc


def train_one_epoch(model: torch.nn.Module, criterion, data_loader: Iterable, optimizer, device, epoch: int, loss_scaler,
                    max_norm: float = 0, start_steps=0, lr_schedule_values=None, wd_schedule_values=None,
                    num_training_steps_per_epoch=None, update_freq=1, log=None, model_ema=None, with_ttc=False, smoothed_labels_for_loss=False,
                    grad_norms=None, augment_fn=None, erase_fn=None, mixup_fn=None):
    """engine_for_finetuning.train_one_epoch (engine_for_finetuning.py:24-140) without the DeepSpeed branches.
    ``with_ttc`` / ``smoothed_labels_for_loss`` are the two switches of engine_for_frame_finetuning.train_one_epoch (:49, :114-142), for
    the criteria of ``loss.build_criterion``: the loader's fourth item, ``extra_info = batch[3]``, is then a dict with ``"ttc"`` (time to
    the anomaly per sample, ``frame_targets.compute_time_vector``) and ``"smoothed_labels"`` ([B,2], ``frame_targets.smooth_labels``).
    With ``smoothed_labels_for_loss`` the smoothed labels replace the targets FOR THE LOSS ONLY (``class_acc`` keeps the hard targets);
    with ``with_ttc`` the criterion is called as ``criterion(outputs, targets_loss, ttc)``.  As in the reference, a ``mixup_fn`` does
    not reach the loss targets once they are taken (:114-123).
    ``mixup_fn`` (a ``mixup.Mixup`` or anything with ``(samples, targets) -> (samples, soft_targets)``) is applied to every batch once it
    is on the device (:59-60); the criterion then has to take soft targets (``loss.SoftTargetCrossEntropy``), and ``class_acc`` is
    logged as ``None`` for the step, as the reference does (:104-107), so it does not appear in ``averaged``.
    ``erase_fn`` (a ``random_erasing.RandomErasing`` or anything with ``samples -> samples``) is applied before it, to the batch on the
    device: the reference erases in its dataset workers (dota.py:318-329), i.e. before the batch is mixed as well.
    ``augment_fn`` (anything with ``samples -> samples``) is applied first of the three, right after the batch has reached the device
    (the reference augments its PIL frames before it normalises and erases them, dota.py:299-316).  With a loader that yields uint8
    frames [B,T,H,W,3] there are two routes: ``augment_fn=rand_augment.RandAugment`` alone -- uint8 out, which the model's uint8
    input stage takes as it is -- or ``augment_fn=lambda x: frames_to_clip(randaug(x), mean, std)`` -- normalised f32 clips
    [B,3,T,H,W] out, which ``erase_fn`` and ``mixup_fn`` then take, and after them the model.  With the default nothing changes.
    ``model_ema`` (an ``ema.ModelEma`` or anything with ``update(model)``) is updated after every completed optimizer step, i.e. on
    the last micro-step of each ``update_freq`` group, as the reference does (:96-99) -- also after a step that the loss scaler
    skipped on the device, where the average then moves toward the unchanged weights.  The update is queued on the stream behind
    the optimizer step: no host sync.
    ``grad_norms`` (a ``grad_norms.GradNormCollector`` over this model and optimizer) switches on the per-head gradient-norm diagnostics
    of engine_for_frame_finetuning.train_one_epoch(get_grad_norms=True) (:76-83, 173-185, 232-251): one device-side collect after
    every scaler call, no host sync per step, and ``stats["grad_norms"]`` = the epoch averages {"qkv", "proj", "patch_embed"} the
    reference returns, read back once at the end.  Without a collector nothing changes: no launch, no key.
    The loader yields (samples [B,3,T,H,W], targets [B], *rest).  Returns the per-step meter lists of THIS rank plus
    ``stats["averaged"]`` = the cross-rank epoch averages the reference returns (``{k: meter.global_avg}``)."""
    model.train(True)
    dp = model if isinstance(model, DataParallel) else None
    zero = (dp.zero_grad if dp is not None else lambda: optimizer.zero_grad(set_to_none=False))
    zero()
    stats = {k: [] for k in METER_NAMES}
    params = [p for p in model.parameters() if p.requires_grad]
    for data_iter_step, batch in enumerate(data_loader):
        samples, targets = batch[0], batch[1]
        step = data_iter_step // update_freq
        if num_training_steps_per_epoch is not None and step >= num_training_steps_per_epoch:
            continue
        it = start_steps + step
        if (lr_schedule_values is not None or wd_schedule_values is not None) and data_iter_step % update_freq == 0:
            for group in optimizer.param_groups:
                if lr_schedule_values is not None:
                    group["lr"] = lr_schedule_values[it] * group.get("lr_scale", 1.0)
                if wd_schedule_values is not None and group["weight_decay"] > 0:
                    group["weight_decay"] = wd_schedule_values[it]
        samples = samples.to(device, non_blocking=True)
        targets = targets.to(device, non_blocking=True)
        if augment_fn is not None:
            samples = augment_fn(samples)
        if erase_fn is not None:
            samples = erase_fn(samples)
        if with_ttc or smoothed_labels_for_loss:
            targets_loss, ttc = _loss_inputs(batch, targets, device, with_ttc, smoothed_labels_for_loss)
        if mixup_fn is not None:
            samples, targets = mixup_fn(samples, targets)
        if with_ttc:
            loss, output = train_class_batch_ttc(model, samples, targets_loss, ttc, criterion)
        elif smoothed_labels_for_loss:
            loss, output = train_class_batch(model, samples, targets_loss, criterion)
        else:
            loss, output = train_class_batch(model, samples, targets, criterion)
        loss_value = loss.item()
        if not math.isfinite(loss_value):
            print("Loss is {}, stopping training".format(loss_value))
            sys.exit(1)
        loss = loss / update_freq
        last = (data_iter_step + 1) % update_freq == 0
        grad_norm = loss_scaler(loss, optimizer, clip_grad=max_norm if max_norm else None, parameters=params, update_grad=last)
        if grad_norms is not None:
            # What the reference sees in p.grad at this point (engine_for_frame_finetuning.py:170-174) differs by micro-step, and so does
            # what is collected: after an update step its scaler has unscaled and clipped the gradients in place, so the norms carry the
            # coefficient (here it stays on the device: the scaler's last_coef; 0 = the step was skipped there and nothing is added); on
            # the micro-steps in between (update_freq > 1) it sees the raw, still loss-scaled partial sums, i.e. coefficient 1.  Both
            # kinds of step enter the same average, as they do there.
            grad_norms.collect(getattr(loss_scaler, "last_coef", None) if last else None)
        if last:
            zero()
            if model_ema is not None:
                model_ema.update(model)
        if device.type == "cuda":
            torch.cuda.synchronize()
        stats["loss"].append(loss_value)
        stats["class_acc"].append(None if mixup_fn is not None else (output.max(-1)[-1] == targets).float().mean().item())
        stats["grad_norm"].append(None if grad_norm is None else float(grad_norm))
        stats["loss_scale"].append(loss_scaler.state_dict()["scale"])
        stats["lr"].append(max(g["lr"] for g in optimizer.param_groups))
        stats["min_lr"].append(min(g["lr"] for g in optimizer.param_groups))
        if log is not None:
            log(epoch, data_iter_step, stats)
    # gather the stats from all processes (engine_for_finetuning.py:137-140): per-step lists stay per rank, "averaged" is global
    stats["averaged"] = synchronize_meters(stats, device, group=dp.pg if dp is not None else None, names=METER_NAMES)
    if grad_norms is not None:
        stats["grad_norms"] = grad_norms.result(len(data_loader))  # (the reference's divisor, :245-248; the one read-back of the epoch)
    return stats


# ----------------------------------------------------------------------------------------------------------------- evaluation
def gather_predictions(tensors, world_size=None):
    """utils.gather_predictions_nontensor (utils.py:791-810) for lists of per-batch tensors: concatenate locally, all-gather the
    (equal-shaped or padded) result across ranks; single process: the local concatenation."""
    import torch.distributed as dist
    local = torch.cat([t.detach() for t in tensors], dim=0)
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return local
    world = dist.get_world_size()
    n = torch.tensor([local.shape[0]], device=local.device)
    sizes = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(sizes, n)
    m = int(max(int(s) for s in sizes))
    pad = torch.zeros((m,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    pad[: local.shape[0]] = local
    out = [torch.zeros_like(pad) for _ in range(world)]
    dist.all_gather(out, pad)
    return torch.cat([o[: int(s)] for o, s in zip(out, sizes)], dim=0)


@torch.no_grad()
def validation_one_epoch(data_loader, model, device, criterion=None, with_ttc=False, smoothed_labels_for_loss=False):
    """engine_for_frame_finetuning.validation_one_epoch (:282-383) without the plotting branches: eval-mode forward over the loader,
    loss and top-1 per batch, predictions gathered across ranks, then ``metrics.calculate_metrics``.  ``criterion`` (default: the
    reference's ``CrossEntropyLoss``), ``with_ttc`` and ``smoothed_labels_for_loss`` mean what they mean in ``train_one_epoch``
    (:302-318): the loss takes ``batch[3]["smoothed_labels"]`` / ``batch[3]["ttc"]``, accuracy and metrics the hard targets."""
    from . import metrics as M
    if criterion is None:
        criterion = torch.nn.CrossEntropyLoss()
    model.eval()
    preds, labels, losses, correct, seen = [], [], [], 0, 0
    for batch in data_loader:
        videos = batch[0].to(device, non_blocking=True)
        target = batch[1].to(device, non_blocking=True)
        output = model(videos)
        targets_loss, ttc = _loss_inputs(batch, target, device, with_ttc, smoothed_labels_for_loss)
        losses.append((criterion(output, targets_loss, ttc) if with_ttc else criterion(output, targets_loss)).item())
        correct += int((output.max(-1)[1] == target).sum())
        seen += videos.shape[0]
        preds.append(output.detach())
        labels.append(target.detach())
    all_preds, all_labels = gather_predictions(preds), gather_predictions(labels)
    acc, recall, precision, f1, confmat, auroc, ap, pr_curve, roc_curve, mcc = M.calculate_metrics(all_preds, all_labels)
    values = torch.nn.functional.softmax(all_preds, dim=1)[:, 1]
    my = {"metr_acc": acc, "recall": recall, "precision": precision, "f1": f1, "auroc": auroc, "ap": ap, "mcc_auc": mcc[0],
          "mcc_max": mcc[1], "mcc_max_thresh": mcc[2], "mcc_05": mcc[3],
          "logitsP_mean": all_preds[:, 1].mean().item(), "logitsP_std": all_preds[:, 1].std().item(),
          "logitsP_median": all_preds[:, 1].median().item(), "logitsN_mean": all_preds[:, 0].mean().item(),
          "logitsN_std": all_preds[:, 0].std().item(), "logitsN_median": all_preds[:, 0].median().item(),
          "probs_mean": values.mean().item(), "probs_std": values.std().item(), "probs_median": values.median().item()}
    return {"loss": float(np.mean(losses)), "acc": 100.0 * correct / max(seen, 1)}, my, {"confmat": confmat, "pr_curve": pr_curve, "roc_curve": roc_curve}


# ----------------------------------------------------------------------------------------------------------------- final test
PREDICTION_COLUMNS = ("clip", "filename", "logits_safe", "logits_risk", "label", "ttc")


def merge_prediction_shards(name_shards, logits, labels, ttc):
    """The table ``final_test`` writes, from what the ranks gathered: ``name_shards[r] = (clips, filenames)`` of rank r (what
    ``all_gather_object`` returns, rank after rank) and ``logits`` [S,2] / ``labels`` [S] / ``ttc`` [S], the rank-ordered concatenations
    ``gather_predictions`` returns.  Rows keep that order: rank 0's windows first.  Pure host code (tests/test_frame_store_cpu.py).
    Returns {column: list or numpy array} with the columns of PREDICTION_COLUMNS."""
    clips = [c for shard in name_shards for c in shard[0]]
    files = [f for shard in name_shards for f in shard[1]]
    for r, shard in enumerate(name_shards):
        if len(shard[0]) != len(shard[1]):
            raise ValueError(f"merge_prediction_shards: rank {r} sent {len(shard[0])} clip names but {len(shard[1])} file names")
    logits = logits.detach().to(torch.float32).cpu().numpy()
    labels = labels.detach().cpu().numpy().astype(int)
    ttc = ttc.detach().cpu().numpy()
    if logits.ndim != 2 or logits.shape[1] != 2 or not (len(clips) == logits.shape[0] == labels.shape[0] == ttc.shape[0]):
        raise ValueError(f"merge_prediction_shards: {len(clips)} names, logits {logits.shape}, labels {labels.shape}, ttc {ttc.shape}")
    return {"clip": clips, "filename": files, "logits_safe": logits[:, 0], "logits_risk": logits[:, 1], "label": labels, "ttc": ttc}


def write_predictions_csv(path, table) -> None:
    """``DataFrame(table).to_csv(path, index=True, header=True)`` with the csv module: an unnamed index column, then
    PREDICTION_COLUMNS.  Floats are written with ``repr`` of their exact value, so that parsing a float32 logit returns that float32."""
    import csv
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(("",) + PREDICTION_COLUMNS)
        for i in range(len(table["clip"])):
            w.writerow((i, table["clip"][i], table["filename"][i], repr(float(table["logits_safe"][i])), repr(float(table["logits_risk"][i])),
                        int(table["label"][i]), repr(float(table["ttc"][i]))))


@torch.no_grad()
def final_test(data_loader, model, device, preds_file, stats_file, plot_dir=None, with_ttc=False, smoothed_labels_for_loss=False,
               criterion=None, group_annotations=None, group_report_file=None):
    """engine_for_frame_finetuning.final_test (:385-545): run the model over the test windows, write ``preds_file`` (a CSV with an index
    column and clip, filename, logits_safe, logits_risk, label, ttc: the input of anaysis/metrics*.py) and ``stats_file`` (the five
    lines mAP / auroc / acc, P / R / F1 at 0.5, confusion matrix, from ``metrics.calculate_metrics``), return the global averages
    ``{"loss", "acc1"}`` (acc1 in percent, weighted by batch size; loss per batch, as the reference's meters count them).
    A batch is ``(videos, target, ids, extra_info)``: ``videos`` a clip tensor or a ``frame_store.FrameWindows`` (``StoreViews.batches``),
    ``extra_info`` a dict with ``ttc`` [B], ``clip`` and ``frame`` (B names each) and, for ``smoothed_labels_for_loss``, ``smoothed_labels``.
    ``criterion`` (default CrossEntropyLoss, the reference's), ``with_ttc`` and ``smoothed_labels_for_loss`` as in validation_one_epoch.
    Differences, by design: the plots are not built (``plot_dir`` is accepted and ignored with one warning); the reference reads
    ``output`` before it is assigned when no process group exists (:414) -- the labels collected are the targets in every case.
    With several ranks the tensors travel through ``gather_predictions``, the names through ``all_gather_object``; rank 0 writes.
    ``group_annotations`` (default None: nothing more is written): ``{"clip_lvl_cat": {clip name: category code}, "clip_lvl_ego":
    {clip name: bool}}`` and optionally ``"cat_codes"`` -- rank 0 then also writes ``metrics.group_report`` of the logits it gathered
    (the group_metrics.txt of anaysis/metrics_dota.py) to ``group_report_file`` (default: group_metrics.txt next to ``preds_file``)."""
    import torch.distributed as dist
    from . import metrics as M
    if group_report_file is not None and group_annotations is None:
        raise ValueError("final_test: group_report_file needs group_annotations")
    if plot_dir is not None:
        import warnings
        warnings.warn("final_test: the PR / ROC plots of the reference are not built; plot_dir is ignored")
    if criterion is None:
        criterion = torch.nn.CrossEntropyLoss()
    model.eval()
    clips, frame_names, preds, labels, ttcs = [], [], [], [], []
    loss_sum, n_batches, correct, seen = 0.0, 0, 0, 0
    for batch in data_loader:
        videos = batch[0].to(device, non_blocking=True)
        target = batch[1].to(device, non_blocking=True)
        extra_info = batch[3]
        clips.extend(extra_info["clip"])
        frame_names.extend(extra_info["frame"])
        labels.append(target.detach())
        ttcs.append(torch.as_tensor(extra_info["ttc"]).clone().detach().to(device, non_blocking=True))
        targets_loss, ttc = _loss_inputs(batch, target, device, with_ttc, smoothed_labels_for_loss)
        output = model(videos)
        loss = criterion(output, targets_loss, ttc) if with_ttc else criterion(output, targets_loss)
        preds.append(output.detach())
        loss_sum += loss.item()
        n_batches += 1
        correct += int((output.max(-1)[1] == target).sum())
        seen += int(videos.shape[0])
    distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    all_preds, all_labels, all_ttcs = gather_predictions(preds), gather_predictions(labels), gather_predictions(ttcs)
    name_shards = [(clips, frame_names)]
    meters = torch.tensor([loss_sum, n_batches, correct, seen], dtype=torch.float64)
    if distributed:
        name_shards = [None] * dist.get_world_size()
        dist.all_gather_object(name_shards, (clips, frame_names))
        if dist.get_backend() == "nccl":
            meters = meters.to(device)
        dist.all_reduce(meters)
        meters = meters.cpu()
    if not distributed or dist.get_rank() == 0:
        table = merge_prediction_shards(name_shards, all_preds, all_labels, all_ttcs)
        acc, recall, precision, f1, confmat, auroc, ap, _, _, _ = M.calculate_metrics(all_preds.float(), all_labels)
        lines = ["\n===================================",
                 f"mAP: {ap}, auroc: {auroc}, acc: {acc}",
                 f"P@0.5: {precision}, R@0.5: {recall}, F1@0.5: {f1}",
                 f"Confmat: \n\t{confmat[0][0]} | {confmat[0][1]} \n\t{confmat[1][0]} | {confmat[1][1]}",
                 "----------------------------"]
        with open(stats_file, "w") as f:
            for line in lines:
                f.write(line + "\n")
                print(line)
        write_predictions_csv(preds_file, table)
        if group_annotations is not None:
            cat, ego = group_annotations["clip_lvl_cat"], group_annotations["clip_lvl_ego"]
            report = M.group_report(torch.softmax(all_preds.float(), dim=1)[:, 1], all_labels, table["clip"],
                                    clip_lvl_cat=[cat[c] for c in table["clip"]], clip_lvl_ego=[bool(ego[c]) for c in table["clip"]],
                                    cat_codes=group_annotations.get("cat_codes", M.DOTA_CAT_CODES))
            with open(group_report_file or os.path.join(os.path.dirname(preds_file), "group_metrics.txt"), "w") as f:
                f.write("\n".join(report))
    result = {"loss": float(meters[0] / max(float(meters[1]), 1.0)), "acc1": float(100.0 * meters[2] / max(float(meters[3]), 1.0))}
    print("* Acc@1 {:.3f} loss {:.3f}".format(result["acc1"], result["loss"]))
    return result
