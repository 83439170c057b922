"""Weight EMA of the fine-tuning loop: counterpart of ``timm.utils.ModelEma`` (timm 0.4.12), which the reference builds for
``--model_ema`` (run_frame_finetuning.py:487-494, run_class_finetuning.py:395-402), updates after every completed optimizer step
(engine_for_finetuning.py:98-99) and saves as ``checkpoint['model_ema']`` (utils.py:450-470).

Same surface and the same arithmetic, ``ema_v.copy_(ema_v * decay + (1. - decay) * model_v)`` for every state-dict entry, but every
f32 pair resident on one GPU goes through ONE HIP launch for the whole model (``tad_ema_update``: 12 B per element, bit-identical
to the torch expression).  Any other entry (a CPU copy for ``--model_ema_force_cpu``, a non-f32 buffer) takes the reference's torch
expression itself.

Two rules keep the fused path correct:
* the device table of addresses is rebuilt whenever an address or a size changes -- the reference builds the EMA before the
  optimizer, and ``FusedAdamW`` then moves every parameter into its flat buffer;
* the kernel writes through raw pointers, so the version counters of the EMA tensors are bumped afterwards as ``copy_`` would have
  done: the cached 16-bit weight copies (``ops._wcache``) and the captured graphs of ``inference.SlidingWindow`` are keyed on them.
"""
from __future__ import annotations

from collections import OrderedDict
from copy import deepcopy

import torch

from . import kernels as K
from ._lib import TadError


def _fused(ema_v: torch.Tensor, model_v: torch.Tensor) -> bool:
    return (ema_v.is_cuda and ema_v.dtype == torch.float32 and model_v.dtype == torch.float32 and model_v.device == ema_v.device
            and ema_v.shape == model_v.shape and ema_v.is_contiguous() and model_v.is_contiguous())


class _Plan:
    """device table of one set of f32 pairs on one GPU (kernels.ema_table), reused while the addresses and sizes stay the same"""

    def __init__(self, sig, device):
        buf, self.n_tensors, self.n_chunks = K.ema_table([sig[i:i + 3] for i in range(0, len(sig), 3)])
        self.sig = sig
        self.n_elements = sum(sig[2::3])
        self.table = buf.to(device)

    def run(self, decay: float):
        K.ema_update(self.table, self.n_tensors, self.n_chunks, decay, self.n_elements)


def update_tensors_(ema_tensors, model_tensors, decay: float, plan: _Plan = None) -> _Plan:
    """ema = ema * decay + (1 - decay) * model over contiguous f32 tensor pairs on one GPU, ONE launch; bumps the version counters
    of ``ema_tensors``.  Pass the returned plan back in to skip rebuilding the table while the tensors stay where they are."""
    ema_tensors, model_tensors = list(ema_tensors), list(model_tensors)
    if len(ema_tensors) != len(model_tensors) or not ema_tensors:
        raise ValueError("update_tensors_: need as many model tensors as EMA tensors, at least one")
    device = ema_tensors[0].device
    sig = []
    for e, m in zip(ema_tensors, model_tensors):
        if not _fused(e, m) or e.device != device:
            raise TadError("update_tensors_: expected contiguous f32 pairs of equal shape on one GPU")
        if e.numel():
            sig += (e.data_ptr(), m.data_ptr(), e.numel())
    if not sig:
        return plan
    sig = tuple(sig)
    with torch.cuda.device(device):
        if plan is None or plan.sig != sig:
            plan = _Plan(sig, device)
        plan.run(decay)
    torch.autograd.graph.increment_version(ema_tensors)
    return plan


class ModelEma:
    """timm.utils.ModelEma: keeps ``ema`` = a moving average of the model's state dict, ``ema = decay * ema + (1 - decay) * model``
    after every optimizer step.  ``device``: keep the copy there instead (``'cpu'`` for ``--model_ema_force_cpu``); ``resume``: a
    checkpoint to restore the average from (``_load_checkpoint``)."""

    def __init__(self, model, decay=0.9999, device='', resume=''):
        self.ema = deepcopy(model)
        self.ema.eval()
        self.decay = decay
        self.device = device
        if device:
            self.ema.to(device=device)
        self.ema_has_module = hasattr(self.ema, 'module')
        if resume:
            self._load_checkpoint(resume)
        for p in self.ema.parameters():
            p.requires_grad_(False)
        self._plans = {}  # device -> _Plan

    def _load_checkpoint(self, checkpoint_path):
        """timm's loader: a path or file object of a checkpoint holding ``'state_dict_ema'`` (``module.`` added to the keys when the
        EMA module has one).  Unlike timm, an already loaded object is accepted too, and so is a BARE state dict -- what
        ``utils.auto_load_model`` hands over (``checkpoint['model_ema']``, utils.py:229-236), which timm ignores for lack of the key."""
        checkpoint = checkpoint_path if isinstance(checkpoint_path, dict) else torch.load(checkpoint_path, map_location='cpu')
        assert isinstance(checkpoint, dict)
        if 'state_dict_ema' in checkpoint:
            sd = checkpoint['state_dict_ema']
        elif checkpoint and all(isinstance(v, torch.Tensor) for v in checkpoint.values()):
            sd = checkpoint
        else:
            print("Failed to find state_dict_ema, starting from loaded model weights")
            return
        new_state_dict = OrderedDict()
        for k, v in sd.items():
            new_state_dict[('module.' + k if not k.startswith('module') else k) if self.ema_has_module else k] = v
        self.ema.load_state_dict(new_state_dict)

    @torch.no_grad()
    def update(self, model):
        needs_module = hasattr(model, 'module') and not self.ema_has_module
        msd = model.state_dict(keep_vars=True)
        groups = {}  # device -> ([ema tensors], [model tensors]) of the fused path
        seen = set()  # (an entry sharing its storage with an earlier one -- tied weights -- is updated once more, as in the reference,
        for k, ema_v in self.ema.state_dict(keep_vars=True).items():  # but not by a second workgroup of the same launch)
            if needs_module:
                k = 'module.' + k
            model_v = msd[k]
            if _fused(ema_v, model_v) and ema_v.data_ptr() not in seen:
                seen.add(ema_v.data_ptr())
                g = groups.get(ema_v.device)
                if g is None:
                    g = groups[ema_v.device] = ([], [])
                g[0].append(ema_v)
                g[1].append(model_v)
                continue
            # the reference's expression, bit-identical by construction (CPU copy, non-f32 or non-contiguous entries)
            ema_v, model_v = ema_v.detach(), model_v.detach()
            if self.device:
                model_v = model_v.to(device=self.device)
            ema_v.copy_(ema_v * self.decay + (1. - self.decay) * model_v)
        for dev, (es, ms) in groups.items():
            self._plans[dev] = update_tensors_(es, ms, self.decay, self._plans.get(dev))
