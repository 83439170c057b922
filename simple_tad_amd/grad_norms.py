"""Per-head gradient-norm diagnostics: ``utils.collect_grad_norms`` / ``collect_grad_norms_pretrain`` (utils.py:813-1011) and the
per-epoch averages the reference's engines keep of them (engine_for_frame_finetuning.py:76-83, 173-185, 232-251;
engine_for_pretraining.py:30-33, 84-91, 134-147), which its run scripts write to ``grad_norms/gradnorm_ep{epoch}.npz``.

The reference calls ``.norm().item()`` once per attention head (the Q, K, V slices of ``qkv.weight.grad.view(3, H, hd, D)``, the
q and v bias slices) and once per proj / fc1 / fc2 weight and bias and patch-embedding tensor: 794 kernels and host syncs per step of
a ViT-B.  Here every gradient is a view of ONE flat buffer (``flat.FlatSpace``), every slice the reference looks at is a contiguous
run of it, and the whole table is one segmented sum-of-squares pass (``tad_grad_segnorm``, csrc/grad_segnorm.hip): two launches, no
host sync; the per-step values accumulate on the device and are read once, at the end of the epoch.

Column order (the reference's):  qkv [L,H,5] = [Wq, Wk, Wv, q_bias, v_bias];  proj [L,6] = [proj.w, proj.b, fc1.w, fc1.b, fc2.w,
fc2.b];  patch_embed [2] = [patch.w, patch.b].  A frozen or absent parameter (``--freeze_layers``, ``qkv_bias=False``) has no
segment: its slot stays 0, which is what the reference writes there.

Non-finite values: the reference ends with ``np.nan_to_num``.  Its NaN -> 0 is kept (a non-finite norm adds 0 and is counted in
``nonfinite_values``); its inf -> 1.8e308 is deliberately NOT reproduced -- one overflowed step would own the epoch average.
There is no CPU path: ``collect`` needs the flat gradient buffer on the GPU.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import kernels as K
from ._lib import TadError
from .parallel import DataParallel

QKV_COLUMNS = ("Wq", "Wk", "Wv", "q_bias", "v_bias")
PROJ_COLUMNS = ("proj.w", "proj.b", "fc1.w", "fc1.b", "fc2.w", "fc2.b")
PATCH_COLUMNS = ("patch.w", "patch.b")
KEYS = ("qkv", "proj", "patch_embed")
COUNTERS = ("steps_added", "steps_skipped", "nonfinite_values")


class SegmentTable(NamedTuple):
    segments: List[Tuple[int, int, int]]     # (offset, length, slot) in floats of the flat gradient buffer
    slots: Dict[tuple, int]                  # ("qkv", l, h, c) / ("proj", l, c) / ("patch_embed", c) -> slot, with or without a segment
    shapes: Dict[str, tuple]                 # {"qkv": (L, H, 5), "proj": (L, 6), "patch_embed": (2,)}


class GradNorms(dict):
    """the reference's dict {"qkv", "proj", "patch_embed"} (``np.savez(path, **result)`` as it stands); ``counters`` rides along"""
    counters: Dict[str, int] = {}


def encoder_of(model):
    """the module whose ``blocks`` / ``patch_embed`` the reference walks: ``model``, without a DataParallel wrapper, or its
    ``encoder`` for the pre-training wrapper"""
    m = model.module if isinstance(model, DataParallel) else model
    enc = getattr(m, "encoder", None)
    return enc if enc is not None and hasattr(enc, "blocks") else m


def segment_table(model, space, num_heads: Optional[int] = None) -> SegmentTable:
    """The host-side layout: one (offset, length, slot) segment per slice of ``space``'s flat buffer the reference takes a norm of.
    ``space``: a ``flat.FlatSpace`` (anything with ``offset[id(p)]`` and ``p in space``).  Pure Python."""
    enc = encoder_of(model)
    H = int(num_heads if num_heads is not None else enc.num_heads)
    L = len(enc.blocks)
    shapes = {"qkv": (L, H, 5), "proj": (L, 6), "patch_embed": (2,)}
    proj0, patch0 = L * H * 5, L * H * 5 + L * 6
    slots = {("qkv", l, h, c): (l * H + h) * 5 + c for l in range(L) for h in range(H) for c in range(5)}
    slots.update({("proj", l, c): proj0 + l * 6 + c for l in range(L) for c in range(6)})
    slots.update({("patch_embed", c): patch0 + c for c in range(2)})
    segments = []

    def live(p):
        return p is not None and p.requires_grad and p in space

    def whole(p, slot):
        if live(p):
            segments.append((space.offset[id(p)], p.numel(), slot))

    pe = getattr(enc.patch_embed, "proj", None)
    if pe is not None:
        whole(pe.weight, slots[("patch_embed", 0)])
        whole(pe.bias, slots[("patch_embed", 1)])
    for l, blk in enumerate(enc.blocks):
        a = blk.attn
        w = a.qkv.weight
        if live(w):
            if w.shape[0] % (3 * H):
                raise TadError(f"segment_table: qkv.weight {tuple(w.shape)} does not split into 3 x {H} heads")
            per = w.shape[0] // (3 * H) * w.shape[1]        # one head's slice of .view(3, H, hd, D)[i, h]: hd * D contiguous floats
            o = space.offset[id(w)]
            for h in range(H):
                for i in range(3):
                    segments.append((o + (i * H + h) * per, per, slots[("qkv", l, h, i)]))
        for c, b in ((3, getattr(a, "q_bias", None)), (4, getattr(a, "v_bias", None))):
            if live(b):
                if b.numel() % H:
                    raise TadError(f"segment_table: a bias of {b.numel()} elements does not split into {H} heads")
                hd = b.numel() // H
                for h in range(H):
                    segments.append((space.offset[id(b)] + h * hd, hd, slots[("qkv", l, h, c)]))
        for c, p in enumerate((a.proj.weight, a.proj.bias, blk.mlp.fc1.weight, blk.mlp.fc1.bias, blk.mlp.fc2.weight, blk.mlp.fc2.bias)):
            whole(p, slots[("proj", l, c)])
    return SegmentTable(segments, slots, shapes)


class _GradSpace:
    """the flat layout read off the gradients themselves (each ``p.grad`` a view of ONE 1-D f32 buffer), for callers that hold the
    model alone: the one-shot functions with the reference's signatures"""

    def __init__(self, enc):
        self.offset, self.flat_grad = {}, None
        for p in enc.parameters():
            g = p.grad
            if g is None or not p.requires_grad:
                continue
            base = g._base
            if base is None or base.dim() != 1 or base.dtype != torch.float32 or not g.is_contiguous() or \
                    (self.flat_grad is not None and base is not self.flat_grad):
                raise TadError("grad_norms: the gradients are not views of one flat buffer (optim.FusedAdamW or parallel.DataParallel "
                               "lays them out that way; there is no per-tensor path)")
            self.flat_grad = base
            self.offset[id(p)] = g.storage_offset() - base.storage_offset()
        if self.flat_grad is None:
            raise TadError("grad_norms: no parameter of the model holds a gradient")

    def __contains__(self, p):
        return id(p) in self.offset


def _space_of(model, optimizer_or_space):
    x = optimizer_or_space
    if x is None:
        return model.space if isinstance(model, DataParallel) else _GradSpace(encoder_of(model))
    if hasattr(x, "offset") and hasattr(x, "flat_grad"):
        space = x
    elif hasattr(getattr(x, "space", None), "offset"):
        space = x.space
    elif isinstance(model, DataParallel):
        space = model.space
    else:
        raise TadError(f"grad_norms: {type(x).__name__} keeps no flat gradient buffer: the gradients are not views of one flat buffer "
                       "(use optim.FusedAdamW or parallel.DataParallel; there is no per-tensor path)")
    if space.flat_grad is None:
        raise TadError("grad_norms: the flat space holds no gradient buffer yet (FlatSpace.ensure_grads)")
    return space


class GradNormCollector:
    """Builds the segment and work tables of ``model`` over the flat gradient buffer once (device copies through pinned memory) and owns
    the device-side state: ``acc`` f64 [slots], ``last`` f32 [slots], ``counters`` int32 {steps_added, steps_skipped, nonfinite_values}.

    ``collect(coef)`` launches (no host sync); ``result(steps)`` reads back once; ``reset()`` zeroes the accumulators.
    ``optimizer_or_space``: an ``optim.FusedAdamW``, a ``flat.FlatSpace``, or None (a DataParallel model's own space, else the layout
    is read off the gradients).  ``group``: the process group ``result`` sums over (default: a DataParallel model's, else the default)."""

    def __init__(self, model, optimizer_or_space=None, num_heads: Optional[int] = None, group=None):
        space = _space_of(model, optimizer_or_space)
        self.flat_grad = space.flat_grad
        self.layout = segment_table(model, space, num_heads)
        if not self.layout.segments:
            raise TadError("grad_norms: none of the tensors the diagnostics look at is trainable")
        self.nslots = len(self.layout.slots)
        self.group = group if group is not None else (model.pg if isinstance(model, DataParallel) else None)
        table, work = K.grad_segnorm_tables(self.layout.segments, self.flat_grad.numel(), self.nslots)  # (plan-checked here, once)
        dev = self.flat_grad.device
        if dev.type == "cuda":
            table, work = table.pin_memory().to(dev, non_blocking=True), work.pin_memory().to(dev, non_blocking=True)
        self.table, self.work = table, work
        # acc and the counters share one allocation so that result() is ONE copy to the host: [slots] f64, then 3 int32 (+ 1 pad)
        self._state = torch.zeros(self.nslots + 2, dtype=torch.float64, device=dev)
        self.acc = self._state[:self.nslots]
        self.counters = self._state[self.nslots:].view(torch.int32)[:3]
        self.last = torch.zeros(self.nslots, dtype=torch.float32, device=dev)

    def collect(self, coef: Optional[torch.Tensor] = None) -> None:
        """add this step: ``last = coef * norms``, ``acc += last``.  ``coef``: a device f32 tensor of one element (the scaler's
        unscale-and-clip coefficient; 0 = the step was skipped on the device, nothing is added) or None (1.0)"""
        K.grad_segnorm(self.flat_grad, self.table, self.work, self.acc, self.last, self.counters, coef)

    def reset(self) -> None:
        self._state.zero_()
        self.last.zero_()

    def _read_back(self) -> torch.Tensor:
        """the one device-to-host copy: acc and the counters"""
        return self._state.cpu()

    def _arrays(self, flat: np.ndarray) -> GradNorms:
        L, H, _ = self.layout.shapes["qkv"]
        a, b = L * H * 5, L * H * 5 + L * 6
        return GradNorms(qkv=flat[:a].reshape(L, H, 5).copy(), proj=flat[a:b].reshape(L, 6).copy(), patch_embed=flat[b:b + 2].copy())

    def result(self, steps: int) -> GradNorms:
        """{"qkv" [L,H,5], "proj" [L,6], "patch_embed" [2]}: float64 numpy, the accumulated norms divided by ``steps`` (normally
        ``len(data_loader)``, the reference's divisor); ``.counters`` = {steps_added, steps_skipped, nonfinite_values}.  With an
        initialised process group of more than one rank the tables (and the counters) are summed over the ranks before the division,
        as the reference's gather + ``np.sum(axis=0)`` does (engine_for_frame_finetuning.py:232-240)."""
        import torch.distributed as dist
        host = self._read_back()
        packed = torch.cat((host[:self.nslots], host[self.nslots:].view(torch.int32)[:3].double()))
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            if dist.get_backend(self.group) == "nccl":
                packed = packed.to(self.flat_grad.device)
            dist.all_reduce(packed, group=self.group)
            packed = packed.cpu()
        out = self._arrays(packed[:self.nslots].numpy() / float(steps))
        out.counters = {k: int(v) for k, v in zip(COUNTERS, packed[self.nslots:].tolist())}
        return out

    def last_step(self) -> GradNorms:
        """this step's norms alone (a read-back: for the one-shot functions and for tests, not for the training loop)"""
        out = self._arrays(self.last.cpu().double().numpy())
        out.counters = {}
        return out


def _one_shot(model):
    c = GradNormCollector(model)
    c.collect()
    r = c.result(1)
    return r["qkv"], r["proj"], r["patch_embed"]


def collect_grad_norms(model, num_layers=12, num_heads=6):
    """utils.collect_grad_norms (utils.py:813-913): (qkv [L,H,5], proj [L,6], patch_embed [2]) float64 numpy of the gradients ``model``
    holds now.  ``num_layers`` / ``num_heads`` are ignored, as the reference ignores them (it reads ``len(model.blocks)`` and
    ``model.num_heads``).  One collect and one read-back; a training loop keeps a ``GradNormCollector`` instead.  A non-finite norm reads
    0 (the reference: NaN -> 0, inf -> 1.8e308)."""
    return _one_shot(model)


def collect_grad_norms_pretrain(model, num_layers=12, num_heads=6):
    """utils.collect_grad_norms_pretrain (utils.py:916-1011): the same over ``model.encoder`` of the pre-training wrapper"""
    return _one_shot(model)
