"""Mixup / CutMix of the fine-tune loop: counterpart of the reference's ``mixup.Mixup`` (mixup.py:90-218, timm's), which
``run_class_finetuning.py`` builds by default (``--mixup 0.8 --cutmix 1.0 --smoothing 0.1``, :300-307, :449-456) and
``engine_for_finetuning.train_one_epoch`` applies to every batch on the device (:59-60).

Same surface -- constructor arguments, attribute names, ``__call__(x, target) -> (x, soft_target)``, modes ``batch`` / ``pair`` /
``elem`` -- and the same results bit for bit, but the work is split differently.  One host routine (``Mixup.plan``) turns the random
draws into a per-sample plan: keep, blend with two coefficients, or paste a box of the partner ``B-1-i``.  A contiguous f32 clip batch
on the GPU is then mixed in place by ONE HIP launch (``tad_mixup_clips``: each element pair read once and written once, no copy of the
batch) and its soft targets come from one more (``tad_mixup_target``); the plan reaches the device through pinned memory, so a call
never waits for the GPU.  Anything else (CPU tensors, other dtypes, non-contiguous views) is mixed by the torch expressions below,
which state the same plan and are what the CPU tests compare with the reference.

RNG contract.  The draws come from numpy's GLOBAL stream, in the reference's order and with its calls, so a script seeded like the
reference mixes the same way:
* ``batch`` (mixup.py:141-157, :196-207): ``rand()`` against ``prob`` (only while ``mixup_enabled``); with both alphas positive
  ``rand()`` against ``switch_prob``; one ``beta(a, a)`` of the chosen kind; for CutMix then the box draws.
* ``elem`` / ``pair`` (mixup.py:121-139, n = B or B/2): with both alphas ``rand(n)``, ``beta(cutmix_alpha, .., size=n)``,
  ``beta(mixup_alpha, .., size=n)`` (both always drawn); else one ``beta(.., size=n)``; then ``rand(n)`` against ``prob``; lam is kept as
  float32.  Box draws follow per sample, in index order, for the samples that cut.
* box (mixup.py:30-87): ``randint(0, H, size=None)``, ``randint(0, W, size=None)`` for the centre of a
  ``int(H * sqrt(1 - lam)) x int(W * sqrt(1 - lam))`` box cut to the image, or with ``cutmix_minmax`` the four draws
  ``randint(int(H * lo), int(H * hi))``, ``randint(int(W * lo), int(W * hi))``, ``randint(0, H - h)``, ``randint(0, W - w)``.
  With ``correct_lam`` (or min/max) lam becomes ``1 - area / (H * W)``.

Coefficients.  ``batch`` blends with ``lam`` and ``1.0 - lam`` taken in double and rounded to the clip's dtype (mixup.py:205-206);
``pair`` / ``elem`` with the float32 ``lam`` and the float32 difference ``1 - lam`` (mixup.py:173, :191-192).  Each result is
``fl(fl(x_i * w_self) + fl(x_j * w_other))`` of the ORIGINAL values, three roundings, on both paths.

Pair-mode quirk (mixup.py:187-188).  The reference indexes a sample as ``x[i][:, yl:yh, xl:xh]``: on a video sample [C,T,H,W] the box
drawn for (H, W) therefore lands on the T and H axes over the whole width, its T range cut to T by the slice, while lam stays the
(H, W) area ratio.  ``batch`` and ``elem`` index with ``...`` and cut H and W.  This is reproduced, and it is why a plan's box has
three axes.
"""
from __future__ import annotations

import numpy as np
import torch

from . import kernels as K
from ._lib import MIX_BLEND, MIX_KEEP, MIX_PASTE

_WHOLE = None  # box placeholder of the kinds that have none


def _smoothed_rows(labels, num_classes, on_value, off_value, device):
    labels = labels.long().reshape(-1)
    rows = torch.full((labels.numel(), num_classes), off_value, device=device)
    rows[torch.arange(labels.numel(), device=device), labels.to(device)] = on_value
    return rows


def mixup_target(target, num_classes, lam=1., smoothing=0.0, device='cuda'):
    """mixup.py:22-27: the smoothed one-hot rows of ``target`` and of ``target.flip(0)`` weighted by lam and 1 - lam (a float, or a
    [B,1] tensor of per-sample values); ``off = smoothing / num_classes``, ``on = 1 - smoothing + off`` in double, stored as f32"""
    off_value = smoothing / num_classes
    on_value = 1. - smoothing + off_value
    first = _smoothed_rows(target, num_classes, on_value, off_value, device)
    second = _smoothed_rows(target.flip(0), num_classes, on_value, off_value, device)
    return first * lam + second * (1. - lam)


def _draw_box(height, width, lam, minmax, correct_lam):
    """one CutMix box over (height, width) from the global numpy stream -> (lo_h, hi_h, lo_w, hi_w), lam"""
    if minmax is not None:
        assert len(minmax) == 2
        box_h = np.random.randint(int(height * minmax[0]), int(height * minmax[1]), size=None)
        box_w = np.random.randint(int(width * minmax[0]), int(width * minmax[1]), size=None)
        lo_h = np.random.randint(0, height - box_h, size=None)
        lo_w = np.random.randint(0, width - box_w, size=None)
        hi_h, hi_w = lo_h + box_h, lo_w + box_w
    else:
        side = np.sqrt(1 - lam)  # (in lam's own precision: float32 for the per-sample modes)
        box_h, box_w = int(height * side), int(width * side)
        mid_h = np.random.randint(0, height, size=None)
        mid_w = np.random.randint(0, width, size=None)
        lo_h, hi_h = np.clip(mid_h - box_h // 2, 0, height), np.clip(mid_h + box_h // 2, 0, height)
        lo_w, hi_w = np.clip(mid_w - box_w // 2, 0, width), np.clip(mid_w + box_w // 2, 0, width)
    if correct_lam or minmax is not None:
        lam = 1. - ((hi_h - lo_h) * (hi_w - lo_w)) / float(height * width)
    return (int(lo_h), int(hi_h), int(lo_w), int(hi_w)), lam


class Mixup:
    """mixup.py:90-119.  mixup_alpha / cutmix_alpha: Beta parameters, a kind is active when positive; cutmix_minmax: box sides as a
    (lo, hi) share of the image instead of the Beta draw (forces cutmix_alpha = 1); prob: chance that a batch / sample is mixed at all;
    switch_prob: chance of CutMix when both kinds are active; mode: 'batch' (one draw for the batch), 'pair' (one per pair (i, B-1-i)),
    'elem' (one per sample); correct_lam: lam = the share of the image the cut box leaves; label_smoothing, num_classes: of the
    soft target.  ``mixup_enabled = False`` (set by a training loop) switches the mixing off."""

    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch', correct_lam=True,
                 label_smoothing=0.1, num_classes=1000):
        self.mixup_alpha = mixup_alpha
        self.cutmix_alpha = cutmix_alpha
        self.cutmix_minmax = cutmix_minmax
        if cutmix_minmax is not None:
            assert len(cutmix_minmax) == 2
            self.cutmix_alpha = 1.0
        self.mix_prob = prob
        self.switch_prob = switch_prob
        self.label_smoothing = label_smoothing
        self.num_classes = num_classes
        self.mode = mode
        self.correct_lam = correct_lam
        self.mixup_enabled = True

    # ------------------------------------------------------------------ the random draws
    def _kinds(self):
        both = self.mixup_alpha > 0. and self.cutmix_alpha > 0.
        assert both or self.mixup_alpha > 0. or self.cutmix_alpha > 0., \
            "One of mixup_alpha > 0., cutmix_alpha > 0., cutmix_minmax not None should be true."
        return both

    def _draw_batch(self):
        """-> (lam as a Python float, CutMix?) for the whole batch"""
        if not (self.mixup_enabled and np.random.rand() < self.mix_prob):
            return 1., False
        cut = self.cutmix_alpha > 0.
        if self._kinds():
            cut = np.random.rand() < self.switch_prob
        alpha = self.cutmix_alpha if cut else self.mixup_alpha
        return float(np.random.beta(alpha, alpha)), bool(cut)

    def _draw_each(self, n):
        """-> (lam float32 [n], CutMix? bool [n]) for n samples or pairs"""
        lam = np.ones(n, dtype=np.float32)
        cut = np.zeros(n, dtype=bool)
        if not self.mixup_enabled:
            return lam, cut
        if self._kinds():
            cut = np.random.rand(n) < self.switch_prob
            for_cut = np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=n)
            for_blend = np.random.beta(self.mixup_alpha, self.mixup_alpha, size=n)
            drawn = np.where(cut, for_cut, for_blend)
        elif self.mixup_alpha > 0.:
            drawn = np.random.beta(self.mixup_alpha, self.mixup_alpha, size=n)
        else:
            cut = np.ones(n, dtype=bool)
            drawn = np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=n)
        mixed = np.random.rand(n) < self.mix_prob
        return np.where(mixed, drawn.astype(np.float32), lam), cut

    def plan(self, shape):
        """Consume the random draws for a batch of ``shape`` = [B,C,T,H,W] (or [B,C,H,W]) and return ``(rows, lam)``:
        rows[i] = (kind, w_self, w_other, (t0, t1, y0, y1, x0, x1)) for sample i with partner B-1-i -- coefficients in the precision the
        reference holds them in (Python float for 'batch', numpy float32 otherwise) -- and lam = the soft target's weight: a Python
        float ('batch') or a float32 array [B]."""
        B = int(shape[0])
        assert B % 2 == 0, 'Batch size should be even when using this'
        video = len(shape) == 5
        T = int(shape[2]) if video else 1
        H, W = int(shape[-2]), int(shape[-1])
        keep = (MIX_KEEP, 1., 0., _WHOLE)
        if self.mode not in ('elem', 'pair'):
            lam, cut = self._draw_batch()
            if lam == 1.:
                return [keep] * B, 1.
            if cut:
                (y0, y1, x0, x1), lam = _draw_box(H, W, lam, self.cutmix_minmax, self.correct_lam)
                return [(MIX_PASTE, 0., 1., (0, T, y0, y1, x0, x1))] * B, lam
            return [(MIX_BLEND, lam, 1. - lam, _WHOLE)] * B, lam
        pair = self.mode == 'pair'
        n = B // 2 if pair else B
        lams, cuts = self._draw_each(n)
        rows = [keep] * B
        for i in range(n):
            lam = lams[i]
            if lam == 1.:
                continue
            if cuts[i]:
                (a0, a1, b0, b1), lam = _draw_box(H, W, lam, self.cutmix_minmax, self.correct_lam)
                if pair and video:  # the box indexes the two axes behind the channel axis: T and H, all of W (see the module docstring)
                    box = (min(a0, T), min(a1, T), min(b0, H), min(b1, H), 0, W)
                else:
                    box = (0, T, a0, a1, b0, b1)
                row = (MIX_PASTE, 0., 1., box)
                lams[i] = lam
            else:
                row = (MIX_BLEND, lam, 1 - lam, _WHOLE)
            rows[i] = row
            if pair:
                rows[B - 1 - i] = row
        if pair:
            lams = np.concatenate((lams, lams[::-1]))
        return rows, lams

    # ------------------------------------------------------------------ the two ways to carry a plan out
    @staticmethod
    def _fused(x, target):
        return (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() in (4, 5) and x.numel() > 0
                and isinstance(target, torch.Tensor) and target.device == x.device and not target.is_floating_point())

    def _mix_torch(self, x, rows):
        """the plan as torch expressions, in place (any device, dtype and layout)"""
        if all(r[0] == MIX_KEEP for r in rows):
            return
        B = len(rows)
        v = x if x.dim() == 5 else x.unsqueeze(2)
        was = v.clone()
        for i, (kind, w_self, w_other, box) in enumerate(rows):
            j = B - 1 - i
            if kind == MIX_BLEND:
                v[i] = was[i] * w_self + was[j] * w_other
            elif kind == MIX_PASTE:
                t0, t1, y0, y1, x0, x1 = box
                v[i][:, t0:t1, y0:y1, x0:x1] = was[j][:, t0:t1, y0:y1, x0:x1]

    def _mix_hip(self, x, target, rows, lam):
        B = len(rows)
        v = x if x.dim() == 5 else x.unsqueeze(2)
        T, H, W = v.shape[2:]
        f32 = np.float32
        if isinstance(lam, float):
            t_self, t_other = [f32(lam)] * B, [f32(1. - lam)] * B
        else:
            t_self, t_other = lam.astype(f32), f32(1) - lam.astype(f32)
        table = K.mixup_plan_table([(kind, f32(ws), f32(wo), (0, T, 0, H, 0, W) if box is None else box, t_self[i], t_other[i])
                                    for i, (kind, ws, wo, box) in enumerate(rows)], T, H, W)
        with torch.cuda.device(x.device):
            # pinned staging + asynchronous copy: the host never waits for the device (the caching host allocator keeps the staging
            # block alive until the copy has run)
            plan = table.pin_memory().to(x.device, non_blocking=True)
            if any(r[0] != MIX_KEEP for r in rows):
                K.mixup_clips(v, plan)
                torch.autograd.graph.increment_version(x)  # (raw-pointer write: tell autograd as an in-place op would)
            off_value = self.label_smoothing / self.num_classes
            on_value = 1. - self.label_smoothing + off_value
            labels = target.reshape(-1)
            return K.mixup_target(plan, labels if labels.dtype == torch.int64 else labels.long(), self.num_classes, on_value, off_value)

    def __call__(self, x, target):
        assert len(x) % 2 == 0, 'Batch size should be even when using this'
        if x.dim() not in (4, 5):
            raise ValueError(f"Mixup: expected [B,C,T,H,W] clips or [B,C,H,W] images, got {tuple(x.shape)}")
        rows, lam = self.plan(x.shape)
        if self._fused(x, target):
            return x, self._mix_hip(x, target, rows, lam)
        with torch.no_grad():
            self._mix_torch(x, rows)
        if not isinstance(lam, float):
            lam = torch.tensor(lam, device=x.device, dtype=x.dtype).unsqueeze(1)
        return x, mixup_target(target, self.num_classes, lam, self.label_smoothing, x.device)
