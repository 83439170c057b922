"""The two criteria ``run_class_finetuning.py`` takes from ``timm.loss`` (:467-473): ``SoftTargetCrossEntropy`` for the soft
[B, classes] targets a ``mixup.Mixup`` produces, ``LabelSmoothingCrossEntropy`` for hard labels when mixup is off.  Same call
signatures; timm itself is not needed.

Both are one weighted sum over the log-softmax, ``mean_b sum_c -t[b,c] * log_softmax(z[b])[c]`` -- for label smoothing with
``t[c] = smoothing / classes + (c == label) * (1 - smoothing)`` -- and on the GPU, for f32 logits, both run through ONE HIP launch
(``tad_soft_target_ce``) that also leaves ``dloss/dz = (softmax(z) * sum_c t - t) / B`` behind, so the backward pass is a scaling by
the incoming gradient.  CPU tensors and other dtypes take the torch expressions below.

The criteria of the FRAME fine-tuning script follow (``run_frame_finetuning.py --loss``, :571-586; the classes of ``utils.py:638-734`` and
``:1091-1118``): ``FocalLoss``, ``FocalLoss2``, ``SmoothAPLoss``, ``TemporalExponentialLoss``, ``DoubleBCELoss``, with the reference's
constructor arguments, defaults and call signatures, and ``build_criterion(name)`` for the eight ``--loss`` names.  On the GPU, for
contiguous f32 logits, mean reduction and targets that carry no gradient, each is ONE HIP launch (``tad_frame_loss``) that leaves the loss
and ``dloss/dlogits`` behind; everything else -- CPU tensors, other dtypes, ``reduction='sum'/'none'``, ``gamma < 1`` -- takes the
reference's torch expression, restated below."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from . import kernels as K


class _SoftTargetCE(torch.autograd.Function):
    """loss (0-dim) of f32 GPU logits against soft rows (``target``) or smoothed hard labels (``labels``); the gradient reaches the
    logits only -- a target that requires grad takes the torch expression instead"""

    @staticmethod
    def forward(ctx, logits, target, labels, smoothing):
        loss, dlogits = K.soft_target_ce(logits.detach(), target, labels, smoothing)
        ctx.save_for_backward(dlogits)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        dlogits, = ctx.saved_tensors
        return dlogits * grad_out, None, None, None


def _on_hip(x):
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] > 0 and x.shape[1] >= 2


class SoftTargetCrossEntropy(torch.nn.Module):
    """timm.loss.SoftTargetCrossEntropy: ``sum(-target * log_softmax(x, -1), -1).mean()``"""

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if (_on_hip(x) and target.device == x.device and target.dtype == torch.float32 and target.shape == x.shape
                and not target.requires_grad):
            return _SoftTargetCE.apply(x.contiguous(), target.contiguous(), None, 0.0)
        return torch.sum(-target * F.log_softmax(x, dim=-1), dim=-1).mean()


class LabelSmoothingCrossEntropy(torch.nn.Module):
    """timm.loss.LabelSmoothingCrossEntropy: ``(1 - smoothing) * nll(x, target) + smoothing * mean_c(-log_softmax(x))``, batch mean"""

    def __init__(self, smoothing=0.1):
        super().__init__()
        assert smoothing < 1.0
        self.smoothing = smoothing
        self.confidence = 1. - smoothing

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if _on_hip(x) and target.device == x.device and target.dtype == torch.int64 and tuple(target.shape) == (x.shape[0],):
            return _SoftTargetCE.apply(x.contiguous(), None, target.contiguous(), float(self.smoothing))
        logprobs = F.log_softmax(x, dim=-1)
        nll = -logprobs.gather(dim=-1, index=target.unsqueeze(1)).squeeze(1)
        return (self.confidence * nll + self.smoothing * -logprobs.mean(dim=-1)).mean()


# ----------------------------------------------------------------------------------------- the frame fine-tuning losses
class _FrameLoss(torch.autograd.Function):
    """loss (0-dim) of f32 GPU logits under one kind of ``tad_frame_loss``; the gradient reaches the logits only"""

    @staticmethod
    def forward(ctx, logits, kind, operands, scalars):
        loss, dlogits = K.frame_loss(kind, logits.detach(), **operands, **scalars)
        ctx.save_for_backward(dlogits)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        dlogits, = ctx.saved_tensors
        return dlogits * grad_out, None, None, None


def _hard_on_hip(x, target, two_classes=False):
    return (_on_hip(x) and target.device == x.device and target.dtype == torch.int64 and tuple(target.shape) == (x.shape[0],)
            and (not two_classes or x.shape[1] == 2))


def _finite(*values, nonneg=False):
    """what tad_frame_loss accepts for a scalar; anything else takes the torch expression, like the reference"""
    try:
        return all(math.isfinite(float(v)) and (not nonneg or float(v) >= 0) for v in values)
    except (TypeError, ValueError):
        return False


def _reduce(per_row, reduction):
    if reduction == 'mean':
        return torch.mean(per_row)
    if reduction == 'sum':
        return torch.sum(per_row)
    return per_row


class FocalLoss(torch.nn.Module):
    """utils.FocalLoss (utils.py:638-656): ``multiplier * alpha * (1 - pt)**gamma * ce`` with ``ce`` the per-row cross entropy and
    ``pt = exp(-ce)``, reduced by ``reduction``.  The HIP route (mean reduction, ``gamma >= 1``) forms ``1 - pt`` as ``-expm1(-ce)``,
    which keeps its relative accuracy on confidently correct rows where ``1 - exp(-ce)`` is 0 or one ulp of 1."""

    def __init__(self, alpha=1, gamma=2, reduction='mean', multiplier=1.):
        super().__init__()
        self.alpha = alpha
        self.gamma = gamma
        self.reduction = reduction
        self.multiplier = multiplier

    def forward(self, inputs, targets):
        if (self.reduction == 'mean' and _finite(self.gamma, self.multiplier, nonneg=True) and self.gamma >= 1 and _finite(self.alpha)
                and _hard_on_hip(inputs, targets)):
            return _FrameLoss.apply(inputs.contiguous(), "focal", dict(labels=targets.contiguous()),
                                    dict(alpha=self.alpha, gamma=self.gamma, multiplier=self.multiplier))
        ce_loss = F.cross_entropy(inputs, targets, reduction='none')
        pt = torch.exp(-ce_loss)
        return _reduce(self.multiplier * self.alpha * ((1 - pt) ** self.gamma) * ce_loss, self.reduction)


class FocalLoss2(torch.nn.Module):
    """utils.FocalLoss2 (utils.py:659-682): the focal loss with a weight per class, ``alpha[target]`` (``alpha=None``: no weight).
    The reference builds ``torch.tensor(alpha, device=...)`` on every call, a host-to-device copy; here the device copy is made once
    per device (and per value of ``alpha``) and kept."""

    def __init__(self, alpha=[0.40, 0.60], gamma=2, reduction='mean', multiplier=1.):
        super().__init__()
        self.alpha = alpha
        self.gamma = gamma
        self.reduction = reduction
        self.multiplier = multiplier
        self._alpha_cache = {}

    def _alpha_on(self, device, dtype):
        key = (device, dtype, tuple(float(a) for a in self.alpha))
        t = self._alpha_cache.get(key)
        if t is None:
            self._alpha_cache.clear()
            t = self._alpha_cache[key] = torch.tensor(self.alpha, dtype=dtype, device=device)
        return t

    def forward(self, inputs, targets):
        if (self.reduction == 'mean' and _finite(self.gamma, self.multiplier, nonneg=True) and self.gamma >= 1 and _hard_on_hip(inputs, targets)
                and (self.alpha is None or (len(self.alpha) == inputs.shape[1] and _finite(*self.alpha)))):
            at = None if self.alpha is None else self._alpha_on(inputs.device, torch.float32)
            return _FrameLoss.apply(inputs.contiguous(), "focal2", dict(labels=targets.contiguous(), class_alpha=at),
                                    dict(gamma=self.gamma, multiplier=self.multiplier))
        ce_loss = F.cross_entropy(inputs, targets, reduction='none')
        pt = torch.exp(-ce_loss)
        if self.alpha is not None:
            ce_loss = self._alpha_on(inputs.device, inputs.dtype)[targets] * ce_loss
        return _reduce(((1 - pt) ** self.gamma) * ce_loss * self.multiplier, self.reduction)


class SmoothAPLoss(torch.nn.Module):
    """utils.SmoothAPLoss (utils.py:685-708): with ``p = softmax(predictions)[:, 1]``, the sum over (positive i, negative j) pairs of
    ``relu(p_j - p_i + delta)``, divided by the number of positives.  The reference sorts the negatives and loops over the positives in
    Python; the sort only fixes a summation order, and neither is done here.
    Difference from the reference: for a batch WITHOUT a positive row it returns the Python float ``0.0``, on which ``.backward()``
    fails; this returns a zero tensor attached to the graph, whose gradient is zero."""

    def __init__(self, delta=0.01):
        super().__init__()
        self.delta = delta

    def forward(self, predictions, labels):
        if _finite(self.delta, nonneg=True) and _hard_on_hip(predictions, labels, two_classes=True):
            return _FrameLoss.apply(predictions.contiguous(), "smoothap", dict(labels=labels.contiguous()), dict(delta=self.delta))
        pred_probs = F.softmax(predictions, dim=1)[:, 1]
        positive_probs = pred_probs[labels == 1]
        negative_probs = pred_probs[labels == 0]
        if positive_probs.shape[0] == 0:
            return predictions.sum() * 0.0
        return torch.relu(negative_probs.unsqueeze(0) - positive_probs.unsqueeze(1) + self.delta).sum() / positive_probs.shape[0]


class TemporalExponentialLoss(torch.nn.Module):
    """utils.TemporalExponentialLoss (utils.py:711-734): the per-row cross entropy weighted by
    ``min(1, exp(alpha_pre * t))`` before the anomaly (``t < 0``) and ``min(1, exp(-alpha_post * t))`` after it (``t > 0``), weight 1
    at ``t == 0`` (and for a NaN ``t``); batch mean.  ``t`` is the time to the anomaly in seconds, float64 from the datasets
    (``frame_targets.compute_time_vector``): the HIP route casts it to f32 on the device first.  ``max_time_pre`` / ``max_time_post``
    are stored and unused, as in the reference."""

    def __init__(self, alpha_pre=0.1, alpha_post=0.5, max_time_pre=1.0, max_time_post=0.5):
        super().__init__()
        self.alpha_pre = alpha_pre
        self.alpha_post = alpha_post
        self.max_time_pre = max_time_pre
        self.max_time_post = max_time_post

    def forward(self, y_pred, y_true, time_to_anomaly):
        t = time_to_anomaly
        if (_finite(self.alpha_pre, self.alpha_post) and _hard_on_hip(y_pred, y_true) and t.device == y_pred.device and t.is_floating_point() and tuple(t.shape) == tuple(y_true.shape)
                and not t.requires_grad):
            return _FrameLoss.apply(y_pred.contiguous(), "exponential", dict(labels=y_true.contiguous(), ttc=t.to(torch.float32).contiguous()),
                                    dict(alpha_pre=self.alpha_pre, alpha_post=self.alpha_post))
        base_loss = F.cross_entropy(y_pred, y_true, reduction='none')
        weight = torch.ones_like(y_true, dtype=torch.float)      # (f32 whatever the logits are, as in the reference)
        weight = torch.where(t < 0, torch.exp(self.alpha_pre * t).to(weight.dtype), weight)
        weight = torch.where(t > 0, torch.exp(-self.alpha_post * t).to(weight.dtype), weight)
        weight = torch.clamp(weight, max=1.0)
        return (base_loss * weight).mean()


class DoubleBCELoss(torch.nn.Module):
    """utils.DoubleBCELoss (utils.py:1091-1118): ``BCEWithLogits`` of each of the two logits against its temporally smoothed label
    (``frame_targets.smooth_labels``), the two added per row, batch mean.  The constructor arguments are accepted and unused, as in the
    reference."""

    def __init__(self, alpha=1, gamma=2, reduction='mean', multiplier=1.):
        super().__init__()

    def forward(self, logits, smoothed_labels):
        s = smoothed_labels
        if (_on_hip(logits) and logits.shape[1] == 2 and s.device == logits.device and s.dtype == torch.float32 and s.shape == logits.shape
                and not s.requires_grad):
            return _FrameLoss.apply(logits.contiguous(), "2bce", dict(soft=s.contiguous()), {})
        loss_safe = F.binary_cross_entropy_with_logits(logits[:, 0], s[:, 0], reduction='none')
        loss_anomaly = F.binary_cross_entropy_with_logits(logits[:, 1], s[:, 1], reduction='none')
        return (loss_safe + loss_anomaly).mean()


LOSS_NAMES = ("crossentropy", "focal", "focal6x100", "focal2_6", "focal2_2", "2bce", "smoothap", "exponential1")


def build_criterion(name: str):
    """the criterion of a ``--loss`` name of run_frame_finetuning.py (:571-586), with its constants.  ``exponential1`` is the one that is
    called as ``criterion(outputs, targets, ttc)``: run it with ``engine.train_one_epoch(..., with_ttc=True)``, as the reference does.
    Difference from the reference: its ``exponential1`` passes ``lambda_param=0.1``, an argument ``TemporalExponentialLoss.__init__``
    does not have, so that option raises a TypeError there; here it is the default ``TemporalExponentialLoss()``."""
    if name == "crossentropy":
        return torch.nn.CrossEntropyLoss()
    if name == "focal":
        return FocalLoss(alpha=0.75, gamma=2)
    if name == "focal6x100":
        return FocalLoss(alpha=0.75, gamma=6, multiplier=100)
    if name == "focal2_6":
        return FocalLoss2(gamma=6, multiplier=50)
    if name == "focal2_2":
        return FocalLoss2(gamma=2, multiplier=10)
    if name == "2bce":
        return DoubleBCELoss()
    if name == "smoothap":
        return SmoothAPLoss()
    if name == "exponential1":
        return TemporalExponentialLoss()
    raise NotImplementedError(f"Loss not implemented: {name}")
