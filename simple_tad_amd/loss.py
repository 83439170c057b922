"""The two criteria ``run_class_finetuning.py`` takes from ``timm.loss`` (:467-473): ``SoftTargetCrossEntropy`` for the soft
[B, classes] targets a ``mixup.Mixup`` produces, ``LabelSmoothingCrossEntropy`` for hard labels when mixup is off.  Same call
signatures; timm itself is not needed.

Both are one weighted sum over the log-softmax, ``mean_b sum_c -t[b,c] * log_softmax(z[b])[c]`` -- for label smoothing with
``t[c] = smoothing / classes + (c == label) * (1 - smoothing)`` -- and on the GPU, for f32 logits, both run through ONE HIP launch
(``tad_soft_target_ce``) that also leaves ``dloss/dz = (softmax(z) * sum_c t - t) / B`` behind, so the backward pass is a scaling by
the incoming gradient.  CPU tensors and other dtypes take the torch expressions below."""
from __future__ import annotations

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
