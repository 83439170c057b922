"""Where a scored window looks: attention rollout (Abnar & Zuidema, 2020) and the attention each token receives, as saliency maps over the
token grid -- without ever forming an N x N attention matrix.

The head of the classifier reads one linear functional of the last block's tokens: their mean (``final_reduction="fc_norm"``) or token 0
(``"cls"``).  Rollout with the residual weight alpha multiplies the per-layer matrices A~_l = alpha I + (1 - alpha) mean_h P_{l,h}; only the
row vector u^T A~_L ... A~_1 is wanted, so it is propagated from the last layer to the first as a vector,

    v_{l-1} = alpha v_l + (1 - alpha) mean_h( sum_i v_l[i] P_{l,h}[i, :] ),

and each step is a weighted column sum of the softmax, recomputed from the layer's ``qkv`` and ``lse`` by ONE launch of
``kernels.attn_colsum`` (csrc/attn_colsum.hip).  The records come from ``ops.capture_attention()``; the head mean and the
blend are plain torch on [B, H, N].
"""
from __future__ import annotations

import torch

from . import kernels as K
from . import ops
from ._lib import TadError

__all__ = ["token_rollout", "attention_received", "attention_rollout", "saliency_to_frames", "token_grid"]


def _kernel_colsum(rec, v):
    qkv, lse, B, N, H, d, scale, q_prescaled = rec
    if tuple(v.shape) != (B, N):
        raise TadError(f"explain: the weight vector is {tuple(v.shape)}, the captured layer has [B, N] = {(B, N)}")
    return K.attn_colsum(qkv, lse, v.to(torch.float32).contiguous(), B, N, H, scale, q_prescaled=q_prescaled, d=d)


def token_rollout(records, start, residual: float = 0.5, *, colsum=None):
    """records: the list ``ops.capture_attention()`` filled, first layer first.  start [B,N]: the functional the head reads (uniform 1/N for
    the token mean, one-hot for a single token).  Returns [B,N], normalised to sum 1 per clip.  Exactly this arithmetic, from the LAST record
    to the first: ``v = residual * v + (1 - residual) * c.mean(1)`` with ``c = attn_colsum(layer, v)`` [B,H,N]; then ``v / v.sum(-1)``.
    colsum(record, v) -> [B,H,N] replaces the kernel (tests run the recurrence on explicit matrices in fp64)."""
    if not len(records):
        raise TadError("token_rollout: no attention records (run the model inside ops.capture_attention())")
    if not 0.0 <= float(residual) < 1.0:
        raise ValueError(f"residual must lie in [0, 1), got {residual}")
    f = colsum or _kernel_colsum
    v = start
    for rec in reversed(records):
        c = f(rec, v)
        v = residual * v + (1 - residual) * c.mean(1)
    return v / v.sum(-1, keepdim=True)


def attention_received(records, layer: int = -1):
    """[B,H,N]: the attention token j receives in ``layer``, averaged over the queries -- attn_colsum with w = 1/N.  Sums to 1 per head."""
    rec = records[layer]
    B, N = rec[2], rec[3]
    return _kernel_colsum(rec, torch.full((B, N), 1.0 / N, dtype=torch.float32, device=rec[0].device))


def token_grid(model):
    """(T / tubelet, H / patch, W / patch): the token order of PatchEmbed is time-major"""
    pe = model.patch_embed
    return (int(model.num_frames) // int(pe.tubelet_size), int(pe.img_size[0]) // int(pe.patch_size[0]), int(pe.img_size[1]) // int(pe.patch_size[1]))


def _captured_forward(model, x):
    """(logits, records) of the evaluation forward of ``x`` under no_grad; the model's mode is put back"""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            with ops.capture_attention(model) as records:
                logits = model(x)
    finally:
        model.train(was_training)
    if not records:
        raise TadError("explain: the forward ran no attention the capture could see")
    return logits, records


def _to_grid(model, tokens):
    B, N = tokens.shape
    grid = token_grid(model)
    if grid[0] * grid[1] * grid[2] != N:
        raise TadError(f"explain: {N} tokens do not fill the model's grid {grid} (masked token sets have no grid mapping)")
    return tokens.reshape(B, *grid)


def start_vector(model, B: int, N: int, device):
    fr = getattr(model, "final_reduction", None)
    if fr == "fc_norm":
        return torch.full((B, N), 1.0 / N, dtype=torch.float32, device=device)
    if fr == "cls":
        s = torch.zeros((B, N), dtype=torch.float32, device=device)
        s[:, 0] = 1.0
        return s
    raise TadError(f'attention_rollout: final_reduction={fr!r} reads every token; pass start=[B,N], the functional to explain')


def attention_rollout(model, x, residual: float = 0.5, start=None):
    """(logits, saliency [B, T/tubelet, H/patch, W/patch]).  x: anything ``VisionTransformer.forward`` takes (f32 clips, uint8 frames,
    ``FrameWindows``).  Runs the model in eval mode under no_grad (its mode is put back); the logits are those of the plain evaluation
    forward, bit for bit.  start (optional [B,N]) replaces the head's own functional: uniform for "fc_norm", one-hot on token 0 for "cls"."""
    logits, records = _captured_forward(model, x)
    B, N = records[-1][2], records[-1][3]
    if start is None:
        start = start_vector(model, B, N, records[-1][0].device)
    return logits, _to_grid(model, token_rollout(records, start, residual))


def attention_received_map(model, x, layer: int = -1):
    """(logits, [B, T/tubelet, H/patch, W/patch]): ``attention_received`` of one layer, averaged over the heads, on the token grid"""
    logits, records = _captured_forward(model, x)
    return logits, _to_grid(model, attention_received(records, layer).mean(1))


def saliency_to_frames(sal, size, mode: str = "nearest"):
    """sal [B, T', gh, gw] -> [B, T, H, W] with size = (T, H, W): every token's value on the frames of its tubelet (T / T' each) and, in
    space, on its patch ("nearest") or interpolated between patch centres ("bilinear").  A heat map for display: values are copied, not
    divided among the pixels."""
    if sal.dim() != 4:
        raise ValueError(f"saliency must be [B, T', gh, gw], got {tuple(sal.shape)}")
    T, H, W = (int(s) for s in size)
    Tp = sal.shape[1]
    if mode not in ("nearest", "bilinear"):
        raise ValueError(f"mode must be nearest or bilinear, got {mode!r}")
    if T % Tp:
        raise ValueError(f"{T} frames are no whole number of tubelets for {Tp} token rows")
    kw = {} if mode == "nearest" else {"align_corners": False}
    up = torch.nn.functional.interpolate(sal.float(), size=(H, W), mode=mode, **kw)
    return up.repeat_interleave(T // Tp, dim=1)
