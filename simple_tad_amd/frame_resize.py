"""The first stage of every input path on the device: the loader's ``cv2.resize(frame, (S, S), INTER_CUBIC)`` and the fine-tune datasets'
``video_transforms.pad_wide_clips``.

The reference resizes every decoded frame on the host before anything else sees it: ``run_inference.py:76,91`` per camera frame,
``load_images(final_resize=True)`` (dota.py:347-348, dada.py:309-310) per test frame, and ``_aug_frame`` (dota.py:293-297) per training
clip behind ``pad_wide_clips(h, w, crop_size)`` (video_transforms.py:1301-1337), which pads a wide frame at top and bottom -- black, a
random colour, a reflection faded towards black, or replicated edges -- before the resize.  Here decoded uint8 frames of any size go to
the device once and ONE HIP launch (``tad_frame_resize``, csrc/frame_resize.hip) turns them into the model-size uint8 frames, or the
normalised f32 clips, that the rest of the package takes.  The pad bands are never materialised: they are a row map the kernel's
horizontal pass applies.

THE CONTRACT is OpenCV's generic integer formulation of the 8-bit cubic resize (include/tad_mi355x.h states it; tests/
frame_resize_recipe.py restates it in numpy), NOT the bytes of a particular OpenCV build: a build's vector path finishes the vertical
pass in float, its scalar path in integers, the two can differ by one grey level, and which bytes take which path depends on the build
and the row width.  The kernel equals the recipe bit for bit; the recipe lies within one grey level of an independent float64 bicubic.
All float work is done here, in numpy float32 / float64 (``cubic_coeffs``); the device sees integers only.

RNG contract of ``PadWideClips.plan``: torch's GLOBAL CPU generator, one reference call per clip in index order --
``torch.randint(0, 12, (1,))`` picks the mode from (None x5, black, black, color, reflect, reflect, replicate, replicate); only with a
mode and ``w - h > 0`` follow, always all three, ``torch.rand(1)`` for pad_top = int(round(u * 0.5 * (w - h))), ``torch.rand(1)`` for
pad_bottom, ``torch.rand(1) * 0.7`` for alpha; for ``color`` alone then ``torch.randint(0, 256, (3,))``.

There is no CPU path: a CPU tensor raises ``TadError``.  Not built: the other loader resizes (INTER_AREA, INTER_LINEAR), pads above the
frame's height (a second reflection), clips of different source sizes in one call.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import TadError

_BITS = 11                      # OpenCV's INTER_RESIZE_COEF_BITS: the coefficients are 11-bit fixed point
_MODES = (None, None, None, None, None, "black", "black", "color", "reflect", "reflect", "replicate", "replicate")
_MODE_CODE = {None: _lib.FR_NONE, "black": _lib.FR_CONST, "color": _lib.FR_CONST, "reflect": _lib.FR_REFLECT, "replicate": _lib.FR_REPLICATE}

# the pad of one clip: ``mode`` None | black | color | reflect | replicate; ``colour`` one byte per stored channel
Pad = namedtuple("Pad", "mode pad_top pad_bottom alpha colour")
NO_PAD = Pad(None, 0, 0, 0.0, (0, 0, 0))


@functools.lru_cache(maxsize=256)
def cubic_coeffs(n_src: int, n_dst: int):
    """(first int32 [n_dst], k int32 [n_dst, 4]) of the cubic resize from ``n_src`` to ``n_dst`` samples: output d reads the source
    indices first[d] .. first[d] + 3, each clamped to [0, n_src - 1], with the 11-bit weights k[d] (Keys, A = -0.75; not
    renormalised: they sum to 2047, 2048 or 2049)."""
    if n_src < 1 or n_dst < 1:
        raise TadError(f"cubic_coeffs: {n_src} -> {n_dst} samples")
    scale = n_src / n_dst
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    x = f - s                                                   # float32
    one, A = np.float32(1), np.float32(-0.75)
    x1, xr = x + one, one - x
    c = np.empty((n_dst, 4), dtype=np.float32)
    c[:, 0] = ((A * x1 - np.float32(5) * A) * x1 + np.float32(8) * A) * x1 - np.float32(4) * A
    c[:, 1] = ((A + np.float32(2)) * x - (A + np.float32(3))) * x * x + one
    c[:, 2] = ((A + np.float32(2)) * xr - (A + np.float32(3))) * xr * xr + one
    c[:, 3] = one - c[:, 0] - c[:, 1] - c[:, 2]
    k = np.clip(np.rint(c * np.float32(1 << _BITS)), -32768, 32767).astype(np.int32)
    first = s.astype(np.int32) - 1
    first.setflags(write=False)
    k.setflags(write=False)
    return first, k


def _size(size):
    S_h, S_w = (size, size) if isinstance(size, int) else tuple(size)
    if int(S_h) < 1 or int(S_w) < 1:
        raise TadError(f"frame_resize: size {size!r} must be S or (S_h, S_w)")
    return int(S_h), int(S_w)


def pad_table(pads, B: int, H: int, W: int, S_h: int, S_w: int):
    """the kernel's table (kernels.frame_resize_table) for B clips of H x W frames, clip b padded as ``pads[b]``: (int32 CPU tensor,
    n_vsets).  Host only."""
    if len(pads) != B:
        raise TadError(f"frame_resize: {len(pads)} pads for {B} clips")
    vsets, rows = {}, []
    for b, p in enumerate(pads):
        if p.mode not in _MODE_CODE:
            raise TadError(f"frame_resize: clip {b}: unknown pad mode {p.mode!r}")
        top, bottom = (0, 0) if p.mode is None else (int(p.pad_top), int(p.pad_bottom))
        if top > H or bottom > H:
            raise TadError(f"frame_resize: clip {b}: pad ({top}, {bottom}) above the frame's height {H} needs a second reflection (not built)")
        rows.append((b, _MODE_CODE[p.mode], top, bottom, float(p.alpha), p.colour if p.mode == "color" else (0, 0, 0),
                     vsets.setdefault(top + H + bottom, len(vsets))))
    table = K.frame_resize_table(rows, (W, *cubic_coeffs(W, S_w)), [(hv, *cubic_coeffs(hv, S_h)) for hv in vsets], B, H, W, S_h, S_w)
    return table, len(vsets)


@functools.lru_cache(maxsize=64)
def _plain_table(B, H, W, S_h, S_w, pinned):
    table, _ = pad_table([NO_PAD] * B, B, H, W, S_h, S_w)
    return table.pin_memory() if pinned else table


def _frames(x, who):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.uint8 and x.dim() in (4, 5) and x.shape[-1] == 3
            and x.is_contiguous() and x.numel() > 0):
        raise TadError(f"{who}: expected contiguous uint8 frames [N,H,W,3] or [B,T,H,W,3] on the GPU (there is no CPU path)")
    return x.unsqueeze(0) if x.dim() == 4 else x


def resize_frames(x, size, mean=None, std=None, out=None):
    """cv2.resize(frame, (S_w, S_h), INTER_CUBIC) of every frame of the uint8 frames x ([N,H,W,3] or [B,T,H,W,3]) on the device, ONE launch;
    ``size`` = S or (S_h, S_w).  Returns uint8 frames of x's layout at the new size, or with ``mean`` / ``std`` the normalised f32
    clips ([3,N,S_h,S_w] / [B,3,T,S_h,S_w]).  ``out``: a contiguous view of that shape to write into (a ring slot, a slice of a frame
    store).  The table reaches the device through pinned memory: the call never waits for the GPU."""
    x5 = _frames(x, "resize_frames")
    S_h, S_w = _size(size)
    B, T, H, W, _ = x5.shape
    flat = x.dim() == 4
    if out is not None and flat:
        if not isinstance(out, torch.Tensor) or out.dim() != 4:
            raise TadError(f"resize_frames.out: expected a tensor of {x.shape[0]} frames, got {type(out).__name__}")
        out = out.unsqueeze(0)
    with torch.cuda.device(x.device):
        dev = _plain_table(B, H, W, S_h, S_w, True).to(x.device, non_blocking=True)
        y = K.frame_resize(x5, dev, 1, S_h, S_w, mean, std, out)
    return y[0] if flat else y


class PadWideClips:
    """video_transforms.pad_wide_clips (:1301-1337) for a batch: ``plan(B, h, w)`` draws what B calls of the reference draw, and the
    call carries a plan out on uint8 clips [B,T,h,w,3] on the GPU, giving the uint8 clips [B,T,S,S,3] ``rand_augment.RandAugment``
    takes (``_aug_frame``, dota.py:293-297: pad, resize, then RandAugment)."""

    def __init__(self, crop_size: int):
        if int(crop_size) < 1:
            raise TadError(f"PadWideClips: crop_size {crop_size!r} must be positive")
        self.crop_size = int(crop_size)

    def plan(self, B: int, h: int, w: int):
        """Consume the random draws of B clips of h x w frames (the module docstring gives their order) and return one ``Pad`` per
        clip.  Host only."""
        pads = []
        for _ in range(int(B)):
            mode = _MODES[torch.randint(0, len(_MODES), (1,)).item()]
            slack = w - h
            if mode is None or slack <= 0:
                pads.append(NO_PAD)
                continue
            top = int(round(torch.rand(1).item() * 0.5 * slack))
            bottom = int(round(torch.rand(1).item() * 0.5 * slack))
            alpha = torch.rand(1).item() * 0.7
            colour = tuple(torch.randint(0, 256, (3,)).tolist()) if mode == "color" else (0, 0, 0)
            pads.append(Pad(mode, top, bottom, alpha, colour))
        return pads

    def __call__(self, x, plan=None, mean=None, std=None, out=None):
        x5 = _frames(x, "PadWideClips")
        if x.dim() != 5:
            raise TadError("PadWideClips: expected uint8 clips [B,T,H,W,3] on the GPU")
        B, _, H, W, _ = x5.shape
        pads = self.plan(B, H, W) if plan is None else [Pad(*p) for p in plan]
        table, nv = pad_table(pads, B, H, W, self.crop_size, self.crop_size)
        with torch.cuda.device(x.device):
            # pinned staging + asynchronous copy: the host never waits for the device
            dev = table.pin_memory().to(x.device, non_blocking=True)
            return K.frame_resize(x5, dev, nv, self.crop_size, self.crop_size, mean, std, out)
