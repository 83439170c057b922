"""The spatial sampling of the class fine-tuning recipe: counterpart of the reference's ``spatial_sampling`` (kinetics.py:369-440,
ssv2.py) and of the ``video_transforms`` functions it chains (video_transforms.py:60-267, 515-634): the Inception-style random
resized crop (``scale`` / ``aspect_ratio``), its ``motion_shift`` variant with one box per frame, or the short-side scale jitter
followed by a random crop; then the horizontal flip; and, with ``spatial_idx`` 0 / 1 / 2, the three deterministic test-time crops.

Same keywords and defaults -- ``SpatialSampling(spatial_idx, min_scale, max_scale, crop_size, random_horizontal_flip,
inverse_uniform_sampling, aspect_ratio, scale, motion_shift)`` -- but, like ``rand_augment.RandAugment`` and
``transforms.GroupMultiScaleCrop``, the work is split.  One host routine (``plan``) turns the random draws into one ``Window`` per
(clip, frame): a window of the source, the grid it is resized to, the ``crop_size`` square taken from that grid, a flip.  ONE HIP
launch (``tad_spatial_sample``, csrc/spatial_sample.hip) then carries the windows out on a contiguous batch on the GPU -- the
normalised f32 clips [B,3,T,H,W], or the uint8 frames [B,T,H,W,3] ``RandAugment`` returns, normalised on the fly -- into the f32 clips
[B,3,T,S,S].  The table reaches the device through pinned memory, so a call never waits for the GPU.  Every resize is the
reference's ``torch.nn.functional.interpolate(mode="bilinear", align_corners=False)``: four taps per output, no antialiasing; the
f32 arithmetic is stated in include/tad_mi355x.h and restated in tests/spatial_sampling_recipe.py.  There is no CPU path: a CPU
tensor raises ``TadError``.

RNG contract.  Clips run in index order; each consumes Python's GLOBAL ``random`` and numpy's GLOBAL stream exactly as one call of
the reference's ``spatial_sampling`` does:

* random resized crop: up to 10 attempts, each ``random.uniform(*scale)``, ``random.uniform(log ratio[0], log ratio[1])`` and one
  ``np.random.uniform()`` (the reference's axis-swap coin, drawn on every attempt and never acted on); an attempt that fits the
  source then draws ``random.randint(0, H - h)`` and ``random.randint(0, W - w)``.  After 10 misses: the central crop at the nearest
  allowed ratio, no further draw.  ``motion_shift=True`` draws two such boxes and gives frame t the truncated ``torch.linspace``
  between them.
* jitter + random crop (neither ``scale`` nor ``aspect_ratio``): ``np.random.uniform(min_scale, max_scale)`` -- or, with
  ``inverse_uniform_sampling``, ``np.random.uniform(1 / max_scale, 1 / min_scale)`` -- then ``np.random.randint(0, extent - crop_size)``
  (upper bound exclusive) for the rows and then for the columns, each only where ``extent > crop_size``.
* ``random_horizontal_flip``: one ``np.random.uniform()`` after either route; below 0.5 flips the whole clip.
* ``spatial_idx`` 0 / 1 / 2: the jitter's one ``np.random.uniform(min_scale, max_scale)`` and nothing else.

Batch-level ordering.  The reference augments clip by clip in its dataset workers: RandAugment draws for clip 0, then the crop of
clip 0, then its erasing, then clip 1.  This package draws each augmenter for the whole batch: all of ``RandAugment``'s draws, then
all crops here, then ``RandomErasing``'s, then ``Mixup``'s.  RandAugment and the crop share Python's ``random`` and numpy's stream, so a
seeded batch of more than one clip sees other draws than the reference's interleaved loop; each augmenter alone, and a batch of one,
consume the streams as the reference does.

Not mirrored, refused with ``TadError``: where the reference itself raises (a ``spatial_idx`` outside -1..2; ``min_scale``,
``max_scale`` and ``crop_size`` not all equal with ``spatial_idx`` >= 0; only one of ``scale`` / ``aspect_ratio``); a jittered clip
that is exactly ``crop_size`` square, where the reference's ``random_crop`` returns a bare tensor and its caller's two-name
assignment raises ``ValueError``; and a jittered clip smaller than ``crop_size`` along an axis, where the reference would return a
clip that is not ``crop_size`` square.  The ``boxes=`` arguments of the reference's functions are not built.
"""
from __future__ import annotations

import math
import random
from collections import namedtuple

import numpy as np
import torch

from . import kernels as K
from ._lib import TadError

# what happens to frame `frame` of clip `clip`: x[.., i:i+h, j:j+w] is resized to (rh, rw); the output is [oy:oy+S, ox:ox+S] of that,
# flipped horizontally when `flip`
Window = namedtuple("Window", "clip frame i j h w rh rw oy ox flip")
_ATTEMPTS = 10


def _box(scale, ratio, H, W):
    """(i, j, h, w) of one Inception-style box in an H x W source (video_transforms.py:515-554); the module docstring gives the draws"""
    area = H * W
    log_lo, log_hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(_ATTEMPTS):
        target = random.uniform(*scale) * area
        aspect = math.exp(random.uniform(log_lo, log_hi))
        w = int(round(math.sqrt(target * aspect)))
        h = int(round(math.sqrt(target / aspect)))
        np.random.uniform()                                  # the axis-swap coin: spent, never acted on
        if 0 < w <= W and 0 < h <= H:
            i = random.randint(0, H - h)
            j = random.randint(0, W - w)
            return i, j, h, w
    in_ratio = float(W) / float(H)
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w


def _jittered(size, H, W):
    """(rh, rw): the short side becomes ``size``, the long side floor(long / short * size) (video_transforms.py:89-104)"""
    if (W <= H and W == size) or (H <= W and H == size):
        return H, W
    if W < H:
        return int(math.floor((float(H) / W) * size)), size
    return size, int(math.floor((float(W) / H) * size))


class SpatialSampling:
    """kinetics.py:369-440.  The keywords are the reference's."""

    def __init__(self, spatial_idx=-1, min_scale=256, max_scale=320, crop_size=224, random_horizontal_flip=True,
                 inverse_uniform_sampling=False, aspect_ratio=None, scale=None, motion_shift=False):
        if spatial_idx not in (-1, 0, 1, 2):
            raise TadError(f"SpatialSampling: spatial_idx {spatial_idx!r} must be -1, 0, 1 or 2")
        if spatial_idx != -1 and len({min_scale, max_scale, crop_size}) != 1:
            raise TadError(f"SpatialSampling: with spatial_idx {spatial_idx} nothing is jittered: min_scale {min_scale}, max_scale "
                           f"{max_scale} and crop_size {crop_size} must be the same")
        if spatial_idx == -1 and (aspect_ratio is None) != (scale is None):
            raise TadError("SpatialSampling: scale and aspect_ratio come together")
        if int(crop_size) != crop_size or crop_size < 1:
            raise TadError(f"SpatialSampling: crop_size {crop_size!r} must be a positive integer")
        self.spatial_idx, self.min_scale, self.max_scale, self.crop_size = spatial_idx, min_scale, max_scale, int(crop_size)
        self.random_horizontal_flip, self.inverse_uniform_sampling = random_horizontal_flip, inverse_uniform_sampling
        self.aspect_ratio, self.scale, self.motion_shift = aspect_ratio, scale, motion_shift

    # ------------------------------------------------------------------ the random draws
    def _jitter(self, H, W, inverse):
        if inverse:
            size = int(round(1.0 / np.random.uniform(1.0 / self.max_scale, 1.0 / self.min_scale)))
        else:
            size = int(round(np.random.uniform(self.min_scale, self.max_scale)))
        if size < 1:
            raise TadError(f"SpatialSampling: the jitter drew a short side of {size}")
        rh, rw = _jittered(size, H, W)
        S = self.crop_size
        if rh < S or rw < S:
            raise TadError(f"SpatialSampling: the jittered clip {rh} x {rw} is smaller than crop_size {S} (the reference would return a "
                           f"clip that is not {S} x {S})")
        return rh, rw

    def draw(self, T, H, W):
        """the T windows (i, j, h, w, rh, rw, oy, ox, flip) of one clip of T frames H x W, consuming both streams as one call of the
        reference's ``spatial_sampling`` does"""
        S = self.crop_size
        if self.spatial_idx != -1:
            rh, rw = self._jitter(H, W, False)
            oy, ox = int(math.ceil((rh - S) / 2)), int(math.ceil((rw - S) / 2))
            if rh > rw:
                oy = {0: 0, 1: oy, 2: rh - S}[self.spatial_idx]
            else:
                ox = {0: 0, 1: ox, 2: rw - S}[self.spatial_idx]
            return [(0, 0, H, W, rh, rw, oy, ox, 0)] * T
        if self.scale is None:
            rh, rw = self._jitter(H, W, self.inverse_uniform_sampling)
            if rh == S and rw == S:
                raise TadError(f"SpatialSampling: the jittered clip is exactly {S} x {S}: the reference's random_crop returns a bare "
                               f"tensor there and spatial_sampling raises ValueError")
            oy = int(np.random.randint(0, rh - S)) if rh > S else 0
            ox = int(np.random.randint(0, rw - S)) if rw > S else 0
            boxes = [(0, 0, H, W, rh, rw, oy, ox)] * T
        elif self.motion_shift:
            first, last = _box(self.scale, self.aspect_ratio, H, W), _box(self.scale, self.aspect_ratio, H, W)
            per_axis = [[int(v) for v in torch.linspace(a, b, steps=T).tolist()] for a, b in zip(first, last)]
            boxes = [(i, j, h, w, S, S, 0, 0) for i, j, h, w in zip(*per_axis)]
        else:
            boxes = [_box(self.scale, self.aspect_ratio, H, W) + (S, S, 0, 0)] * T
        flip = int(np.random.uniform() < 0.5) if self.random_horizontal_flip else 0
        return [b + (flip,) for b in boxes]

    def plan(self, B, T, H, W):
        """Consume the random draws for B clips of T frames H x W (the module docstring gives their order) and return the ``Window``
        list, clip by clip and frame by frame.  Host only."""
        return [Window(b, t, *win) for b in range(B) for t, win in enumerate(self.draw(T, H, W))]

    # ------------------------------------------------------------------ carrying a plan out
    def table(self, plan, B, T, H, W):
        """the plan as the kernel's table (kernels.spatial_sample_table): int32 CPU tensor [B * T, 12]"""
        rows = [None] * (B * T)
        for win in plan:
            if not (0 <= win.clip < B and 0 <= win.frame < T) or rows[win.clip * T + win.frame] is not None:
                raise TadError(f"SpatialSampling: {win} is not one window per frame of {B} clips of {T} frames")
            rows[win.clip * T + win.frame] = (win.clip * T + win.frame,) + tuple(int(v) for v in win[2:])
        if any(r is None for r in rows):
            raise TadError(f"SpatialSampling: the plan does not hold one window per frame of {B} clips of {T} frames")
        return K.spatial_sample_table(rows, B, T, H, W, self.crop_size)

    def apply(self, x, plan, out=None, normalize=None):
        """carry out the plan (``plan(B, T, H, W)``, or windows stated by hand) on the f32 clips [B,3,T,H,W], or with
        ``normalize=(mean, std)`` on the uint8 frames [B,T,H,W,3] (each tap becomes (v / 255 - mean) / std first: the bits of the f32
        route on ``frames_to_clip(x)``); contiguous, on the device.  Returns the f32 clips [B,3,T,S,S] (``out=`` is honoured); x is
        only read."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 5 and x.is_contiguous() and x.numel() > 0):
            raise TadError("SpatialSampling: expected contiguous f32 clips [B,3,T,H,W] or uint8 frames [B,T,H,W,3] on the GPU (there is "
                           "no CPU path)")
        if x.dtype == torch.uint8:
            if normalize is None:
                raise TadError("SpatialSampling: uint8 frames need normalize=(mean, std)")
            if x.shape[-1] != 3:
                raise TadError(f"SpatialSampling: expected uint8 frames [B,T,H,W,3], got {tuple(x.shape)}")
            B, T, H, W, _ = x.shape
        elif x.dtype == torch.float32:
            if normalize is not None:
                raise TadError("SpatialSampling: f32 clips are normalised already; normalize= goes with uint8 frames")
            if x.shape[1] != 3:
                raise TadError(f"SpatialSampling: expected f32 clips [B,3,T,H,W], got {tuple(x.shape)}")
            B, _, T, H, W = x.shape
        else:
            raise TadError(f"SpatialSampling: expected f32 clips or uint8 frames, got {x.dtype}")
        mean, std = normalize if normalize is not None else (None, None)
        if normalize is not None and (len(mean) != 3 or len(std) != 3):
            raise TadError("SpatialSampling: mean and std hold one value per RGB channel")
        table = self.table(plan, B, T, H, W)
        with torch.cuda.device(x.device):
            # pinned staging + asynchronous copy: the host never waits for the device
            dev = table.pin_memory().to(x.device, non_blocking=True)
            return K.spatial_sample(x, dev, self.crop_size, mean, std, out)

    def __call__(self, x, normalize=None, out=None):
        if not isinstance(x, torch.Tensor) or x.dim() != 5:
            raise TadError("SpatialSampling: expected f32 clips [B,3,T,H,W] or uint8 frames [B,T,H,W,3] on the GPU")
        if x.dtype == torch.uint8:
            B, T, H, W, _ = x.shape
        else:
            B, _, T, H, W = x.shape
        return self.apply(x, self.plan(B, T, H, W), out=out, normalize=normalize)
