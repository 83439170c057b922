"""The augmentation of the MAE pre-training path: counterpart of the reference's ``transforms.GroupMultiScaleCrop`` (transforms.py:91-160)
and of ``DataAugmentationForVideoMAE`` / ``DataAugmentationForVideoMAE_LightCrop`` (datasets.py), which chain the crop with ``Stack``,
``ToTorchFormatTensor`` and ``GroupNormalize`` and hand every clip a tube mask.

Same surface -- ``GroupMultiScaleCrop(input_size, scales, max_distort, fix_crop, more_fix_crop)`` -- but, like ``rand_augment.RandAugment``,
the work is split.  One host routine (``plan``) turns the random draws into one crop per clip.  A contiguous uint8 batch [B,T,Hs,Ws,3]
on the GPU (all clips of one source size) is then cropped and resized by ONE HIP launch (``tad_multiscale_crop``), to uint8 frames
[B,T,S_h,S_w,3] or straight to the normalised f32 clips [B,3,T,S_h,S_w]; the table reaches the device through pinned memory, so a
call never waits for the GPU.  The result is PIL's ``Image.resize(size, BILINEAR)`` of the cropped frames byte for byte: the host
states Pillow's per-axis coefficients in Python floats (doubles) and rounds them to 22-bit integers, the device runs both integer
passes (csrc/multiscale_crop.hip, tests/multiscale_crop_recipe.py).  There is no CPU path: a CPU tensor raises ``TadError``.

RNG contract.  Clips run in index order, each as one call of the reference's transform would, from Python's GLOBAL ``random``
stream: ``random.choice(pairs)`` over the (w, h) crop sizes, then ``random.choice(offsets)`` over the 5 (``more_fix_crop=False``) or
13 fixed offsets -- or, with ``fix_crop=False``, ``random.randint(0, Ws - w)`` and ``random.randint(0, Hs - h)``.  The tube masks of
``DataAugmentationForVideoMAE`` come from numpy's GLOBAL stream, one ``TubeMaskingGenerator`` call per clip (another stream than the
crops', so drawing the batch's crops first and its masks second consumes both as the reference's per-sample calls do).

Not built: a crop that shrinks an axis by more than 8 (Pillow's kernel grows past 17 taps; ``TadError``).  (The fine-tune recipe's
``spatial_sampling`` -- random resized crop, scale jitter + crop, flip, the three test-time crops -- is
``spatial_sampling.SpatialSampling``; the cv2 ``INTER_CUBIC`` loader resize and ``pad_wide_clips`` of the fine-tune datasets are
``frame_resize.resize_frames`` and ``frame_resize.PadWideClips``.)
"""
from __future__ import annotations

import functools
import math
import random
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import TadError
from .masking_generator import TubeMaskingGenerator

IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)
IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)
_PRECISION_BITS = 32 - 8 - 2       # Pillow's PRECISION_BITS: the coefficients are 22-bit fixed point
MAX_FILTERSCALE = 8
_DEFAULT_SCALES = (1, .875, .75, .66)
_SNAP = 3                          # a crop side closer than this to the output extent becomes the output extent
# the fixed offsets in quarter steps of the slack (Ws - w, Hs - h): the four corners and the centre; then, with more_fix_crop, the
# middles of the four edges and the four inner quarter points
_OFFSET_GRID = ((0, 0), (4, 0), (0, 4), (4, 4), (2, 2), (0, 2), (4, 2), (2, 4), (2, 0), (1, 1), (3, 1), (1, 3), (3, 3))

# the crop of one clip: frames[clip][:, y0:y0+h, x0:x0+w]
Crop = namedtuple("Crop", "clip w h x0 y0")


@functools.lru_cache(maxsize=256)
def resample_coefficients(in_size: int, out_size: int):
    """(in_size, ksize, bounds, kk) of Pillow's BILINEAR resample from ``in_size`` to ``out_size`` samples (Resample.c:
    precompute_coeffs with the triangle filter of support 1, then normalize_coeffs_8bpc), in Python floats: bounds [out][2] =
    (xmin, count), kk [out][ksize] int32."""
    if in_size < 1 or out_size < 1:
        raise TadError(f"resample_coefficients: {in_size} -> {out_size} samples")
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    if filterscale > MAX_FILTERSCALE:
        raise TadError(f"GroupMultiScaleCrop: {in_size} -> {out_size} samples shrinks by {scale:.3f}; a filter scale above "
                       f"{MAX_FILTERSCALE} (more than {_lib.MSC_MAX_KSIZE} taps) is not built")
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        weights = []
        ww = 0.0
        for x in range(xmax):
            a = (x + xmin - center + 0.5) * ss
            if a < 0.0:
                a = -a
            w = 1.0 - a if a < 1.0 else 0.0
            weights.append(w)
            ww += w
        for x, w in enumerate(weights):
            if ww != 0.0:
                w /= ww
            kk[xx, x] = int(-0.5 + w * (1 << _PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << _PRECISION_BITS))
        bounds[xx] = xmin, xmax
    bounds.setflags(write=False)
    kk.setflags(write=False)
    return in_size, ksize, bounds, kk


class GroupMultiScaleCrop:
    """transforms.py:91-160.  input_size: S or [S_w, S_h]; scales: crop sizes as shares of the source's short side."""

    def __init__(self, input_size, scales=None, max_distort=1, fix_crop=True, more_fix_crop=True):
        side = [input_size, input_size] if isinstance(input_size, int) else input_size
        if len(side) != 2 or min(side) < 1:
            raise TadError(f"GroupMultiScaleCrop: input_size {input_size!r} must be S or [S_w, S_h]")
        self.input_size = side
        self.scales = list(_DEFAULT_SCALES) if scales is None else scales
        self.max_distort, self.fix_crop, self.more_fix_crop = max_distort, fix_crop, more_fix_crop

    # ------------------------------------------------------------------ the random draws
    def fixed_offsets(self, Ws, Hs, w, h):
        """the (x0, y0) a fixed-offset draw chooses from, in the reference's order: a grid of quarter steps of the slack, rounded down"""
        qx, qy = (Ws - w) // 4, (Hs - h) // 4
        grid = _OFFSET_GRID if self.more_fix_crop else _OFFSET_GRID[:5]
        return [(i * qx, j * qy) for i, j in grid]

    def crop_pairs(self, im_size):
        """the (w, h) crop sizes one draw chooses from, in the reference's order: per scale the truncated share of the source's short
        side, snapped to the output extent of its axis when within 3 of it; the pairs whose scale indices lie at most ``max_distort``
        apart, the height's index outermost"""
        S_w, S_h = self.input_size
        short = min(im_size[0], im_size[1])
        sides = [int(short * share) for share in self.scales]
        snap = lambda side, S: S if abs(side - S) < _SNAP else side
        return [(snap(sw, S_w), snap(sh, S_h)) for i, sh in enumerate(sides) for j, sw in enumerate(sides) if abs(i - j) <= self.max_distort]

    def draw(self, im_size):
        """(w, h, x0, y0) of one clip of source size (Ws, Hs): one ``random.choice`` over the pairs, then one over the fixed offsets --
        or, with ``fix_crop=False``, ``random.randint`` for x0 and then for y0"""
        Ws, Hs = im_size[0], im_size[1]
        w, h = random.choice(self.crop_pairs(im_size))
        if self.fix_crop:
            x0, y0 = random.choice(self.fixed_offsets(Ws, Hs, w, h))
        else:
            x0 = random.randint(0, Ws - w)
            y0 = random.randint(0, Hs - h)
        return w, h, x0, y0

    def plan(self, B, im_size):
        """Consume the random draws for B clips of source size ``im_size`` = (Ws, Hs) (the module docstring gives their order) and
        return the ``Crop`` list, clip by clip.  Host only."""
        return [Crop(b, *self.draw(im_size)) for b in range(B)]

    # ------------------------------------------------------------------ carrying a plan out
    def table(self, plan, B, Hs, Ws):
        """the plan as the kernel's table (kernels.multiscale_crop_table): (int32 CPU tensor, n_hsets, n_vsets)"""
        S_w, S_h = self.input_size
        hsets, vsets, rows = {}, {}, [None] * B
        for c in plan:
            if not 0 <= c.clip < B or rows[c.clip] is not None:
                raise TadError(f"GroupMultiScaleCrop: {c} is not one crop per clip of {B} clips")
            if not (c.w >= 1 and c.h >= 1 and c.x0 >= 0 and c.y0 >= 0 and c.x0 + c.w <= Ws and c.y0 + c.h <= Hs):
                raise TadError(f"GroupMultiScaleCrop: {c} is not inside the {Ws} x {Hs} source")
            rows[c.clip] = (c.clip, c.x0, c.y0, c.w, c.h, hsets.setdefault(c.w, len(hsets)), vsets.setdefault(c.h, len(vsets)))
        if any(r is None for r in rows):
            raise TadError(f"GroupMultiScaleCrop: the plan does not hold one crop per clip of {B} clips")
        table = K.multiscale_crop_table(rows, [resample_coefficients(w, S_w) for w in hsets], [resample_coefficients(h, S_h) for h in vsets],
                                        B, Hs, Ws, S_h, S_w)
        return table, len(hsets), len(vsets)

    def apply(self, frames, plan, out=None, normalize=None):
        """carry out the plan (``plan(B, (Ws, Hs))``, or crops stated by hand) on uint8 frames [B,T,Hs,Ws,3] on the device.  Returns
        uint8 [B,T,S_h,S_w,3], or with ``normalize=(mean, std)`` the f32 clips [B,3,T,S_h,S_w] = (v / 255 - mean) / std."""
        x = frames
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.uint8 and x.dim() == 5 and x.shape[-1] == 3
                and x.is_contiguous() and x.numel() > 0):
            raise TadError("GroupMultiScaleCrop: expected contiguous uint8 frames [B,T,Hs,Ws,3] on the GPU (there is no CPU path)")
        B, T, Hs, Ws, _ = x.shape
        table, nh, nv = self.table(plan, B, Hs, Ws)
        mean, std = normalize if normalize is not None else (None, None)
        if normalize is not None and (len(mean) != 3 or len(std) != 3):
            raise TadError("GroupMultiScaleCrop: mean and std hold one value per RGB channel")
        with torch.cuda.device(x.device):
            # pinned staging + asynchronous copy: the host never waits for the device
            dev = table.pin_memory().to(x.device, non_blocking=True)
            return K.multiscale_crop(x, dev, nh, nv, self.input_size[1], self.input_size[0], mean, std, out)

    def __call__(self, frames, out=None, normalize=None):
        if not isinstance(frames, torch.Tensor) or frames.dim() != 5:
            raise TadError("GroupMultiScaleCrop: expected uint8 frames [B,T,Hs,Ws,3] on the GPU")
        B, _, Hs, Ws, _ = frames.shape
        return self.apply(frames, self.plan(B, (Ws, Hs)), out=out, normalize=normalize)


class DataAugmentationForVideoMAE:
    """datasets.py:9-35, batched: called on uint8 frames [B,T,Hs,Ws,3] on the GPU it returns (the f32 clips [B,3,T,S,S], the masks
    [B, N] as a CPU tensor of 0 / 1), the reference's per-sample ``(process_data, mask)`` for B samples.  ``args`` carries
    ``input_size``, ``mask_type`` ('tube'), ``window_size`` and ``mask_ratio``.  What ``engine_pretrain.train_one_epoch(augment_fn=...)``
    takes."""
    scales = (1, .875, .75, .66)

    def __init__(self, args):
        self.input_mean = list(IMAGENET_DEFAULT_MEAN)
        self.input_std = list(IMAGENET_DEFAULT_STD)
        self.train_augmentation = GroupMultiScaleCrop(args.input_size, list(self.scales))
        if args.mask_type != "tube":
            raise TadError(f"{type(self).__name__}: mask_type {args.mask_type!r} is not built (the reference knows 'tube' alone)")
        self.masked_position_generator = TubeMaskingGenerator(args.window_size, args.mask_ratio)

    def __call__(self, frames):
        clips = self.train_augmentation(frames, normalize=(self.input_mean, self.input_std))
        masks = np.stack([self.masked_position_generator() for _ in range(frames.shape[0])])
        return clips, torch.from_numpy(masks)

    def __repr__(self):
        return (f"({type(self).__name__},\n  crop = GroupMultiScaleCrop({self.train_augmentation.input_size}, "
                f"{self.train_augmentation.scales}),\n  Masked position generator = {self.masked_position_generator},\n)")


class DataAugmentationForVideoMAE_LightCrop(DataAugmentationForVideoMAE):
    scales = (1, 1, .975, .95, .9, .875, .85)
