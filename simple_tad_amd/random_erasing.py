"""RandomErasing of the fine-tune recipe: counterpart of the reference's ``random_erasing.RandomErasing`` (random_erasing.py:27-173,
timm's), which its datasets apply to every normalised training clip (dota.py:318-329, dada.py: ``RandomErasing(reprob, mode=remode,
max_count=recount, num_splits=recount, max_area=0.1, device="cpu")`` with ``--reprob 0.25 --remode pixel --recount 1``) in "cube" mode:
one box per clip, shared by its frames, with fresh normal noise per frame.

Same surface -- constructor arguments, defaults, attribute names, ``__call__(x) -> x`` erased in place -- but, like ``mixup.Mixup``, the
work is split.  One host routine (``RandomErasing.plan``) turns the random draws into a list of boxes.  A contiguous f32 clip batch
[B,C,T,H,W] on the GPU is then erased by ONE HIP launch (``tad_erase_clips``: it stores the elements inside the boxes and reads nothing);
the box table reaches the device through pinned memory, so a call never waits for the GPU, and a batch without a box launches nothing.
The operator therefore runs on the batch once it is on the device (``engine.train_one_epoch(erase_fn=...)``, before ``mixup_fn``), and
a host-fed loop can leave it out of its CPU workers.  Anything else (CPU tensors, the reference's [T,C,H,W] and [C,H,W] shapes, other
floating dtypes, non-contiguous views) is erased by torch expressions that state the same plan.

RNG contract.  The draws come from Python's GLOBAL ``random`` stream with the reference's calls in its order, so a script seeded like
the reference erases the same boxes.  Clips run in index order; per clip (``cube``) or per frame of each clip (``cube=False``):
``random.random()`` against ``probability``; ``randint(min_count, max_count)`` only when the two differ; per box up to 100 attempts
(``cube``) or 10 (per frame, and a [C,H,W] image), each ``uniform(min_area, max_area)`` and ``uniform(*log_aspect_ratio)``, and on a fit
(``w < W and h < H``) ``randint(0, H - h)``, ``randint(0, W - w)``.  A box whose attempts all fail is left out.

num_splits quirk (random_erasing.py:156-159).  The reference takes the first axis of a 4-d input as a batch and keeps its first
``len // num_splits`` entries clean when ``num_splits > 1``; the datasets hand it a clip as [T,C,H,W] with ``num_splits=recount``, so
``--recount 2`` leaves the first ``T // 2`` FRAMES of every clip untouched.  Reproduced: a box spans the frames [T // num_splits, T).

Noise.  On a CPU [T,C,H,W] / [C,H,W] tensor the values are the reference's own expressions -- ``torch.empty((C,h,w)).normal_()`` from
torch's default generator, once per box and frame -- and the result is bit-identical to the reference under ``random.seed`` +
``torch.manual_seed`` (tests/golden/g15_random_erasing.npz).  The device cannot reproduce that stream, so the kernel generates the values
itself: a counter-based function of (seed, sample, box, c, t, y - y0, x - x0) defined in include/tad_mi355x.h (hash + Box-Muller;
``pixel``: one value per element, ``rand``: one per (box, frame, channel), ``const``: 0).  ``seed`` is one
``torch.randint(0, 2**31 - 1, (1,))`` from torch's default CPU generator per call in ``rand`` / ``pixel`` mode, drawn whether or not a
clip is erased (the stream position does not depend on the plan); ``const`` draws nothing.
"""
from __future__ import annotations

import math
import random

import torch

from . import kernels as K
from ._lib import ERASE_CONST, ERASE_PIXEL, ERASE_RAND, TadError


def _get_pixels(per_pixel, rand_color, patch_size, dtype=torch.float32, device="cuda"):
    """random_erasing.py:11-24: the values of one (C, h, w) patch"""
    if per_pixel:
        return torch.empty(patch_size, dtype=dtype, device=device).normal_()
    if rand_color:
        return torch.empty((patch_size[0], 1, 1), dtype=dtype, device=device).normal_()
    return torch.zeros((patch_size[0], 1, 1), dtype=dtype, device=device)


class RandomErasing:
    """random_erasing.py:27-78.  probability: chance that a clip (frame, image) is erased; min_area / max_area: share of the image a
    box takes, divided by the number of boxes; min_aspect / max_aspect: its aspect ratio (log-uniform); mode: 'const' (zeros), 'rand'
    (one normal value per channel, box and frame) or 'pixel' (one per element); min_count / max_count: boxes per clip; num_splits: see
    the module docstring; device: kept for the reference's surface (values are made where the clip lives); cube: one box per clip
    shared by its frames (the datasets' mode) instead of boxes per frame."""

    def __init__(self, probability=0.5, min_area=0.02, max_area=1 / 3, min_aspect=0.01, max_aspect=None, mode="const", min_count=1,
                 max_count=None, num_splits=0, device="cuda", cube=True):
        self.probability = probability
        self.min_area = min_area
        self.max_area = max_area
        max_aspect = max_aspect or 1 / min_aspect
        self.log_aspect_ratio = (math.log(min_aspect), math.log(max_aspect))
        self.min_count = min_count
        self.max_count = max_count or min_count
        self.num_splits = num_splits
        mode = mode.lower()
        self.rand_color = False
        self.per_pixel = False
        self.cube = cube
        if mode == "rand":
            self.rand_color = True
        elif mode == "pixel":
            self.per_pixel = True
        else:
            assert not mode or mode == "const"
        self.device = device

    # ------------------------------------------------------------------ the random draws
    def _draw(self, out, sample, t0, t1, H, W, attempts):
        """random_erasing.py:80-107 / :109-149: the boxes of one coin flip, appended to ``out``"""
        if random.random() > self.probability:
            return
        area = H * W
        count = self.min_count if self.min_count == self.max_count else random.randint(self.min_count, self.max_count)
        for _ in range(count):
            for _ in range(attempts):
                target_area = random.uniform(self.min_area, self.max_area) * area / count
                aspect_ratio = math.exp(random.uniform(*self.log_aspect_ratio))
                h = int(round(math.sqrt(target_area * aspect_ratio)))
                w = int(round(math.sqrt(target_area / aspect_ratio)))
                if w < W and h < H:
                    top = random.randint(0, H - h)
                    left = random.randint(0, W - w)
                    out.append((sample, t0, t1, top, top + h, left, left + w))
                    break

    def plan(self, B, T, H, W, image=False):
        """Consume the random draws for B clips of T frames of H x W (``image``: one [C,H,W] image, B = T = 1) and return the boxes
        ``(sample, t0, t1, y0, y1, x0, x1)`` in the order the reference writes them: where boxes of a sample overlap, an element ends
        with the value of the last one.  A box may be empty (h or w rounded to 0), as in the reference."""
        boxes = []
        if image:
            self._draw(boxes, 0, 0, 1, H, W, 10)
            return boxes
        first = T // self.num_splits if self.num_splits > 1 else 0
        for b in range(B):
            if self.cube:
                self._draw(boxes, b, first, T, H, W, 100)
            else:
                for t in range(first, T):
                    self._draw(boxes, b, t, t + 1, H, W, 10)
        return boxes

    # ------------------------------------------------------------------ the two ways to carry a plan out
    @property
    def _mode(self):
        return ERASE_PIXEL if self.per_pixel else ERASE_RAND if self.rand_color else ERASE_CONST

    @staticmethod
    def _fused(x):
        return x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 5 and x.numel() > 0

    def _erase_torch(self, frames, boxes):
        """the plan as the reference's expressions, in place: ``frames(sample, t)`` = the [C,H,W] view of one frame"""
        for sample, t0, t1, y0, y1, x0, x1 in boxes:
            for t in range(t0, t1):
                img = frames(sample, t)
                img[:, y0:y1, x0:x1] = _get_pixels(self.per_pixel, self.rand_color, (img.shape[0], y1 - y0, x1 - x0), dtype=img.dtype,
                                                   device=img.device)

    def _erase_hip(self, x, boxes):
        B, _, T, H, W = x.shape
        seed = 0
        if self._mode != ERASE_CONST:
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())  # (a CPU tensor: no device sync)
        if not boxes:
            return
        # (an empty box -- h or w rounded to 0 -- keeps its row, so that a row's index, which keys the noise, is its index in plan())
        table = K.erase_box_table([(s, self._mode, *rest) for s, *rest in boxes], B, T, H, W)
        with torch.cuda.device(x.device):
            # pinned staging + asynchronous copy: the host never waits for the device (the caching host allocator keeps the staging
            # block alive until the copy has run)
            K.erase_clips(x, table.pin_memory().to(x.device, non_blocking=True), seed)
            torch.autograd.graph.increment_version(x)  # (raw-pointer write: tell autograd as an in-place op would)

    def __call__(self, x):
        if not x.is_floating_point():
            raise TadError(f"RandomErasing: expected a normalised floating-point clip, got {x.dtype} {tuple(x.shape)} (the noise is "
                           "N(0, 1) in normalised space: erase after the uint8 input stage has normalised the frames)")
        if x.dim() == 3:        # [C,H,W] (random_erasing.py:152-153)
            boxes = self.plan(1, 1, *x.shape[1:], image=True)
            frames = lambda s, t: x
        elif x.dim() == 4:      # the reference's clip [T,C,H,W] (:155-172)
            boxes = self.plan(1, x.shape[0], *x.shape[2:])
            frames = lambda s, t: x[t]
        elif x.dim() == 5:      # a batch [B,C,T,H,W]: each clip in turn, as the datasets erase them
            boxes = self.plan(x.shape[0], *x.shape[2:])
            if self._fused(x):
                self._erase_hip(x, boxes)
                return x
            frames = lambda s, t: x[s, :, t]
        else:
            raise ValueError(f"RandomErasing: expected [B,C,T,H,W] clips, a [T,C,H,W] clip or a [C,H,W] image, got {tuple(x.shape)}")
        with torch.no_grad():
            self._erase_torch(frames, boxes)
        return x
