"""RandAugment of the fine-tune recipe: counterpart of the reference's ``rand_augment.py`` (timm's, "apply for video"), which its
datasets run on the 16 PIL frames of every training clip (dota.py:299-307: ``create_random_augment(input_size, auto_augment=args.aa,
interpolation=args.train_interpolation, do_transforms=DRIVE_TRANSFORMS)`` with ``--aa rand-m6-n3-mstd0.5-inc1`` and ``bicubic``).

Same surface -- ``rand_augment_transform(config_str, hparams, do_transforms)``, ``create_random_augment(...)``, ``RandAugment(ops,
num_layers, choice_weights)``, ``AugmentOp(name, prob, magnitude, hparams)`` -- but, like ``mixup.Mixup`` and
``random_erasing.RandomErasing``, the work is split.  One host routine (``RandAugment.plan``) turns the random draws into one row per
(clip, layer).  A contiguous uint8 batch [B,T,H,W,3] on the GPU is then augmented by HIP kernels (``tad_randaug_apply``: per layer one
apply launch, plus one statistics launch when a clip of the layer runs AutoContrast, Equalize or Contrast; every clip carries out its
own operator inside the launch); the table reaches the device through pinned memory, so a call never waits for the GPU.  The result
is PIL's: lookup-table and ImageEnhance operators bit for bit, the resampling operators in the same double arithmetic
(csrc/randaug.hip, tests/randaug_recipe.py).  There is no CPU path: a CPU tensor raises ``TadError``.

``frames_to_clip`` turns uint8 frames into the normalised f32 clips [B,3,T,H,W] that ``RandomErasing`` and ``Mixup`` take (the
reference's ToTensor, tensor_normalize and permute, bit for bit), so a training loop can keep its frames uint8 up to the device:
``engine.train_one_epoch(augment_fn=...)``.

RNG contract.  Clips run in index order, each as one call of the reference's transform would: ``np.random.choice`` over the op list
(``num_layers`` draws with replacement, numpy's GLOBAL legacy stream); then per chosen op, from Python's GLOBAL ``random`` stream:
``random.random()`` against ``prob`` (0.5; the op is skipped when the draw is larger), ``random.gauss(magnitude, magnitude_std)`` when
``magnitude_std > 0``, the cut to [0, 10], ``random.random()`` for the sign of the ops whose level function negates, and -- only when
``interpolation`` is left random -- one ``random.choice((BILINEAR, BICUBIC))`` PER FRAME of a geometric op (the reference pops
``resample`` in every image call).  All frames of a clip share op and argument.

Not built: the ``w`` key (weighted choice without replacement; ``TadError``), the absolute ``TranslateX`` / ``TranslateY`` and
``PosterizeOriginal`` (in neither op list of the reference nor in ``DRIVE_TRANSFORMS``), resampling filters other than BILINEAR and
BICUBIC (PIL's transform refuses them as well), a hand-stated Rotate by 90, 180 or 270 degrees (PIL transposes there; ``TadError``;
the level map stays within 30 degrees).
"""
from __future__ import annotations

import math
import random
import re
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import TadError

BILINEAR, BICUBIC = 2, 3       # PIL's Image.Resampling values
_FILL = (128, 128, 128)
_MAX_LEVEL = 10.0
_HPARAMS_DEFAULT = {"translate_const": 250, "img_mean": _FILL}
_RANDOM_INTERPOLATION = (BILINEAR, BICUBIC)

DRIVE_TRANSFORMS = ["AutoContrast", "Equalize", "Invert", "Rotate", "Color", "Contrast", "Brightness", "Sharpness", "ShearX", "ShearY"]
_RAND_TRANSFORMS = ["AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast",
                    "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel"]
_RAND_INCREASING_TRANSFORMS = ["AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing", "SolarizeAdd",
                               "ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing", "ShearX", "ShearY",
                               "TranslateXRel", "TranslateYRel"]


def _randomly_negate(v):
    return -v if random.random() > 0.5 else v


def _rotate_level(level, _hp):
    return _randomly_negate((level / _MAX_LEVEL) * 30.0)


def _enhance_level(level, _hp):
    return (level / _MAX_LEVEL) * 1.8 + 0.1


def _enhance_increasing_level(level, _hp):
    return 1.0 + _randomly_negate((level / _MAX_LEVEL) * 0.9)


def _shear_level(level, _hp):
    return _randomly_negate((level / _MAX_LEVEL) * 0.3)


def _translate_rel_level(level, hp):
    return _randomly_negate((level / _MAX_LEVEL) * hp.get("translate_pct", 0.45))


def _posterize_level(level, _hp):
    return int((level / _MAX_LEVEL) * 4)


def _posterize_increasing_level(level, hp):
    return 4 - _posterize_level(level, hp)


def _solarize_level(level, _hp):
    return int((level / _MAX_LEVEL) * 256)


def _solarize_increasing_level(level, hp):
    return 256 - _solarize_level(level, hp)


def _solarize_add_level(level, _hp):
    return int((level / _MAX_LEVEL) * 110)


# name -> (level function or None, kernel operator of the name; None = affine, stated by _affine_coefficients)
_OPS = {
    "AutoContrast": (None, _lib.RA_AUTOCONTRAST), "Equalize": (None, _lib.RA_EQUALIZE), "Invert": (None, _lib.RA_INVERT),
    "Rotate": (_rotate_level, None),
    "Posterize": (_posterize_level, _lib.RA_POSTERIZE), "PosterizeIncreasing": (_posterize_increasing_level, _lib.RA_POSTERIZE),
    "Solarize": (_solarize_level, _lib.RA_SOLARIZE), "SolarizeIncreasing": (_solarize_increasing_level, _lib.RA_SOLARIZE),
    "SolarizeAdd": (_solarize_add_level, _lib.RA_SOLARIZE_ADD),
    "Color": (_enhance_level, _lib.RA_COLOR), "ColorIncreasing": (_enhance_increasing_level, _lib.RA_COLOR),
    "Contrast": (_enhance_level, _lib.RA_CONTRAST), "ContrastIncreasing": (_enhance_increasing_level, _lib.RA_CONTRAST),
    "Brightness": (_enhance_level, _lib.RA_BRIGHTNESS), "BrightnessIncreasing": (_enhance_increasing_level, _lib.RA_BRIGHTNESS),
    "Sharpness": (_enhance_level, _lib.RA_SHARPNESS), "SharpnessIncreasing": (_enhance_increasing_level, _lib.RA_SHARPNESS),
    "ShearX": (_shear_level, None), "ShearY": (_shear_level, None),
    "TranslateXRel": (_translate_rel_level, None), "TranslateYRel": (_translate_rel_level, None),
}
OP_NAMES = tuple(_OPS)          # PlanRow.op indexes this
GEOMETRIC = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
_ENHANCE = (_lib.RA_COLOR, _lib.RA_CONTRAST, _lib.RA_BRIGHTNESS, _lib.RA_SHARPNESS)

# one row of a plan: clip and layer index, op = index into OP_NAMES, applied = the op's coin (False: the layer leaves the clip as it
# is), arg = what the op's level function returned (None for the ops without one, and when not applied), resample = per frame BILINEAR
# or BICUBIC for an applied geometric op, else None
PlanRow = namedtuple("PlanRow", "clip layer op applied arg resample")


class AugmentOp:
    """rand_augment.py:337-382: one operator with its probability and magnitude.  ``draw(T)`` consumes the random draws of one call
    on a clip of T frames and returns (applied, arg, resample)."""

    def __init__(self, name, prob=0.5, magnitude=10, hparams=None):
        hparams = hparams or _HPARAMS_DEFAULT
        if name not in _OPS:
            raise TadError(f"RandAugment: operator {name!r} is not built (supported: {', '.join(OP_NAMES)})")
        self.name = name
        self.level_fn = _OPS[name][0]
        self.prob = prob
        self.magnitude = magnitude
        self.hparams = hparams.copy()
        self.fill = tuple(int(v) for v in (hparams["img_mean"] if "img_mean" in hparams else _FILL))
        self.resample = hparams["interpolation"] if "interpolation" in hparams else _RANDOM_INTERPOLATION
        if name in GEOMETRIC and not isinstance(self.resample, (list, tuple)) and self.resample not in _RANDOM_INTERPOLATION:
            raise TadError(f"RandAugment: resampling filter {self.resample!r}: the affine operators take BILINEAR (2) or BICUBIC (3)")
        self.magnitude_std = self.hparams.get("magnitude_std", 0)

    def draw(self, T):
        if self.prob < 1.0 and random.random() > self.prob:
            return False, None, None
        magnitude = self.magnitude
        if self.magnitude_std and self.magnitude_std > 0:
            magnitude = random.gauss(magnitude, self.magnitude_std)
        magnitude = min(_MAX_LEVEL, max(0, magnitude))
        arg = self.level_fn(magnitude, self.hparams) if self.level_fn is not None else None
        resample = None
        if self.name in GEOMETRIC:
            if isinstance(self.resample, (list, tuple)):
                resample = tuple(random.choice(self.resample) for _ in range(T))
            else:
                resample = (self.resample,) * T
        return True, arg, resample


def rand_augment_ops(magnitude=10, hparams=None, transforms=None):
    hparams = hparams or _HPARAMS_DEFAULT
    transforms = transforms or _RAND_TRANSFORMS
    return [AugmentOp(name, prob=0.5, magnitude=magnitude, hparams=hparams) for name in transforms]


def _affine_coefficients(name, arg, W, H):
    """the six coefficients PIL's Image.transform(AFFINE) receives, stated as the reference's functions and Image.rotate state them
    (None: Image.rotate returns a copy)"""
    if name == "Rotate":
        angle = arg % 360.0
        if angle == 0:
            return None
        if angle in (90.0, 180.0, 270.0):
            # (Image.rotate turns these into a transpose, which is not the affine map's pixels; the policy stays within 30 degrees)
            raise TadError(f"RandAugment: Rotate by {arg} degrees is not built (PIL transposes at 90, 180 and 270 degrees)")
        cx, cy = W / 2.0, H / 2.0
        angle = -math.radians(angle)
        m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
        m[2] = m[0] * -cx + m[1] * -cy + m[2]
        m[5] = m[3] * -cx + m[4] * -cy + m[5]
        m[2] += cx
        m[5] += cy
        return m
    if name == "ShearX":
        return [1, arg, 0, 0, 1, 0]
    if name == "ShearY":
        return [1, 0, 0, arg, 1, 0]
    if name == "TranslateXRel":
        return [1, 0, arg * W, 0, 1, 0]
    return [1, 0, 0, 0, 1, arg * H]


class RandAugment:
    """rand_augment.py:462-478.  ops: ``AugmentOp`` list; num_layers: operators drawn per clip (with replacement);
    choice_weights: must be None (the weighted choice is not built)."""

    def __init__(self, ops, num_layers=2, choice_weights=None):
        if choice_weights is not None:
            raise TadError("RandAugment: the weighted choice (config key 'w') is not built")
        if not 0 <= num_layers <= _lib.RANDAUG_MAX_LAYERS:
            raise TadError(f"RandAugment: num_layers={num_layers} must be in [0, {_lib.RANDAUG_MAX_LAYERS}]")
        self.ops = ops
        self.num_layers = num_layers
        self.choice_weights = choice_weights

    # ------------------------------------------------------------------ the random draws
    def plan(self, B, T):
        """Consume the random draws for B clips of T frames (the module docstring gives their order) and return the ``PlanRow`` list,
        clip by clip, layer by layer.  Host only."""
        rows = []
        for b in range(B):
            chosen = np.random.choice(len(self.ops), self.num_layers)
            for layer, k in enumerate(chosen):
                op = self.ops[int(k)]
                applied, arg, resample = op.draw(T)
                rows.append(PlanRow(b, layer, OP_NAMES.index(op.name), applied, arg, resample))
        return rows

    # ------------------------------------------------------------------ carrying a plan out
    def _fill_of(self, name):
        for op in self.ops:
            if op.name == name:
                return op.fill
        return _FILL

    def table(self, rows, B, T, H, W):
        """the plan as the kernels' table (kernels.randaug_table): (int32 CPU tensor, statistics bit mask)"""
        L = self.num_layers
        layers = [[None] * B for _ in range(L)]
        for r in rows:
            if not (0 <= r.clip < B and 0 <= r.layer < L) or layers[r.layer][r.clip] is not None or not 0 <= r.op < len(OP_NAMES):
                raise TadError(f"RandAugment: {r} is not one row per (clip, layer) of {B} clips and {L} layers")
            name = OP_NAMES[r.op]
            kop, iarg, farg, coefs, mask = _lib.RA_COPY, 0, 0.0, None, 0
            if r.applied:
                kop = _OPS[name][1]
                if kop is None:
                    coefs = _affine_coefficients(name, r.arg, W, H)
                    kop = _lib.RA_COPY if coefs is None else _lib.RA_AFFINE
                    if r.resample is None or len(r.resample) != T or any(m not in _RANDOM_INTERPOLATION for m in r.resample):
                        raise TadError(f"RandAugment: {r}: a geometric op needs BILINEAR or BICUBIC for each of the {T} frames")
                    mask = sum(1 << t for t, m in enumerate(r.resample) if m == BICUBIC)
                elif kop in _ENHANCE:
                    farg = float(r.arg)
                elif kop == _lib.RA_POSTERIZE:
                    kop, iarg = (_lib.RA_COPY, 0) if r.arg >= 8 else (kop, int(r.arg))
                elif kop in (_lib.RA_SOLARIZE, _lib.RA_SOLARIZE_ADD):
                    iarg = int(r.arg)
            layers[r.layer][r.clip] = (r.clip, kop, iarg, farg, coefs, self._fill_of(name), mask)
        if any(row is None for layer in layers for row in layer):
            raise TadError(f"RandAugment: the plan does not hold one row per (clip, layer) of {B} clips and {L} layers")
        return K.randaug_table(layers, B, T)

    def apply(self, x, rows):
        """carry out the plan ``rows`` (``plan(B, T)``, or rows stated by hand) on uint8 frames [B,T,H,W,3] on the device"""
        single = x.dim() == 4
        if single:
            x = x.unsqueeze(0)
        if not (x.is_cuda and x.dtype == torch.uint8 and x.dim() == 5 and x.shape[-1] == 3 and x.is_contiguous() and x.numel() > 0):
            raise TadError(f"RandAugment: expected contiguous uint8 frames [B,T,H,W,3] (or [T,H,W,3]) on the GPU, got {x.dtype} "
                           f"{tuple(x.shape)} on {x.device} (there is no CPU path)")
        B, T, H, W, _ = x.shape
        table, stats = self.table(rows, B, T, H, W)
        with torch.cuda.device(x.device):
            # pinned staging + asynchronous copy: the host never waits for the device
            out = K.randaug_apply(x, table.pin_memory().to(x.device, non_blocking=True), stats)
        return out[0] if single else out

    def __call__(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() not in (4, 5):
            raise TadError("RandAugment: expected uint8 frames [B,T,H,W,3] or [T,H,W,3] on the GPU")
        B, T = (1, x.shape[0]) if x.dim() == 4 else tuple(x.shape[:2])
        return self.apply(x, self.plan(B, T))


def parse_config(config_str):
    """the reference's config string ('rand-m6-n3-mstd0.5-inc1'): {'magnitude', 'num_layers', 'magnitude_std' (or None), 'increasing'}.
    Keys are read as the reference reads them: 'inc' selects the increasing list for ANY value (bool of a non-empty string)."""
    config = config_str.split("-")
    if config[0] != "rand":
        raise TadError(f"RandAugment: config {config_str!r} must start with 'rand'")
    out = {"magnitude": _MAX_LEVEL, "num_layers": 2, "magnitude_std": None, "increasing": False}
    for c in config[1:]:
        cs = re.split(r"(\d.*)", c)
        if len(cs) < 2:
            continue
        key, val = cs[:2]
        if key == "mstd":
            out["magnitude_std"] = float(val)
        elif key == "inc":
            out["increasing"] = out["increasing"] or bool(val)
        elif key == "m":
            out["magnitude"] = int(val)
        elif key == "n":
            out["num_layers"] = int(val)
        elif key == "w":
            raise TadError("RandAugment: the weighted choice (config key 'w') is not built")
    return out


def rand_augment_transform(config_str, hparams, do_transforms=None):
    """rand_augment.py:481-533.  As there, 'mstd' reaches the ops through ``hparams.setdefault("magnitude_std", ...)`` on the caller's
    dictionary, and ``do_transforms`` replaces the op list."""
    cfg = parse_config(config_str)
    if cfg["magnitude_std"] is not None:
        hparams.setdefault("magnitude_std", cfg["magnitude_std"])
    transforms = _RAND_INCREASING_TRANSFORMS if cfg["increasing"] else _RAND_TRANSFORMS
    if do_transforms is not None:
        transforms = do_transforms
    return RandAugment(rand_augment_ops(magnitude=cfg["magnitude"], hparams=hparams, transforms=transforms), cfg["num_layers"])


def _pil_interp(method):
    if method == "bicubic":
        return BICUBIC
    if method in ("lanczos", "hamming"):
        raise TadError(f"RandAugment: interpolation {method!r}: the affine operators take bilinear or bicubic")
    return BILINEAR


def create_random_augment(input_size, auto_augment=None, interpolation="bilinear", do_transforms=None):
    """video_transforms.create_random_augment (video_transforms.py:637-671); returns the ``RandAugment`` itself (the reference wraps it
    in a one-element Compose)."""
    img_size = input_size[-2:] if isinstance(input_size, tuple) else input_size
    if auto_augment:
        assert isinstance(auto_augment, str)
        img_size_min = min(img_size) if isinstance(img_size, tuple) else img_size
        aa_params = {"translate_const": int(img_size_min * 0.45)}
        if interpolation and interpolation != "random":
            aa_params["interpolation"] = _pil_interp(interpolation)
        if auto_augment.startswith("rand"):
            return rand_augment_transform(auto_augment, aa_params, do_transforms)
    raise NotImplementedError


def frames_to_clip(x, mean, std, out=None):
    """uint8 frames [B,T,H,W,3] on the GPU -> f32 clips [B,3,T,H,W] = (x / 255 - mean) / std: the reference's ToTensor,
    tensor_normalize and permute (dota.py:308-316) in f32 with IEEE division, bit for bit.  What ``RandomErasing`` and ``Mixup`` take."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.uint8 and x.dim() == 5 and x.shape[-1] == 3 and x.is_contiguous()):
        raise TadError("frames_to_clip: expected contiguous uint8 frames [B,T,H,W,3] on the GPU (there is no CPU path)")
    if len(mean) != 3 or len(std) != 3:
        raise TadError("frames_to_clip: mean and std hold one value per RGB channel")
    with torch.cuda.device(x.device):
        return K.frames_to_clip(x, mean, std, out)
