"""Seeded inputs of the Mixup / CutMix fixture G14 (tests/golden/g14_mixup.npz, written by tools/make_goldens_mixup.py from the
reference's own ``mixup.Mixup``).  The fixture holds results only; every input is regenerated from here.

Cases: mode (batch / pair / elem) x configuration x numpy seed.  The clip shape follows the seed, so that every mode and configuration
meets a clip with T < H (pair mode cuts its box to T), one with H != W and one whose W is not a multiple of 4 (the scalar path)."""
import hashlib

import numpy as np
import torch

import golden_recipe as R

NUM_CLASSES = 5
SMOOTHING = 0.1
MODES = ("batch", "pair", "elem")
CONFIGS = {
    "mixup": dict(mixup_alpha=0.8, cutmix_alpha=0.0),
    "cutmix": dict(mixup_alpha=0.0, cutmix_alpha=1.0),
    "switch": dict(mixup_alpha=0.8, cutmix_alpha=1.0, switch_prob=0.5),
    "prob": dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.5),
    "minmax": dict(mixup_alpha=0.8, cutmix_alpha=1.0, cutmix_minmax=(0.2, 0.8)),
}
SEEDS = (101, 102, 103, 104)
SHAPES = {101: (4, 3, 4, 12, 16), 102: (6, 3, 2, 10, 7), 103: (2, 3, 8, 8, 8), 104: (8, 2, 3, 9, 20)}   # [B,C,T,H,W]
SAMPLE_STRIDE = 13   # the strided sample of the mixed clip stored beside its digest


def cases():
    """(key, mode, configuration name, numpy seed, clip shape) of every golden case"""
    for mode in MODES:
        for name in CONFIGS:
            for seed in SEEDS:
                yield f"{mode}.{name}.{seed}", mode, name, seed, SHAPES[seed]


def mixup_kwargs(mode, name):
    return dict(CONFIGS[name], mode=mode, label_smoothing=SMOOTHING, num_classes=NUM_CLASSES)


def clip(key, shape):
    return R.clip_for("g14." + key, shape, seed=14)


def labels(key, batch):
    g = torch.Generator().manual_seed(R._seed_for("g14.labels." + key, 14))
    return torch.randint(0, NUM_CLASSES, (batch,), generator=g)


def digest(t):
    """SHA-256 of the tensor's bytes (contiguous, host) as uint8 [32]"""
    return np.frombuffer(hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).digest(), dtype=np.uint8)


def sample(t):
    return t.detach().cpu().contiguous().flatten()[::SAMPLE_STRIDE].numpy()


# the fine-tune trajectory of G14: golden_recipe.G12's six micro-batches and schedules, mixed by Mixup(0.8, 1.0, smoothing 0.1, 'batch')
TRAJECTORY_SEED = 14
TRAJECTORY_MIXUP = dict(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=R.TINY["num_classes"], mode="batch")


def soft_target_ce_fp64(logits, target):
    """the soft-target criterion as a plain fp64 torch expression (what the reference's trajectory was driven with)"""
    return torch.sum(-target.double() * torch.log_softmax(logits.double(), dim=-1), dim=-1).mean()
