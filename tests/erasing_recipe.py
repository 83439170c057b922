"""Seeded inputs of the RandomErasing fixture G15 (tests/golden/g15_random_erasing.npz, written by tools/make_goldens_erasing.py from the
reference's own ``random_erasing.RandomErasing``), and a float64 restatement of the device noise (include/tad_mi355x.h).  The fixture
holds results only; every input is regenerated from here.

Cases ``<mode>.<configuration>.<seed>``: a batch [B,C,T,H,W] whose clips are erased one after the other, as [T,C,H,W] views, with one
continuing ``random`` stream (``random.seed(seed)`` and ``torch.manual_seed(seed)`` before the first clip).  Shapes: B = 4, C = 3,
T in {4, 5}, H x W in {20 x 20, 18 x 22} (W % 4 != 0, H != W, odd T for the num_splits quirk).  The seeds were picked on the CPU so that
every case with 0 < p < 1 erases at least one clip and keeps at least one, and every other case has at least one box
(tests/test_erasing_cpu.py asserts it)."""
import hashlib

import numpy as np
import torch

import golden_recipe as R

CONFIGS = {
    "recipe": dict(probability=0.25, max_count=1, num_splits=1, max_area=0.1),     # run_frame_finetuning.py:111-116, dota.py:319-326
    "p1": dict(probability=1.0),
    "count2": dict(probability=1.0, max_count=2, num_splits=2),                   # --recount 2: the first T // 2 frames stay clean
    "frames": dict(probability=0.5, cube=False),
}
SQUARE4, WIDE5, WIDE4, SQUARE5 = (4, 3, 4, 20, 20), (4, 3, 5, 18, 22), (4, 3, 4, 18, 22), (4, 3, 5, 20, 20)   # [B,C,T,H,W]
# (mode, configuration, seed, shape)
CASES = (
    ("pixel", "recipe", 1, SQUARE4),
    ("pixel", "recipe", 2, WIDE5),
    ("const", "p1", 202, WIDE4),
    ("rand", "p1", 203, SQUARE5),
    ("pixel", "p1", 204, WIDE4),
    ("pixel", "count2", 305, WIDE5),
    ("const", "count2", 310, SQUARE5),
    ("pixel", "frames", 408, SQUARE4),
    ("rand", "frames", 412, WIDE5),
)
SAMPLE_STRIDE = 13   # the strided sample of the erased batch stored beside its digest
MODE_ID = {"const": 0, "rand": 1, "pixel": 2}


def cases():
    """(key, mode, configuration name, seed, batch shape) of every golden case"""
    for mode, name, seed, shape in CASES:
        yield f"{mode}.{name}.{seed}", mode, name, seed, shape


def erasing_kwargs(mode, name):
    return dict(CONFIGS[name], mode=mode, device="cpu")


def clip(key, shape):
    return R.clip_for("g15." + key, shape, seed=15)


def digest(t):
    """SHA-256 of the tensor's bytes (contiguous, host) as uint8 [32]"""
    return np.frombuffer(hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).digest(), dtype=np.uint8)


def sample(t):
    return t.detach().cpu().contiguous().flatten()[::SAMPLE_STRIDE].numpy()


def pack_mask(mask):
    return np.packbits(np.asarray(mask, dtype=bool).reshape(-1))


def unpack_mask(packed, shape):
    n = int(np.prod(shape))
    return np.unpackbits(packed)[:n].astype(bool).reshape(shape)


def owners(boxes, shape):
    """int32 [B,C,T,H,W]: the index in ``boxes`` = [(sample, t0, t1, y0, y1, x0, x1), ...] of the LAST box that covers an element, -1
    where none does (the reference writes the boxes in this order, so the last one's values stay)"""
    own = np.full(shape, -1, dtype=np.int32)
    for k, (s, t0, t1, y0, y1, x0, x1) in enumerate(boxes):
        own[s, :, t0:t1, y0:y1, x0:x1] = k
    return own


# ------------------------------------------------------------------ the device noise, restated in float64 (include/tad_mi355x.h)
_M32 = np.uint64(0xFFFFFFFF)


def _u(v):
    return np.asarray(v, dtype=np.int64).astype(np.uint64) & _M32


def hash32(a, b, s):
    x = (_u(a) * np.uint64(0x9E3779B1) + _u(b) * np.uint64(0x85EBCA77) + _u(s)) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def normal_of(k):
    k = _u(k)
    k2 = hash32(0, 0, (k + np.uint64(0x6A09E667)) & _M32)
    u1 = ((k >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (k2 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def device_values(boxes, mode, shape, seed):
    """float64 [B,C,T,H,W] of what tad_erase_clips writes for ``boxes`` (as ``owners``; an empty box stands for a row the kernel
    ignores and keeps the indices of the rows behind it) in ``mode`` (one name, or one per box) with ``seed``, and the owner map;
    elements outside every box hold NaN"""
    B, C, T, H, W = shape
    out = np.full(shape, np.nan)
    c = np.arange(C).reshape(C, 1, 1, 1)
    modes = [mode] * len(boxes) if isinstance(mode, str) else list(mode)
    for k, (s, t0, t1, y0, y1, x0, x1) in enumerate(boxes):
        if t1 <= t0 or y1 <= y0 or x1 <= x0:
            continue
        mode = modes[k]
        t = np.arange(t0, t1).reshape(1, -1, 1, 1)
        dy = np.arange(y1 - y0).reshape(1, 1, -1, 1)
        dx = np.arange(x1 - x0).reshape(1, 1, 1, -1)
        key_row = hash32(c, t, hash32(s, k, seed))
        if mode == "pixel":
            val = normal_of(hash32(dy, dx, key_row))
        elif mode == "rand":
            val = np.broadcast_to(normal_of(hash32(0, 0, key_row)), (C, t1 - t0, y1 - y0, x1 - x0))
        else:
            val = np.zeros((C, t1 - t0, y1 - y0, x1 - x0))
        out[s, :, t0:t1, y0:y1, x0:x1] = val
    return out, owners(boxes, shape)
