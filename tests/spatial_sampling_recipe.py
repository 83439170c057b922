"""Spatial sampling fixture G20 (tests/golden/g20_spatial_sampling.npz, written by tools/make_goldens_spatial_sampling.py from the
reference's own ``spatial_sampling`` on CPU torch): its seeded inputs, its cases, and a numpy f32 restatement of the device
arithmetic that include/tad_mi355x.h states for ``tad_spatial_sample`` -- per axis ``src = max(scale * (d + 0.5) - 0.5, 0)``, two
taps, ``l1 = src - i0``, ``l0 = 1 - l1``; the four taps blended columns first, every product and sum rounded to f32 on its own.  The
restatement is the bridge between the reference's results (the goldens; tests/test_spatial_sampling_cpu.py holds it to them within
the reference's own f32 error) and the kernel of csrc/spatial_sample.hip, which must equal it bit for bit.  Test infrastructure
only.

Clips are f32 [B, 3, T, H, W] on the scale of normalised pixels; their uint8 twins [B, T, H, W, 3] give them as
``(v / 255 - mean) / std`` in f32, what ``frames_to_clip`` computes."""
import hashlib

import numpy as np

B, T = 3, 4
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
RECIPE = {"scale": (0.08, 1.0), "aspect_ratio": (0.75, 1.3333)}          # the fine-tuning recipe's ranges

# (key, seed of ``random`` and of numpy's global stream, source (H, W), keywords of SpatialSampling): each names its route
CASES = (
    ("down.37x53", 1, (37, 53), dict(crop_size=16, **RECIPE)),                          # random resized crop, downscale
    ("up.17x19", 2, (17, 19), dict(crop_size=32, **RECIPE)),                            # random resized crop, upscale
    ("s18.37x53", 3, (37, 53), dict(crop_size=18, **RECIPE)),                           # S no multiple of 4: rows off 16-byte alignment
    ("portrait.91x23", 4, (91, 23), dict(crop_size=16, **RECIPE)),
    ("noflip.37x53", 5, (37, 53), dict(crop_size=8, random_horizontal_flip=False, **RECIPE)),
    # jitter to the source's own short side (no resize) + random crop: weights 0 / 1, the output is a slice of the source
    ("scale1.20x27", 6, (20, 27), dict(crop_size=12, min_scale=20, max_scale=20)),
    ("wide1.37x53", 7, (37, 53), dict(crop_size=8, scale=(0.004, 0.005), aspect_ratio=(0.1, 0.12))),   # boxes one pixel wide: i1 clamps
    ("high1.37x53", 8, (37, 53), dict(crop_size=8, scale=(0.004, 0.005), aspect_ratio=(8.5, 10.0))),   # boxes one pixel high
    ("shift.37x53", 9, (37, 53), dict(crop_size=16, motion_shift=True, **RECIPE)),      # one box per frame
    ("fallback.6x120", 10, (6, 120), dict(crop_size=8, **RECIPE)),                      # no attempt fits: the central crop h=6, w=8
    ("jitter.20x27", 11, (20, 27), dict(crop_size=12, min_scale=14, max_scale=24)),     # jitter + random crop
    ("inverse.20x27", 12, (20, 27), dict(crop_size=12, min_scale=14, max_scale=24, inverse_uniform_sampling=True)),
    ("idx0.10x14", 13, (10, 14), dict(spatial_idx=0, crop_size=8, min_scale=8, max_scale=8)),
    ("idx1.10x14", 14, (10, 14), dict(spatial_idx=1, crop_size=8, min_scale=8, max_scale=8)),
    ("idx2.10x14", 15, (10, 14), dict(spatial_idx=2, crop_size=8, min_scale=8, max_scale=8)),
    ("idx0.15x10", 16, (15, 10), dict(spatial_idx=0, crop_size=8, min_scale=8, max_scale=8)),
    ("idx1.15x10", 17, (15, 10), dict(spatial_idx=1, crop_size=8, min_scale=8, max_scale=8)),
    ("idx2.15x10", 18, (15, 10), dict(spatial_idx=2, crop_size=8, min_scale=8, max_scale=8)),
)
CASE_IDS = [c[0] for c in CASES]
EXACT_CASES = ("scale1.20x27",)                                           # 0 differing bits against the reference


def frames(H, W):
    """the uint8 twins [B, T, H, W, 3]: a smooth gradient plus noise per frame and channel"""
    rng = np.random.default_rng(20_000 + 131 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((B, T, H, W, 3), dtype=np.uint8)
    for b in range(B):
        for t in range(T):
            for c in range(3):
                ax, ay = rng.uniform(-1, 1, 2)
                g = ax * xx / W + ay * yy / H
                g = (g - g.min()) / max(g.max() - g.min(), 1e-9)
                v = -20 + g * 295 + rng.normal(0, 25, (H, W))
                out[b, t, :, :, c] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return out


def normalise(u8, mean=MEAN, std=STD):
    """f32 [B, 3, T, H, W] = ((float)v / 255 - mean) / std of uint8 [B, T, H, W, 3], every step rounded to f32 (frames_to_clip's)"""
    v = u8.astype(np.float32) / np.float32(255)
    v = (v - np.asarray(mean, dtype=np.float32)) / np.asarray(std, dtype=np.float32)
    assert v.dtype == np.float32
    return np.ascontiguousarray(v.transpose(0, 4, 1, 2, 3))


def clips(H, W):
    """the f32 clips [B, 3, T, H, W]: the normalised twins"""
    return normalise(frames(H, W))


def inputs_digest():
    h, seen = hashlib.sha256(), set()
    for _, _, size, _ in CASES:
        if size not in seen:
            seen.add(size)
            h.update(clips(*size).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------- the device arithmetic, in numpy f32
def axis_taps(n_in, n_out, d):
    """(i0, i1, l0, l1) of the grid indices d (int array) of a resize from n_in to n_out samples, in f32"""
    f = np.float32
    scale = f(n_in) / f(n_out)
    src = np.maximum(scale * (d.astype(f) + f(0.5)) - f(0.5), f(0))
    assert src.dtype == f
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = src - i0.astype(f)
    l0 = f(1) - l1
    return i0, i1, l0, l1


def sample_frame(frame, win, S):
    """f32 [C, S, S] of one frame [C, H, W] under win = (i, j, h, w, rh, rw, oy, ox, flip)"""
    i, j, h, w, rh, rw, oy, ox, flip = [int(v) for v in win]
    src = frame[:, i:i + h, j:j + w]
    assert src.dtype == np.float32 and src.shape[1:] == (h, w)
    y0, y1, ly0, ly1 = axis_taps(h, rh, oy + np.arange(S))
    cols = S - 1 - np.arange(S) if flip else np.arange(S)
    x0, x1, lx0, lx1 = axis_taps(w, rw, ox + cols)
    a, b = src[:, y0][:, :, x0], src[:, y0][:, :, x1]
    c, d = src[:, y1][:, :, x0], src[:, y1][:, :, x1]
    top = lx0 * a + lx1 * b
    bot = lx0 * c + lx1 * d
    out = ly0[None, :, None] * top + ly1[None, :, None] * bot
    assert out.dtype == np.float32
    return out


def sample(x, windows, S):
    """f32 [B, 3, T, S, S] of the clips x [B, 3, T, H, W] under windows int [B * T, 11] = (clip, frame, i, j, h, w, rh, rw, oy, ox, flip)"""
    out = np.full((x.shape[0], 3, x.shape[2], S, S), np.nan, dtype=np.float32)
    for row in np.asarray(windows):
        b, t = int(row[0]), int(row[1])
        out[b, :, t] = sample_frame(x[b, :, t], row[2:], S)
    assert not np.isnan(out).any()
    return out


def ulp_of(v):
    return float(np.spacing(np.float32(v)))


def bound(g, key):
    """2 * gap + 4 ulp(max |out|): the reference's own f32 coordinate arithmetic puts it up to ``gap`` away from the exact resample, and
    another f32 evaluation order can sit as far away on the other side; the ulp term covers the cases whose gap is a rounding or two"""
    out = g[f"{key}.out"]
    return 2.0 * float(g[f"{key}.gap"]) + 4.0 * ulp_of(np.abs(out).max())
