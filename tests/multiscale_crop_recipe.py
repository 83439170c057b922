"""Multi-scale crop fixture G18 (tests/golden/g18_multiscale_crop.npz, written by tools/make_goldens_multiscale_crop.py from the
reference's own ``transforms.GroupMultiScaleCrop`` and PIL): its seeded input frames, its cases, and a numpy restatement of the plan
(the draws from Python's global ``random``) and of Pillow's 8-bit BILINEAR resize -- per-axis coefficients in doubles, rounded to
22-bit integers; the horizontal pass to a rounded byte, then the vertical pass over those bytes.  The restatement is the bridge
between PIL's results (the goldens; tests/test_multiscale_crop_cpu.py holds it to them byte for byte) and the kernel of
csrc/multiscale_crop.hip, which states the same integer arithmetic.  Test infrastructure only.

Frames are uint8 [H, W, 3] (RGB); clips [B, T, H, W, 3]."""
import hashlib
import math
import random

import numpy as np

B, T = 3, 2
PRECISION_BITS = 32 - 8 - 2       # Pillow's: coefficients are 22-bit fixed point
DEFAULT_SCALES = (1, .875, .75, .66)
LIGHT_SCALES = (1, 1, .975, .95, .9, .875, .85)

# (key, seed of ``random``, source (Hs, Ws), output S, keywords of GroupMultiScaleCrop, kind of input frames)
CASES = (
    ("down.45x80.s1", 1, (45, 80), 32, {}, "noise"),                    # a mild downscale; four seeds of the default recipe
    ("down.45x80.s2", 2, (45, 80), 32, {}, "noise"),
    ("down.45x80.s5", 5, (45, 80), 32, {}, "noise"),
    ("down.45x80.s8", 8, (45, 80), 32, {}, "noise"),
    ("up.20x23", 3, (20, 23), 32, {}, "noise"),                         # an upscale with odd row bytes (Ws * 3 = 69)
    ("portrait.100x37", 4, (100, 37), 48, {}, "noise"),
    ("snap.34x60", 22, (34, 60), 32, {}, "noise"),                      # int(34 * 1) = 34 snaps to 32: one axis is the identity
    ("k17.120x200", 7, (120, 200), 16, {}, "noise"),                    # scale 7.5: ksize 17, the limit
    ("light.32x32", 9, (32, 32), 32, {"scales": LIGHT_SCALES}, "noise"),
    ("nofix.45x80", 10, (45, 80), 32, {"fix_crop": False}, "noise"),
    ("fewfix.45x80", 11, (45, 80), 32, {"more_fix_crop": False}, "noise"),
    ("nodistort.45x80", 12, (45, 80), 32, {"max_distort": 0}, "noise"),
    ("special.45x80", 13, (45, 80), 32, {}, "special"),                 # a constant channel; alternating 0 / 255 rows
)
CASE_IDS = [c[0] for c in CASES]


def frames(Hs, Ws, kind="noise"):
    """the input clips uint8 [B, T, Hs, Ws, 3]: a smooth gradient plus noise per frame and channel.  kind "special": frame (0, 0)
    has a constant green channel, frame (1, 0) alternating rows of 0 and 255, frame (2, 1) alternating columns"""
    rng = np.random.default_rng(18_000 + 131 * Hs + Ws)
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    out = np.zeros((B, T, Hs, Ws, 3), dtype=np.uint8)
    for b in range(B):
        for t in range(T):
            for c in range(3):
                ax, ay = rng.uniform(-1, 1, 2)
                g = ax * xx / Ws + ay * yy / Hs
                g = (g - g.min()) / max(g.max() - g.min(), 1e-9)
                v = -20 + g * 295 + rng.normal(0, 25, (Hs, Ws))
                out[b, t, :, :, c] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    if kind == "special":
        out[0, 0, :, :, 1] = 77
        out[1, 0, 0::2] = 0
        out[1, 0, 1::2] = 255
        out[2, 1, :, 0::2] = 255
        out[2, 1, :, 1::2] = 0
    return out


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def case_inputs():
    """every distinct input of the cases, in case order (what ``input.sha`` of the golden digests)"""
    seen, out = set(), []
    for _, _, size, _, _, kind in CASES:
        if (size, kind) not in seen:
            seen.add((size, kind))
            out.append(frames(*size, kind))
    return out


def inputs_digest():
    h = hashlib.sha256()
    for x in case_inputs():
        h.update(np.ascontiguousarray(x).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------- the plan
def fixed_offsets(more_fix_crop, image_w, image_h, crop_w, crop_h):
    ws, hs = (image_w - crop_w) // 4, (image_h - crop_h) // 4
    ret = [(0, 0), (4 * ws, 0), (0, 4 * hs), (4 * ws, 4 * hs), (2 * ws, 2 * hs)]
    if more_fix_crop:
        ret += [(0, 2 * hs), (4 * ws, 2 * hs), (2 * ws, 4 * hs), (2 * ws, 0), (ws, hs), (3 * ws, hs), (ws, 3 * hs), (3 * ws, 3 * hs)]
    return ret


def sample_crop(image_w, image_h, S_w, S_h, scales=DEFAULT_SCALES, max_distort=1, fix_crop=True, more_fix_crop=True):
    """(crop_w, crop_h, x0, y0) of one clip, consuming Python's global ``random`` as one call of the reference does"""
    base = min(image_w, image_h)
    sizes = [int(base * s) for s in scales]
    crop_h = [S_h if abs(v - S_h) < 3 else v for v in sizes]
    crop_w = [S_w if abs(v - S_w) < 3 else v for v in sizes]
    pairs = [(w, h) for i, h in enumerate(crop_h) for j, w in enumerate(crop_w) if abs(i - j) <= max_distort]
    w, h = random.choice(pairs)
    if not fix_crop:
        x0 = random.randint(0, image_w - w)
        y0 = random.randint(0, image_h - h)
    else:
        x0, y0 = random.choice(fixed_offsets(more_fix_crop, image_w, image_h, w, h))
    return w, h, x0, y0


# ---------------------------------------------------------------------------------------------------- Pillow's resample, 8 bits
def coefficients(in_size, out_size):
    """(ksize, bounds int [out, 2] = (xmin, count), kk int32 [out, ksize]) of Pillow's BILINEAR (triangle, support 1) from ``in_size``
    to ``out_size`` samples: precompute_coeffs in doubles, then normalize_coeffs_8bpc"""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), dtype=np.int64)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) * ss)
            v = 1.0 - a if a < 1.0 else 0.0
            w.append(v)
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = xmin, xmax
    return ksize, bounds, kk


def _pass(a, axis, out_size):
    """one pass along ``axis`` of the uint8 array a: ss = 1 << 21; ss += pixel * k; clip(ss >> 22, 0, 255)"""
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    _, bounds, kk = coefficients(a.shape[0], out_size)
    out = np.zeros((out_size,) + a.shape[1:], dtype=np.int64)
    for o in range(out_size):
        xmin, n = bounds[o]
        acc = np.full(a.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for j in range(n):
            acc += a[xmin + j] * int(kk[o, j])
        assert np.abs(acc).max() < 2 ** 31                       # Pillow's accumulator is an int
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def resize(frame, S_w, S_h):
    """PIL's Image.resize((S_w, S_h), BILINEAR) of a uint8 frame [h, w, 3]: horizontally to bytes, then vertically"""
    return _pass(_pass(frame, 1, S_w), 0, S_h)


def crop_resize(x, crops, S_w, S_h):
    """uint8 [B, T, S_h, S_w, 3]: clip b of x [B, T, Hs, Ws, 3] cut to crops[b] = (w, h, x0, y0) and resized"""
    out = np.zeros(x.shape[:2] + (S_h, S_w, 3), dtype=np.uint8)
    for b, (w, h, x0, y0) in enumerate(crops):
        for t in range(x.shape[1]):
            out[b, t] = resize(x[b, t, y0:y0 + h, x0:x0 + w], S_w, S_h)
    return out


def run_case(case):
    """(crops int [B, 4] = (w, h, x0, y0), the next random.random(), output frames) of a case, by the restatement"""
    _, seed, (Hs, Ws), S, kw, kind = case
    random.seed(seed)
    crops = [sample_crop(Ws, Hs, S, S, **kw) for _ in range(B)]
    nxt = random.random()
    return np.array(crops, dtype=np.int64), nxt, crop_resize(frames(Hs, Ws, kind), crops, S, S)


# ---------------------------------------------------------------------------------------------------- a malformed table
WILD_PLAN = ((45, 39, 8, 1), (39, 45, 20, 0), (39, 45, 20, 0))        # (w, h, x0, y0) of three clips of a 45 x 80 source towards 32 x 32


def wild_table(table, x, S=32):
    """(the table of WILD_PLAN made malformed, what the device must write for clip 2).  Row 1 names a sample outside the batch (ignored);
    row 2 states a crop and set indices far outside, and the horizontal set it is cut to states ksize and bounds far outside.  The
    clamps of the kernel define the result: the crop is the one pixel (y 0, x Ws - 1); set 99 -> 1 with ksize 17 and every bound cut to
    one tap at 0, its weight whatever word lies at kk[ox][0] under a stride of 17; set -3 -> 0 with its bounds cut to that one row."""
    bad = np.array(table, dtype=np.int32)
    Ws = x.shape[3]
    slot = 4 + S * 19
    hset1, vset0 = 3 * 8 + slot, 3 * 8 + 2 * slot
    bad[8 * 1 + 0] = 7
    bad[8 * 2 + 1:8 * 2 + 7] = 1 << 20, -5, 1 << 30, -(1 << 30), 99, -3
    bad[hset1 + 2] = 1 << 20
    bad[hset1 + 4:hset1 + 4 + 2 * S] = [1 << 28, 1 << 28] * S
    clip8 = lambda v: np.clip(v >> PRECISION_BITS, 0, 255)
    half = 1 << (PRECISION_BITS - 1)
    kh = bad[hset1 + 4 + 2 * S:][np.arange(S) * 17].astype(np.int64)
    vks = int(bad[vset0 + 2])
    vcount = np.clip(bad[vset0 + 4 + 1:vset0 + 4 + 2 * S:2], 0, min(vks, 1)).astype(np.int64)
    kv = bad[vset0 + 4 + 2 * S:][np.arange(S) * vks].astype(np.int64)
    pix = x[2, :, 0, Ws - 1, :].astype(np.int64)                                          # [T, 3]
    hbyte = clip8(half + pix[:, None, :] * kh[None, :, None])                             # [T, S, 3]
    want = clip8(half + hbyte[:, None, :, :] * (kv * vcount)[None, :, None, None])        # [T, S, S, 3]
    return bad, want.astype(np.uint8)
