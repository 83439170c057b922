"""RandAugment fixture G16 (tests/golden/g16_rand_augment.npz, written by tools/make_goldens_randaug.py from the reference's own
``rand_augment.AugmentOp`` / ``rand_augment_transform`` and PIL): its seeded input frames, its cases, and a numpy restatement of every
operator in the arithmetic PIL uses -- integers, C ``float`` for the ImageEnhance blend and the SMOOTH filter, C ``double`` for the
affine resampling.  The restatement is the bridge between PIL's results (the goldens; tests/test_randaug_cpu.py holds it to them bit
for bit) and the kernels of csrc/randaug.hip, which state the same arithmetic.  Test infrastructure only.

Frames are uint8 [H, W, 3] (RGB).  ``apply(frame, name, arg, resample, fill)`` carries out one operator on one frame: ``name`` one of
the reference's op names, ``arg`` the value its level function returned (None for the ops without one), ``resample`` BILINEAR or
BICUBIC for the geometric ops.

Fixture G25 (tests/golden/g25_rand_augment_shapes.npz, tools/make_goldens_randaug_shapes.py) holds PIL's results for the same per-op
cases at the shapes ``SHAPES`` on the frames of ``frames_at`` (any shape), as SHA-256 per output frame: tests/test_randaug_shapes_cpu.py
holds the restatement to them, tests/test_randaug_shapes_gpu.py the kernels to the restatement."""
import hashlib
import math

import numpy as np

BILINEAR, BICUBIC = 2, 3          # PIL's Image.Resampling values
B, T, H, W = 3, 2, 20, 23         # the one shape of the fixture
FILL = (128, 128, 128)
POLICY = "rand-m6-n3-mstd0.5-inc1"
NEGATING = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel", "ColorIncreasing", "ContrastIncreasing",
            "BrightnessIncreasing", "SharpnessIncreasing")
GEOMETRIC = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
PLAIN = ("AutoContrast", "Equalize", "Invert", "Posterize", "PosterizeIncreasing", "Solarize", "SolarizeIncreasing", "SolarizeAdd",
         "Color", "Contrast", "Brightness", "Sharpness")
ALL_NAMES = PLAIN + NEGATING
# ops whose device result must equal PIL's bit for bit.  The issue requires it of the integer / lookup-table / ImageEnhance ops and
# allows Sharpness and the geometric ops one unit in at most 0.1 % of a case's bytes; the MI355X reproduces those bit for bit as well
# (f32 / f64 without contraction), so they are held to it too
EXACT = ALL_NAMES
# policy cases: (key, seed, op list: "drive" | "default", interpolation: BICUBIC | None = random per frame)
POLICIES = (("policy.drive.1", 1, "drive", BICUBIC), ("policy.drive.2", 2, "drive", BICUBIC), ("policy.drive.3", 3, "drive", BICUBIC),
            ("policy.drive.7", 7, "drive", BICUBIC), ("policy.default.9", 9, "default", BICUBIC),
            ("policy.random.3", 3, "drive", None))


def op_cases():
    """(key, name, magnitude, seed of ``random`` (picks the sign), resample) of every per-op golden case: every name, both signs of
    the negating ops, both resampling filters of the geometric ones, enhance factors below and above 1"""
    out = []
    for name in PLAIN:
        mags = (2, 9) if name in ("Color", "Contrast", "Brightness", "Sharpness") else (3, 7) if name not in (
            "AutoContrast", "Equalize", "Invert") else (5,)
        for m in mags:
            out.append((f"op.{name}.m{m}", name, m, 0, BILINEAR))
    for name in NEGATING:
        for sign, seed in (("neg", SIGN_SEEDS[0]), ("pos", SIGN_SEEDS[1])):
            for rs in ((BILINEAR, BICUBIC) if name in GEOMETRIC else (BILINEAR,)):
                tag = f".{'bilinear' if rs == BILINEAR else 'bicubic'}" if name in GEOMETRIC else ""
                out.append((f"op.{name}.m6.{sign}{tag}", name, 6, seed, rs))
    return out


# random.seed(s): the first random.random() is > 0.5 for s = 0 (the level is negated) and <= 0.5 for s = 1 (kept); the tool asserts it
SIGN_SEEDS = (0, 1)


def frames():
    """the input clips uint8 [B, T, H, W, 3]: a smooth gradient plus noise per frame, cut to a per-frame, per-channel range.  Frame
    (0, 0): channels on different sub-ranges; (0, 1): 0..255; (1, 0): a constant channel; the rest: other sub-ranges"""
    rng = np.random.default_rng(16)
    ranges = {(0, 0): ((37, 201), (12, 130), (90, 255)), (0, 1): ((0, 255),) * 3, (1, 0): ((20, 230), (77, 77), (0, 180)),
              (1, 1): ((5, 250), (60, 190), (30, 99)), (2, 0): ((0, 128), (100, 255), (64, 192)), (2, 1): ((10, 245), (0, 255), (128, 255))}
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((B, T, H, W, 3), dtype=np.uint8)
    for (b, t), rr in ranges.items():
        for c, (lo, hi) in enumerate(rr):
            ax, ay = rng.uniform(-1, 1, 2)
            g = ax * (xx - W / 2) / W + ay * (yy - H / 2) / H
            g = (g - g.min()) / max(g.max() - g.min(), 1e-9)
            v = lo - 20 + g * (hi - lo + 40) + rng.normal(0, 12, (H, W))
            v = np.clip(np.rint(v), lo, hi)
            if hi > lo:      # both ends of the range occur
                v.flat[rng.integers(0, H * W)] = lo
                v.flat[(np.argmin(v) + 1 + rng.integers(0, H * W - 1)) % (H * W)] = hi
            out[b, t, :, :, c] = v.astype(np.uint8)
    return out


# fixture G25 (tests/golden/g25_rand_augment_shapes.npz, tools/make_goldens_randaug_shapes.py): the per-op cases at other shapes
# (B, T, H, W): frames below 3 pixels in a direction, one row, one column, a short pointwise item, a real frame, two non-square mid sizes
SHAPES = ((2, 3, 1, 1), (2, 3, 1, 7), (2, 3, 7, 1), (2, 3, 2, 2), (2, 3, 3, 3), (2, 3, 2, 9), (2, 3, 3, 40), (1, 2, 224, 224),
          (2, 2, 45, 80), (2, 2, 67, 63), (1, 4, 9, 11))
SHAPES_SEED = 26          # (a seed at which the 224 x 224 frames show both ends of the Equalize cut: tests/test_randaug_shapes_cpu.py)
KINDS = ("gradient", "full", "constant", "two-level")


def shape_key(shape):
    return "x".join(str(int(v)) for v in shape)


def case_arg(value, name):
    """a stored argument (float64, NaN = the op has none) as ``apply`` takes it"""
    value = float(value)
    return None if np.isnan(value) else (int(value) if name.startswith(("Posterize", "Solarize")) else value)


def golden_args(g, shape):
    """{case key: argument} of one shape of fixture G25"""
    cases = op_cases()
    assert [c[0] for c in cases] == list(g["cases"])
    return {c[0]: case_arg(a, c[1]) for c, a in zip(cases, g[f"{shape_key(shape)}.args"])}


def kind_of(b, t, T):
    """the kind of frame (b, t) of ``frames_at``: frames run through the four kinds in memory order"""
    return KINDS[(b * T + t) % 4]


def frames_at(B, T, H, W, seed):
    """seeded input clips uint8 [B, T, H, W, 3] at any shape.  The kind of a frame is fixed by (b, t) (``kind_of``):
      gradient   a smooth gradient plus noise per channel, cut to a drawn sub-range (as ``frames()``)
      full       the same on 0..255 in every channel
      constant   channel 1 holds one value, the others are gradients
      two-level  channel 2 holds two values, the upper one in more than H * W - 255 pixels (two occupied bins; Equalize's step is 0
                 once H * W >= 256), the others are gradients
    Where a frame has two pixels or more, both ends of a gradient channel's range occur."""
    rng = np.random.default_rng([seed, B, T, H, W])
    n = H * W
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((B, T, H, W, 3), dtype=np.uint8)
    for b in range(B):
        for t in range(T):
            kind = kind_of(b, t, T)
            for c in range(3):
                lo = int(rng.integers(0, 120))
                hi = int(rng.integers(lo + 40, 256))
                ax, ay = rng.uniform(-1, 1, 2)
                noise = rng.normal(0, 12, (H, W))
                spot = rng.integers(0, n, 2)
                few = int(rng.integers(1, 255))
                if kind == "full":
                    lo, hi = 0, 255
                if kind == "constant" and c == 1:
                    out[b, t, :, :, c] = lo
                    continue
                if kind == "two-level" and c == 2:
                    v = np.full(n, hi, dtype=np.uint8)
                    v[rng.permutation(n)[:min(few, n // 2)]] = lo
                    out[b, t, :, :, c] = v.reshape(H, W)
                    continue
                g = ax * (xx - W / 2) / W + ay * (yy - H / 2) / H
                g = (g - g.min()) / max(g.max() - g.min(), 1e-9)
                v = np.clip(np.rint(lo - 20 + g * (hi - lo + 40) + noise), lo, hi)
                if n >= 2:
                    v.flat[spot[0]] = lo
                    v.flat[(spot[0] + 1 + spot[1] % (n - 1)) % n] = hi
                out[b, t, :, :, c] = v.astype(np.uint8)
    return out


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


# ------------------------------------------------------------------ lookup-table ops
def _lut(f, lut3):
    lut3 = np.asarray(lut3).reshape(3, 256)
    return np.stack([np.clip(lut3[c], 0, 255).astype(np.uint8)[f[..., c]] for c in range(3)], -1)


def _histograms(f):
    return [np.bincount(f[..., c].ravel(), minlength=256) for c in range(3)]


def autocontrast_lut(h):
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return list(range(256))
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return [min(255, max(0, int(ix * scale + offset))) for ix in range(256)]


def equalize_lut(h):
    nz = [int(v) for v in h if v]
    if len(nz) <= 1:
        return list(range(256))
    step = (sum(nz) - nz[-1]) // 255
    if not step:
        return list(range(256))
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(255, n // step))
        n += int(h[i])
    return lut


def to_l(f):
    p = f.astype(np.int64)
    return ((p[..., 0] * 19595 + p[..., 1] * 38470 + p[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def l_mean(f):
    """ImageEnhance.Contrast: int(mean of the L image + 0.5)"""
    return int(int(to_l(f).astype(np.int64).sum()) / (f.shape[0] * f.shape[1]) + 0.5)


# ------------------------------------------------------------------ ImageEnhance
def blend(deg, img, factor):
    """Image.blend(degenerate, image, factor): C float arithmetic, truncating store; clipped outside [0, 1]"""
    a = np.float32(factor)
    d = deg.astype(np.float32)
    temp = d + a * (img.astype(np.int32) - deg.astype(np.int32)).astype(np.float32)
    assert temp.dtype == np.float32
    if 0.0 <= factor <= 1.0:
        return temp.astype(np.int32).astype(np.uint8)
    return np.where(temp <= 0, 0, np.where(temp >= 255, 255, temp.astype(np.int32))).astype(np.uint8)


def smooth(f):
    """ImageFilter.SMOOTH: 3 x 3 kernel (1 1 1 / 1 5 1 / 1 1 1) / 13 in C float, rows from below upwards, + 0.5 and truncation; the
    outermost rows and columns are copied"""
    k = (np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], dtype=np.float32) / np.float32(13)).astype(np.float32)
    out = f.copy()
    p = f.astype(np.float32)
    h, w = f.shape[:2]
    if h < 3 or w < 3:
        return out
    ss = np.full((h - 2, w - 2, 3), np.float32(0.5), dtype=np.float32)
    for j, dy in enumerate((1, 0, -1)):
        rows = p[1 + dy:h - 1 + dy]
        ss = ss + ((rows[:, 0:w - 2] * k[3 * j] + rows[:, 1:w - 1] * k[3 * j + 1]) + rows[:, 2:w] * k[3 * j + 2])
    assert ss.dtype == np.float32
    out[1:h - 1, 1:w - 1] = np.where(ss <= 0, 0, np.where(ss >= 255, 255, ss.astype(np.int32))).astype(np.uint8)
    return out


# ------------------------------------------------------------------ affine resampling
def rotate_matrix(degrees, w, h):
    """Image.rotate's matrix about the centre (None: PIL returns a copy)"""
    angle = degrees % 360.0
    if angle == 0:
        return None
    cx, cy = w / 2.0, h / 2.0
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def matrix_of(name, arg, w, h):
    if name == "Rotate":
        return rotate_matrix(arg, w, h)
    return {"ShearX": [1, arg, 0, 0, 1, 0], "ShearY": [1, 0, 0, arg, 1, 0], "TranslateXRel": [1, 0, arg * w, 0, 1, 0],
            "TranslateYRel": [1, 0, 0, 0, 1, arg * h]}[name]


def _floor(v):
    return np.floor(v).astype(np.int64)


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def affine(f, m, resample, fill=FILL):
    h, w = f.shape[:2]
    a0, a1, a2, a3, a4, a5 = (float(v) for v in m)
    yo, xo = np.mgrid[0:h, 0:w]
    xs, ys = xo + 0.5, yo + 0.5
    xin = a0 * xs + a1 * ys + a2
    yin = a3 * xs + a4 * ys + a5
    inside = ~((xin < 0.0) | (xin >= w) | (yin < 0.0) | (yin >= h))
    xin, yin = xin - 0.5, yin - 0.5
    x, y = _floor(xin), _floor(yin)
    dx, dy = (xin - x)[..., None], (yin - y)[..., None]
    p = f.astype(np.float64)
    cx = lambda v: np.clip(v, 0, w - 1)
    cy = lambda v: np.clip(v, 0, h - 1)
    if resample == BILINEAR:
        def row(yy):
            a, b = p[yy, cx(x)], p[yy, cx(x + 1)]
            return a + (b - a) * dx
        v1 = row(cy(y))
        ok = ((y + 1 >= 0) & (y + 1 < h))[..., None]
        v2 = np.where(ok, row(cy(y + 1)), v1)
        v = v1 + (v2 - v1) * dy
        res = v.astype(np.int64)           # (bilinear: a convex combination, stored by truncation)
    else:
        x, y = x - 1, y - 1
        def row(yy):
            return _cubic(p[yy, cx(x)], p[yy, cx(x + 1)], p[yy, cx(x + 2)], p[yy, cx(x + 3)], dx)
        v1 = row(cy(y))
        v2 = np.where(((y + 1 >= 0) & (y + 1 < h))[..., None], row(cy(y + 1)), v1)
        v3 = np.where(((y + 2 >= 0) & (y + 2 < h))[..., None], row(cy(y + 2)), v2)
        v4 = np.where(((y + 3 >= 0) & (y + 3 < h))[..., None], row(cy(y + 3)), v3)
        v = _cubic(v1, v2, v3, v4, dy)
        res = np.where(v <= 0.0, 0, np.where(v >= 255.0, 255, v.astype(np.int64)))
    return np.where(inside[..., None], res, np.asarray(fill, dtype=np.int64)).astype(np.uint8)


# ------------------------------------------------------------------ one operator on one frame
def apply(f, name, arg=None, resample=BILINEAR, fill=FILL):
    base = name.replace("Increasing", "")
    if base == "AutoContrast":
        return _lut(f, [autocontrast_lut(h) for h in _histograms(f)])
    if base == "Equalize":
        return _lut(f, [equalize_lut(h) for h in _histograms(f)])
    if base == "Invert":
        return _lut(f, [[255 - i for i in range(256)]] * 3)
    if base == "Posterize":
        if arg >= 8:
            return f.copy()
        mask = ~(2 ** (8 - arg) - 1)
        return _lut(f, [[i & mask for i in range(256)]] * 3)
    if base == "Solarize":
        return _lut(f, [[i if i < arg else 255 - i for i in range(256)]] * 3)
    if base == "SolarizeAdd":
        return _lut(f, [[min(255, i + arg) if i < 128 else i for i in range(256)]] * 3)
    if base == "Brightness":
        return blend(np.zeros_like(f), f, arg)
    if base == "Contrast":
        return blend(np.full_like(f, l_mean(f)), f, arg)
    if base == "Color":
        return blend(np.repeat(to_l(f)[..., None], 3, -1), f, arg)
    if base == "Sharpness":
        return blend(smooth(f), f, arg)
    if name in GEOMETRIC:
        m = matrix_of(name, arg, f.shape[1], f.shape[0])
        return f.copy() if m is None else affine(f, m, resample, fill)
    raise KeyError(name)


def apply_rows(x, rows, names, fill=FILL):
    """a whole plan on a batch [B, T, H, W, 3]: rows = (clip, op index, applied, arg, per-frame resample) in plan order"""
    out = x.copy()
    for b, op, applied, arg, resample in rows:
        if not applied:
            continue
        for t in range(x.shape[1]):
            out[b, t] = apply(out[b, t], names[op], arg, resample[t] if resample else BILINEAR, fill)
    return out
