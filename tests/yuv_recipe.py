"""The YUV-ingest contract restated in numpy / int64, independent of ``simple_tad_amd``: the integer 4:2:0 YUV -> RGB formula of
include/tad_mi355x_yuv.h (nearest chroma, 20-bit fixed point), the derivation of the colour sets from the luma weights, and packers
that lay Y, U, V planes out as NV12 / NV21 / I420 surfaces with arbitrary pitches and gaps between the planes.

The formula is the one OpenCV documents for its 8-bit COLOR_YUV2RGB_NV12 conversion; that is a citation, not an oracle: no OpenCV build
is consulted anywhere, the contract is the formula as the header writes it.
"""
import numpy as np

# the literal constants of the BT.601 limited-range conversion: {y_off, cy, cvr, cug, cvg, cub}
BT601 = (16, 1220542, 1673527, -409993, -852492, 2116026)
LUMA_WEIGHTS = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def derive(kr, kb, full_range):
    """{y_off, cy, cvr, cug, cvg, cub} from the luma weights by the usual matrix, in fp64, times 2^20, rounded to nearest.  With Y' the
    scaled luma and U', V' the scaled centred chroma: R = Y' + 2 (1 - kr) V', B = Y' + 2 (1 - kb) U', and G from kr R + kg G + kb B = Y'.
    Limited range: luma (Y - 16) * 255 / 219, chroma * 255 / 224; full range: luma and chroma as they are."""
    kr, kb = np.float64(kr), np.float64(kb)
    kg = np.float64(1) - kr - kb
    luma, chroma = (np.float64(1), np.float64(1)) if full_range else (np.float64(255) / 219, np.float64(255) / 224)
    r_v = 2 * (1 - kr)
    b_u = 2 * (1 - kb)
    g_u = -kb * b_u / kg
    g_v = -kr * r_v / kg
    q = lambda v: int(np.rint(v * (1 << 20)))
    return (0 if full_range else 16, q(luma), q(r_v * chroma), q(g_u * chroma), q(g_v * chroma), q(b_u * chroma))


def colour_sets():
    return {"bt601": BT601, "bt709": derive(*LUMA_WEIGHTS["bt709"], False), "bt601-full": derive(*LUMA_WEIGHTS["bt601"], True),
            "bt709-full": derive(*LUMA_WEIGHTS["bt709"], True)}


def bound(cset):
    """the largest magnitude a sum of the formula reaches under this set (it must stay below 2^31)"""
    _, cy, cvr, cug, cvg, cub = cset
    return 255 * cy + 128 * max(abs(cvr), abs(cub), abs(cug) + abs(cvg)) + (1 << 19)


def convert_samples(Y, U, V, cset):
    """uint8 [..., 3] (R, G, B) of int arrays Y, U, V of one shape: the formula, in int64 (python's >> on negative numbers floors)"""
    y_off, cy, cvr, cug, cvg, cub = (int(c) for c in cset)
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    yy = np.maximum(0, Y - y_off) * cy
    r = (yy + cvr * (V - 128) + (1 << 19)) >> 20
    g = (yy + cvg * (V - 128) + cug * (U - 128) + (1 << 19)) >> 20
    b = (yy + cub * (U - 128) + (1 << 19)) >> 20
    out = np.stack([r, g, b], axis=-1)
    assert np.abs(np.stack([yy + cvr * (V - 128), yy + cvg * (V - 128) + cug * (U - 128), yy + cub * (U - 128)])).max() + (1 << 19) < 2 ** 31
    return np.clip(out, 0, 255).astype(np.uint8)


def convert(Y, U, V, cset, bgr=False):
    """uint8 [h, w, 3] of the planes Y [h, w], U and V [(h + 1) // 2, (w + 1) // 2]: luma sample (y, x) takes the chroma pair
    (y >> 1, x >> 1)"""
    Y, U, V = np.asarray(Y), np.asarray(U), np.asarray(V)
    h, w = Y.shape
    assert U.shape == V.shape == ((h + 1) // 2, (w + 1) // 2) and Y.dtype == U.dtype == V.dtype == np.uint8
    yy, xx = np.meshgrid(np.arange(h) >> 1, np.arange(w) >> 1, indexing="ij")
    rgb = convert_samples(Y, U[yy, xx], V[yy, xx], cset)
    return np.ascontiguousarray(rgb[..., ::-1] if bgr else rgb)


def planes(h, w, seed):
    """random planes (Y, U, V) of an h x w frame"""
    rng = np.random.RandomState(104729 * seed + 131 * h + w)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return tuple(rng.randint(0, 256, s).astype(np.uint8) for s in ((h, w), (ch, cw), (ch, cw)))


def pack(Y, U, V, fmt, y_pitch=None, c_pitch=None, gap=0, gap2=0, fill=0, rng=None):
    """(bytes uint8 [n], layout): the surface of one frame.  Luma rows ``y_pitch`` apart, ``gap`` dead bytes, then the chroma rows
    ``c_pitch`` apart: "nv12" U V pairs, "nv21" V U pairs, "i420" the U plane, ``gap2`` dead bytes, the V plane.  Every byte that is no
    live sample is ``fill`` (or random, if ``rng`` is given); the buffer ends on the last live byte.  layout: dict(h, w, y_off, y_pitch,
    u_off, v_off, c_pitch, c_step, nbytes), offsets relative to the first byte."""
    h, w = Y.shape
    ch, cw = U.shape
    step = 1 if fmt == "i420" else 2
    y_pitch = w if y_pitch is None else y_pitch
    c_pitch = cw * step if c_pitch is None else c_pitch
    assert y_pitch >= w and c_pitch >= cw * step and fmt in ("nv12", "nv21", "i420")
    c_at = h * y_pitch + gap
    if fmt == "i420":
        u_off, v_off = c_at, c_at + ch * c_pitch + gap2
        n = v_off + (ch - 1) * c_pitch + cw
    else:
        u_off, v_off = (c_at, c_at + 1) if fmt == "nv12" else (c_at + 1, c_at)
        n = c_at + (ch - 1) * c_pitch + 2 * cw
    buf = rng.randint(0, 256, n).astype(np.uint8) if rng is not None else np.full(n, fill, dtype=np.uint8)
    for y in range(h):
        buf[y * y_pitch:y * y_pitch + w] = Y[y]
    for y in range(ch):
        buf[u_off + y * c_pitch:u_off + y * c_pitch + (cw - 1) * step + 1:step] = U[y]
        buf[v_off + y * c_pitch:v_off + y * c_pitch + (cw - 1) * step + 1:step] = V[y]
    return buf, dict(h=h, w=w, y_off=0, y_pitch=y_pitch, u_off=u_off, v_off=v_off, c_pitch=c_pitch, c_step=step, nbytes=n)


def unpack(buf, lay):
    """(Y, U, V) read back from a packed surface: the inverse of pack, for the packers' own test"""
    h, w, step = lay["h"], lay["w"], lay["c_step"]
    ch, cw = (h + 1) // 2, (w + 1) // 2
    Y = np.stack([buf[lay["y_off"] + y * lay["y_pitch"]:][:w] for y in range(h)])
    U = np.stack([buf[lay["u_off"] + y * lay["c_pitch"]:][:(cw - 1) * step + 1:step] for y in range(ch)])
    V = np.stack([buf[lay["v_off"] + y * lay["c_pitch"]:][:(cw - 1) * step + 1:step] for y in range(ch)])
    return Y, U, V
