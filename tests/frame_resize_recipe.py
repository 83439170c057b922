"""The frame-resize contract restated in numpy, independent of ``simple_tad_amd``: OpenCV's generic integer formulation of the 8-bit
``INTER_CUBIC`` resize and the five pad modes of ``video_transforms.pad_wide_clips`` (include/tad_mi355x.h states both).  The pad is
MATERIALISED here (``pad_frames``) and resized like any other frame; the kernel never builds it.

This is not the bytes of one OpenCV build: a build's vector path finishes the vertical pass in float, its scalar path in integers,
and the two can differ by one grey level.  ``float64_bicubic`` is the independent yardstick (torch's bicubic: the same kernel, A =
-0.75, half-pixel centres, clamped border; no code shared with ``resize``).
"""
import numpy as np

F32 = np.float32
# (source H, W) -> (S_h, S_w): the smallest extents at which each branch of the kernel can go wrong
SHAPES = [((45, 80), (28, 28)),      # plain downscale
          ((72, 128), (32, 32)),     # exact 4x horizontal ratio: every output has the same coefficients
          ((9, 13), (32, 32)),       # upscale: taps of neighbouring outputs coincide, both borders clamp
          ((5, 7), (16, 16)),        # upscale
          ((32, 32), (32, 32)),      # identity: output == input
          ((2, 2), (8, 8)),          # tiny source
          ((1, 5), (4, 4)),          # one source row: all four vertical taps clamp to it
          ((3, 200), (16, 16)),      # taps 12.5 columns apart
          ((37, 53), (20, 24)),      # non-square
          ((70, 90), (33, 35))]      # one output past a tile edge on both axes
# beyond the list every resize must pass: a vertical shrink above 4, where a tile's taps no longer span 4 rows per output row
EXTRA_SHAPES = [((150, 12), (33, 8))]
MODES = ("black", "color", "reflect", "replicate")


def axis(n_src, n_dst):
    """(taps int64 [n_dst, 4] already clamped, k int64 [n_dst, 4]) of one axis, one output at a time"""
    taps = np.zeros((n_dst, 4), dtype=np.int64)
    k = np.zeros((n_dst, 4), dtype=np.int64)
    scale = float(n_src) / float(n_dst)
    A = F32(-0.75)
    for d in range(n_dst):
        f = F32((d + 0.5) * scale - 0.5)          # the double expression, rounded once
        s = int(np.floor(f))
        x = F32(f - F32(s))
        x1 = F32(x + F32(1))
        xr = F32(F32(1) - x)
        c0 = F32(F32(F32(F32(F32(F32(A * x1) - F32(F32(5) * A)) * x1) + F32(F32(8) * A)) * x1) - F32(F32(4) * A))
        c1 = F32(F32(F32(F32(F32(F32(A + F32(2)) * x) - F32(A + F32(3))) * x) * x) + F32(1))
        c2 = F32(F32(F32(F32(F32(F32(A + F32(2)) * xr) - F32(A + F32(3))) * xr) * xr) + F32(1))
        c3 = F32(F32(F32(F32(1) - c0) - c1) - c2)
        for j, c in enumerate((c0, c1, c2, c3)):
            k[d, j] = min(max(int(np.rint(F32(c * F32(2048)))), -32768), 32767)
            taps[d, j] = min(max(s - 1 + j, 0), n_src - 1)
    return taps, k


def resize_unclipped(frames, S_h, S_w):
    """int64 [..., S_h, S_w, 3]: the vertical sums after the rounding shift, BEFORE the clip to [0, 255]"""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.shape[-1] == 3
    H, W = frames.shape[-3], frames.shape[-2]
    tx, kx = axis(W, S_w)
    ty, ky = axis(H, S_h)
    src = frames.astype(np.int64)
    h = (src[..., :, tx, :] * kx[:, :, None]).sum(axis=-2)                     # [..., H, S_w, 3]
    v = (h[..., ty, :, :] * ky[:, :, None, None]).sum(axis=-3)                 # [..., S_h, S_w, 3]
    assert np.abs(v).max() + (1 << 21) < 2 ** 31
    return (v + (1 << 21)) >> 22


def resize(frames, S_h, S_w):
    """uint8 [..., S_h, S_w, 3] of uint8 frames [..., H, W, 3]"""
    return np.ascontiguousarray(np.clip(resize_unclipped(frames, S_h, S_w), 0, 255).astype(np.uint8))


def pad_frames(frames, mode, pad_top, pad_bottom, alpha=0.0, colour=(0, 0, 0)):
    """the padded frames [..., pad_top + H + pad_bottom, W, 3] the reference hands to cv2.resize; ``mode`` None returns the frames"""
    frames = np.asarray(frames)
    if mode is None:
        return frames
    H = frames.shape[-3]
    assert mode in MODES and 0 <= pad_top <= H and 0 <= pad_bottom <= H
    if mode in ("black", "color"):
        fill = np.asarray(colour if mode == "color" else (0, 0, 0), dtype=np.uint8)
        top = np.broadcast_to(fill, frames.shape[:-3] + (pad_top,) + frames.shape[-2:])
        bottom = np.broadcast_to(fill, frames.shape[:-3] + (pad_bottom,) + frames.shape[-2:])
    elif mode == "replicate":
        top = np.repeat(frames[..., :1, :, :], pad_top, axis=-3)
        bottom = np.repeat(frames[..., H - 1:, :, :], pad_bottom, axis=-3)
    else:  # BORDER_REFLECT (the edge row doubled), then addWeighted(reflect, a, black, 1 - a, 0): float product, rint, ties to even
        fade = lambda band: np.rint(band.astype(F32) * F32(alpha)).astype(np.uint8)
        top = fade(frames[..., :pad_top, :, :][..., ::-1, :, :])
        bottom = fade(frames[..., H - pad_bottom:, :, :][..., ::-1, :, :])
    return np.concatenate([top, frames, bottom], axis=-3)


def pad_resize(frames, pad, S):
    """one clip [T,H,W,3] padded as ``pad`` = (mode, pad_top, pad_bottom, alpha, colour) and resized to S x S"""
    return resize(pad_frames(frames, *pad), S, S)


def float64_bicubic(frames, S_h, S_w):
    """float64 [N, S_h, S_w, 3], unclipped: torch.nn.functional.interpolate(mode="bicubic", align_corners=False) on the double frames"""
    import torch
    x = torch.from_numpy(np.asarray(frames)).double().permute(0, 3, 1, 2)
    y = torch.nn.functional.interpolate(x, size=(S_h, S_w), mode="bicubic", align_corners=False)
    return y.permute(0, 2, 3, 1).numpy()


def images(H, W, seed=0):
    """uint8 [3, H, W, 3]: noise, a smooth image, a 0 / 255 step image"""
    rng = np.random.RandomState(1000 + seed + 7 * H + W)
    noise = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    smooth = np.stack([127.5 + 127.5 * np.sin(0.31 * xx + 0.17 * yy + c) for c in range(3)], axis=-1)
    step = np.where(((xx // 3 + yy // 2) % 2)[..., None] == 0, 0, 255) * np.ones(3)
    return np.stack([noise, np.rint(smooth).astype(np.uint8), step.astype(np.uint8)])
