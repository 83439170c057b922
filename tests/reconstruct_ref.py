"""The fp64 yardstick of MAE reconstruction (include/tad_mi355x_recon.h): ``oracle.vit_oracle.mae_target``'s arithmetic and its algebraic
inverse, restated on whole token grids, plus the small builders the reconstruction tests share (sources, masks, slot tables, the byte
rule).  No kernels, no GPU, no file is read.

Layout: a clip [B,3,T,H,W] is cut as the oracle cuts it, 'b c (t p0) (h p1) (w p2) -> b (t h w) (p0 p1 p2) c'; a prediction row is
'(p0 p1 p2) c' flattened, the layout of the labels."""
from types import SimpleNamespace

import torch

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def grid_of(tub, p, T, H, W):
    return T // tub, H // p, W // p


def patchify(v, tub, p):
    """[B,3,T,H,W] -> [B, N, tub*p*p, 3]"""
    B, C, T, H, W = v.shape
    tp, hp, wp = grid_of(tub, p, T, H, W)
    v = v.reshape(B, C, tp, tub, hp, p, wp, p).permute(0, 2, 4, 6, 3, 5, 7, 1)  # b t h w p0 p1 p2 c
    return v.reshape(B, tp * hp * wp, tub * p * p, C)


def tokens_to_frames(tokens, tub, p, T, H, W):
    """[B, N, tub*p*p, 3] -> frames [B,T,H,W,3]: the inverse of ``patchify``, channels last"""
    B = tokens.shape[0]
    tp, hp, wp = grid_of(tub, p, T, H, W)
    v = tokens.reshape(B, tp, hp, wp, tub, p, p, 3).permute(0, 1, 4, 2, 5, 3, 6, 7)  # b t p0 h p1 w p2 c
    return v.reshape(B, T, H, W, 3).contiguous()


def slot_of(mask):
    """bool [B,N] -> int32 [B,N]: the rank of a masked token among its clip's masked tokens in ascending order, -1 where visible"""
    m = mask.to(torch.int64)
    return torch.where(mask, m.cumsum(1) - 1, torch.full_like(m, -1)).to(torch.int32)


def to_byte(x):
    """clamp(rint(x), 0, 255) with halves to even; NaN -> 0, +inf -> 255, -inf -> 0"""
    return torch.nan_to_num(torch.round(x), nan=0.0, posinf=255.0, neginf=0.0).clamp(0, 255).to(torch.uint8)


def unnormalise(videos, mean=MEAN, std=STD):
    """videos * std + mean with the constants as float32 values (promoted when the clip is f64), as the oracle takes them"""
    m = torch.as_tensor(mean, device=videos.device)[None, :, None, None, None]
    s = torch.as_tensor(std, device=videos.device)[None, :, None, None, None]
    return videos * s + m


def unnormalise_fused_f32(videos, mean=MEAN, std=STD):
    """the f32 value fma(videos, std, mean) -- ONE rounding, which is how the kernels form it: the product of two f32 values is exact in
    f64, so the f64 sum carries one rounding to 53 bits before the one to 24 (they disagree with a true fma only where the f64 sum
    falls exactly on an f32 tie: not on these inputs' scale, and a test that used it there would fail loudly, not pass wrongly)"""
    assert videos.dtype == torch.float32
    m = torch.tensor(mean, dtype=torch.float32).double()[None, :, None, None, None]
    s = torch.tensor(std, dtype=torch.float32).double()[None, :, None, None, None]
    return (videos.double() * s + m).float()


def reconstruct_ref(videos, pred, slot, tub, p, mean=MEAN, std=STD, normalize_target=True, visible_gain=1.0):
    """The contract in the dtype of ``videos`` (float64 for the yardstick; float32 on any device for torch's own evaluation).
    videos [B,3,T,H,W]; pred [B,Nm,tub*p*p*3] or None; slot int [B,N] (outside [0, Nm) = visible).  Returns
      value   [B,T,H,W,3]: what is rounded to a byte -- 255 r at masked tokens, 255 visible_gain v at visible ones
      err     [B,N]: mean (pred - target)^2 at masked tokens, 0 at visible ones
      masked  bool [B,N];  scale / centre [B,N,1,3]: sqrt(var) + 1e-6 and the mean (1 and 0 without normalize_target);
      rows    [B,N,tub*p*p,3]: the prediction of every token (zeros where visible);  v: the un-normalised tokens"""
    B, _, T, H, W = videos.shape
    v = patchify(unnormalise(videos, mean, std), tub, p)
    N, npix = v.shape[1], v.shape[2]
    Nm = 0 if pred is None else pred.shape[1]
    slot = slot.to(videos.device).long()
    masked = (slot >= 0) & (slot < Nm)
    if Nm:
        P = pred.to(v.dtype).reshape(B, Nm, npix, 3)
        rows = P[torch.arange(B, device=videos.device)[:, None], slot.clamp(0, Nm - 1)]
        rows = torch.where(masked[:, :, None, None], rows, torch.zeros_like(rows))
    else:
        rows = torch.zeros_like(v)
    if normalize_target:
        centre = v.mean(dim=2, keepdim=True)
        scale = v.var(dim=2, unbiased=True, keepdim=True).sqrt() + 1e-6
        r, target = rows * scale + centre, (v - centre) / scale
    else:
        centre, scale = torch.zeros_like(v[:, :, :1]), torch.ones_like(v[:, :, :1])
        r, target = rows, v
    value = torch.where(masked[:, :, None, None], 255.0 * r, (255.0 * visible_gain) * v)
    err = torch.where(masked, ((rows - target) ** 2).mean(dim=(2, 3)), torch.zeros_like(v[:, :, 0, 0]))
    return SimpleNamespace(value=tokens_to_frames(value, tub, p, T, H, W), err=err, masked=masked, scale=scale, centre=centre, rows=rows, v=v)


# ----------------------------------------------------------------------------- sources and masks
def frames_to_clip_formula(u8, mean=MEAN, std=STD):
    """uint8 frames [B,T,H,W,3] -> the f32 clip [B,3,T,H,W] a loader hands over: (u / 255 - mean) / std, each operation rounded to f32"""
    m, s = torch.tensor(mean), torch.tensor(std)
    return ((u8.float() / 255.0 - m) / s).permute(0, 4, 1, 2, 3).contiguous()


def source(kind, B, tub, p, T, H, W, g):
    """uint8 frames [B,T,H,W,3]: "random" = any levels; "two_grey" = per (patch, channel) two ADJACENT levels k, k+1, both present;
    "constant" = every (patch, channel) one level of its own (levels 0 and 255 included)"""
    tp, hp, wp = grid_of(tub, p, T, H, W)
    N, npix = tp * hp * wp, tub * p * p
    if kind == "random":
        lv = torch.randint(0, 256, (B, N, npix, 3), generator=g)
    elif kind == "two_grey":
        k = torch.randint(0, 255, (B, N, 1, 3), generator=g)
        bit = torch.randint(0, 2, (B, N, npix, 3), generator=g)
        bit[:, :, 0], bit[:, :, -1] = 0, 1
        lv = k + bit
    elif kind == "constant":
        lv = torch.randint(0, 256, (B, N, 1, 3), generator=g).repeat(1, 1, npix, 1)
        lv[0, 0], lv[-1, -1] = 0, 255
    else:
        raise ValueError(kind)
    return tokens_to_frames(lv.to(torch.uint8), tub, p, T, H, W)


def random_masks(B, N, n_mask, g):
    """bool [B,N], n_mask True per clip, another pattern in each clip wherever more than one pattern exists"""
    mask = torch.zeros(B, N, dtype=torch.bool)
    for b in range(B):
        for _ in range(64):
            row = torch.zeros(N, dtype=torch.bool)
            row[torch.randperm(N, generator=g)[:n_mask]] = True
            if not any(torch.equal(row, mask[a]) for a in range(b)) or n_mask in (0, N):
                break
        mask[b] = row
    return mask
