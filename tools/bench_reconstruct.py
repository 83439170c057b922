#!/usr/bin/env python3
"""MAE reconstruction (``tadr_mae_reconstruct``: frames and error map in one launch) against the torch composition of the same
arithmetic on the same device, at

  16 clips of 16 x 224 x 224, patch 16, tubelet 2, tube mask 0.9 and 0.75   (the VideoMAE pre-training shape)
  16 clips of  8 x 224 x 224, patch 14, tubelet 1, tube mask 0.75           (the InternVideo2 pre-training shape)

The torch route is what ``reconstruct`` would be without the kernel: un-normalise, 'b c (t p0) (h p1) (w p2) -> b (t h w) (p0 p1 p2) c',
mean / unbiased variance per (patch, channel), the boolean scatter of the prediction into the token grid, un-standardise, select, times
255, round, clamp, cast, the rearrange back to [B,T,H,W,3], and the per-token mean squared error.  Both routes run interleaved in one
process, round by round; times are device events around ``--calls`` back-to-back calls; reported are the median over ``--rounds`` and
the spread (max - min).  GB/s are over the kernel's algorithmic bytes: the clip read once, the prediction read once, the frames and the
error map written once.  Before anything is timed the two routes are compared: bytes differ by at most 1 (torch's one-float mean and
its own rounding order) and the error maps agree to 1e-4 relative.

usage: python tools/bench_reconstruct.py [--batch 16] [--rounds 7] [--calls 300] [--out profiles/reconstruct.json]
Prints one JSON line and writes it to ``--out``.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SHAPES = (("videomae_16x224_p16_t2_m0.90", 16, 224, 16, 2, 0.90), ("videomae_16x224_p16_t2_m0.75", 16, 224, 16, 2, 0.75),
          ("internvideo2_8x224_p14_t1_m0.75", 8, 224, 14, 1, 0.75))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=300, help="device calls per round and route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reconstruct.json"))
    a = ap.parse_args()
    B = a.batch

    import torch
    from simple_tad_amd import kernels as K
    from simple_tad_amd.modeling_pretrain import slot_table
    if not torch.cuda.is_available():
        raise SystemExit("bench_reconstruct: no GPU (a measurement does not fall back)")
    res = {"bench": "reconstruct", "batch": B, "calls": a.calls, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "shapes": {}}
    mean_t = torch.tensor(MEAN, device="cuda")[None, :, None, None, None]
    std_t = torch.tensor(STD, device="cuda")[None, :, None, None, None]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls

    for name, T, S, p, tub, ratio in SHAPES:
        g = torch.Generator().manual_seed(0)
        tp, hp = T // tub, S // p
        N, npix = tp * hp * hp, tub * p * p
        per_frame = int(ratio * hp * hp)
        mask = torch.zeros(B, tp, hp * hp, dtype=torch.bool)
        for b in range(B):   # tube masks: one spatial pattern per clip
            mask[b, :, torch.randperm(hp * hp, generator=g)[:per_frame]] = True
        mask = mask.reshape(B, N).cuda()
        Nm = per_frame * tp
        u8 = torch.randint(0, 256, (B, T, S, S, 3), generator=g, dtype=torch.uint8).cuda()
        videos = ((u8.float() / 255.0 - torch.tensor(MEAN, device="cuda")) / torch.tensor(STD, device="cuda")).permute(0, 4, 1, 2, 3).contiguous()
        pred = torch.randn(B, Nm, npix * 3, generator=g).cuda()
        slot, _ = slot_table(mask, Nm)

        def kernel_route():
            return K.mae_reconstruct(videos, pred, slot, tub, p, MEAN, STD, True)

        def torch_route():
            v = videos * std_t + mean_t
            v = v.reshape(B, 3, tp, tub, hp, p, hp, p).permute(0, 2, 4, 6, 3, 5, 7, 1).reshape(B, N, npix, 3)
            centre = v.mean(dim=2, keepdim=True)
            scale = v.var(dim=2, unbiased=True, keepdim=True).sqrt() + 1e-6
            rows = torch.zeros_like(v)
            rows[mask] = pred.reshape(B * Nm, npix, 3)
            out = torch.where(mask[:, :, None, None], rows * scale + centre, v)
            frames = (out * 255.0).round().clamp(0, 255).to(torch.uint8)
            frames = frames.reshape(B, tp, hp, hp, tub, p, p, 3).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(B, T, S, S, 3).contiguous()
            err = torch.where(mask, ((rows - (v - centre) / scale) ** 2).mean(dim=(2, 3)), torch.zeros((), device="cuda"))
            return frames, err

        fk, ek = kernel_route()
        ft, et = torch_route()
        diff = (fk.to(torch.int16) - ft.to(torch.int16)).abs()
        assert int(diff.max()) <= 1, int(diff.max())
        assert torch.allclose(ek, et, rtol=1e-4, atol=1e-7), float((ek - et).abs().max())
        agree = {"bytes_differing_by_1": int((diff != 0).sum()), "bytes": diff.numel(), "err_max_rel_diff": float(((ek - et).abs() / et.clamp_min(1e-30))[mask].max())}
        del fk, ek, ft, et, diff
        routes = {"kernel": kernel_route, "torch": torch_route}
        for fn in routes.values():   # warm-up of every route at the timed shape
            for _ in range(3):
                fn()
        ms = {k: [] for k in routes}
        for _ in range(a.rounds):
            for k, fn in routes.items():
                ms[k].append(timed(fn))
        nbytes = videos.numel() * 4 + pred.numel() * 4 + slot.numel() * 4 + u8.numel() + B * N * 4
        med = {k: float(np.median(v)) for k, v in ms.items()}
        res["shapes"][name] = {
            "clip": [T, S, S], "patch": p, "tubelet": tub, "mask_ratio": ratio, "tokens": N, "masked": Nm, "algorithmic_mb": round(nbytes / 1e6, 1),
            "agreement": agree,
            **{k: {"ms": round(med[k], 4), "spread_ms": round(max(v) - min(v), 4), "rounds_ms": [round(t, 4) for t in v]} for k, v in ms.items()},
            "kernel_gb_per_s": round(nbytes / (med["kernel"] * 1e-3) / 1e9, 1),
            "torch_over_kernel": round(med["torch"] / med["kernel"], 2),
        }
        del u8, videos, pred, slot, mask
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
