#!/usr/bin/env python3
"""The loader's cubic resize on the device at the workload's shapes: camera frames of 1280 x 720 to 224 x 224,
  batch    32 clips x 16 frames in one launch          (a fine-tune batch, a chunk of a test video)
  single   one frame                                   (live inference: SlidingWindow.push_raw)
Per shape, measured with device events around ``--calls`` back-to-back calls, ``--rounds`` rounds, the two routes alternating inside
every round of one process:
  kernel   ``frame_resize.resize_frames`` (tad_frame_resize, uint8 in, uint8 out): frames/s of the launch, and the launch against its
           ALGORITHMIC bytes -- the source bytes under taps (distinct rows under vertical taps x distinct columns under horizontal
           taps x 3) plus the output bytes -- as GB/s and as a share of the 8.0 TB/s HBM peak
  torch    torch's own route on the same GPU: ``interpolate(mode="bicubic")`` on the float frames [N,3,H,W], then round, clamp and
           the cast to uint8 (``torch_from_u8`` also counts the uint8 -> float conversion and the permute in front of it)
and the largest difference between the two results in grey levels (the contract allows 1 against a float bicubic).

usage: python tools/bench_frame_resize.py [--batch 32] [--frames 16] [--rounds 5] [--calls 10]
Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W, S = 720, 1280, 224
HBM_PEAK = 8.0e12


def make_frames(n):
    """seeded uint8 [n,H,W,3]: a diagonal gradient plus noise, shifted from frame to frame"""
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.clip(((xx + yy) * 255.0 / (H + W - 2))[:, :, None] + rng.normal(0, 25, (H, W, 3)), 0, 255).astype(np.uint8)
    return np.stack([np.roll(base, 7 * i, axis=1) for i in range(min(n, 16))])


def algorithmic_bytes(n):
    from simple_tad_amd.frame_resize import cubic_coeffs
    under = []
    for n_src in (H, W):
        first, _ = cubic_coeffs(n_src, S)
        under.append(len(np.unique(np.clip(first[:, None] + np.arange(4), 0, n_src - 1))))
    return n * (under[0] * under[1] * 3 + S * S * 3), under


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="calls per round and route")
    a = ap.parse_args()
    import torch
    from simple_tad_amd.frame_resize import resize_frames
    if not torch.cuda.is_available():
        raise SystemExit("bench_frame_resize: no GPU (a measurement does not fall back)")
    ev = lambda: torch.cuda.Event(enable_timing=True)
    med = lambda v: float(np.median(v))
    res = {"bench": "frame_resize", "source": [H, W], "output": S, "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "calls": a.calls}
    some = torch.from_numpy(make_frames(16)).cuda()

    def timed(fn, calls):
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls

    for name, (B, T) in (("batch", (a.batch, a.frames)), ("single", (1, 1))):
        n = B * T
        x = some[torch.arange(n, device="cuda") % some.shape[0]].reshape(B, T, H, W, 3).contiguous()
        xf = x.reshape(n, H, W, 3).permute(0, 3, 1, 2).float().contiguous()           # the float frames torch's route starts from
        out = torch.empty((B, T, S, S, 3), dtype=torch.uint8, device="cuda")
        calls = a.calls if n > 1 else 20 * a.calls

        def kernel():
            return resize_frames(x, S, out=out)

        def torch_route(src=None):
            src = xf if src is None else src
            return torch.nn.functional.interpolate(src, size=(S, S), mode="bicubic", align_corners=False).round_().clamp_(0, 255).to(torch.uint8)

        def torch_from_u8():
            return torch_route(x.reshape(n, H, W, 3).permute(0, 3, 1, 2).float())

        for fn in (kernel, torch_route, torch_from_u8):                              # warm-up of every timed shape
            fn()
        torch.cuda.synchronize()
        diff = (kernel().reshape(n, S, S, 3).permute(0, 3, 1, 2).int() - torch_route().int()).abs()
        ms = {"kernel": [], "torch": [], "torch_from_u8": []}
        for _ in range(a.rounds):
            ms["kernel"].append(timed(kernel, calls))
            ms["torch"].append(timed(torch_route, calls))
            ms["torch_from_u8"].append(timed(torch_from_u8, calls))
        nbytes, under = algorithmic_bytes(n)
        k = med(ms["kernel"])
        res[name] = {"frames": n, "kernel_ms_per_call": k, "kernel_ms_rounds": [round(v, 4) for v in ms["kernel"]],
                     "kernel_frames_per_s": n / (k * 1e-3), "torch_ms_per_call": med(ms["torch"]),
                     "torch_ms_rounds": [round(v, 4) for v in ms["torch"]], "torch_frames_per_s": n / (med(ms["torch"]) * 1e-3),
                     "torch_from_u8_ms_per_call": med(ms["torch_from_u8"]), "torch_from_u8_frames_per_s": n / (med(ms["torch_from_u8"]) * 1e-3),
                     "kernel_over_torch": med(ms["torch"]) / k, "rows_cols_under_taps": under, "algorithmic_bytes": nbytes,
                     "whole_source_bytes": n * H * W * 3, "kernel_algorithmic_gb_per_s": nbytes / (k * 1e-3) / 1e9,
                     "kernel_share_of_hbm_peak": nbytes / (k * 1e-3) / HBM_PEAK, "max_abs_diff_grey_levels": int(diff.max()),
                     "share_of_bytes_that_differ": float((diff > 0).float().mean())}
        del x, xf, out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
