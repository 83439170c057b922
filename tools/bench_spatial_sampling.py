#!/usr/bin/env python3
"""The fine-tune spatial sampling at the recipe's shape (32 clips x 16 frames, 224 x 224 from 256 x 340 and 320 x 426 sources, random
resized crop with scale [0.08, 1] and aspect ratio [0.75, 1.3333] plus the flip): device time of the ONE launch of
``tad_spatial_sample`` alone (the table is planned and uploaded before the timed window), from f32 clips and from uint8 frames, and in
the same run, alternating round by round,

  frames_to_clip   ``tad_frames_to_clip`` at the same output size (uint8 [B,T,224,224,3] -> f32): the streaming kernel that writes the
                   same output bytes
  torch            the same windows through torch on the device: per clip slice + ``interpolate(bilinear)`` + ``flip``, then ``stack``

Times are device events around ``--calls`` back-to-back calls, median over ``--rounds``.  GB/s are over the algorithmic bytes: the
bytes of every frame's source window read once plus the output bytes (for frames_to_clip: input plus output).  ``host_ms_per_call`` is
the host side of a whole ``SpatialSampling`` call (plan, table, check, upload, launch).

usage: python tools/bench_spatial_sampling.py [--batch 32] [--frames 16] [--rounds 5] [--calls 200]
Prints one JSON line.
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
S = 224
SOURCES = ((256, 340), (320, 426))
RECIPE = {"scale": (0.08, 1.0), "aspect_ratio": (0.75, 1.3333)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200, help="device calls per round and route")
    a = ap.parse_args()
    B, T = a.batch, a.frames

    import torch
    from simple_tad_amd import kernels as K
    from simple_tad_amd.rand_augment import frames_to_clip
    from simple_tad_amd.spatial_sampling import SpatialSampling
    if not torch.cuda.is_available():
        raise SystemExit("bench_spatial_sampling: no GPU (a measurement does not fall back)")
    res = {"bench": "spatial_sampling", "batch": B, "frames": T, "output": S, "calls": a.calls, "rounds": a.rounds}
    med = lambda v: float(np.median(v))
    ss = SpatialSampling(crop_size=S, **RECIPE)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls

    rng = np.random.default_rng(0)
    small = torch.from_numpy(rng.integers(0, 256, (B, T, S, S, 3), dtype=np.uint8)).cuda()
    small_out = torch.empty((B, 3, T, S, S), device="cuda")
    for H, W in SOURCES:
        u8 = torch.from_numpy(rng.integers(0, 256, (B, T, H, W, 3), dtype=np.uint8)).cuda()
        x = frames_to_clip(u8, MEAN, STD)
        out = torch.empty((B, 3, T, S, S), device="cuda")
        random.seed(0)
        np.random.seed(0)
        plan = ss.plan(B, T, H, W)
        table = ss.table(plan, B, T, H, W).cuda()
        window_px = sum(w.h * w.w for w in plan)

        def torch_route():
            clips = []
            for b in range(B):
                w = plan[b * T]
                c = torch.nn.functional.interpolate(x[b, :, :, w.i:w.i + w.h, w.j:w.j + w.w], size=(S, S), mode="bilinear", align_corners=False)
                clips.append(c.flip(-1) if w.flip else c)
            return torch.stack(clips)

        routes = {"f32": lambda: K.spatial_sample(x, table, S, out=out),
                  "uint8": lambda: K.spatial_sample(u8, table, S, MEAN, STD, out=out),
                  "frames_to_clip": lambda: K.frames_to_clip(small, MEAN, STD, small_out),
                  "torch": torch_route}
        # the routes agree before they are timed (torch's own f32 arithmetic differs in the last bits)
        got = K.spatial_sample(x, table, S).clone()
        assert torch.equal(got, K.spatial_sample(u8, table, S, MEAN, STD))
        worst = float((got - torch_route()).abs().max())
        assert worst < 1e-4, worst
        for fn in routes.values():                            # warm-up of every route at the timed shape
            for _ in range(3):
                fn()
        ms = {k: [] for k in routes}
        for _ in range(a.rounds):
            for k, fn in routes.items():
                ms[k].append(timed(fn))
        host = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                ss(x, out=out)
            host.append((time.perf_counter() - t0) * 1e3 / a.calls)
            torch.cuda.synchronize()
        out_bytes = out.numel() * 4
        nbytes = {"f32": window_px * 3 * 4 + out_bytes, "uint8": window_px * 3 + out_bytes, "frames_to_clip": small.numel() + out_bytes,
                  "torch": window_px * 3 * 4 + out_bytes}
        res[f"{H}x{W}"] = {"mean_window_px": window_px / (B * T), "max_abs_diff_to_torch": worst, "host_ms_per_call": med(host),
                           **{k: {"device_ms_per_call": round(med(v), 4), "device_ms_rounds": [round(t, 4) for t in v],
                                  "algorithmic_mb": round(nbytes[k] / 1e6, 1), "gb_per_s": round(nbytes[k] / (med(v) * 1e-3) / 1e9, 1)}
                              for k, v in ms.items()}}
        del u8, x, out, table
    print(json.dumps(res))


if __name__ == "__main__":
    main()
