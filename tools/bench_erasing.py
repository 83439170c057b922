"""RandomErasing cost on the GPU (random_erasing.RandomErasing): prints ONE JSON line.

At --batch x 3 x 16 x 224^2 f32, mode ``pixel``, max_area 0.1 (the recipe), for ``probability`` 0.25 and 1.0, with ONE plan per
probability (``random.seed`` before every call, so both paths erase the same boxes every time):
* device_ms: device time (HIP events around --iters calls, after a warm-up call) of the one ``tad_erase_clips`` launch on an uploaded
  table, against the torch expressions of the same plan on the device (``normal_()`` + a strided write per box and frame: the
  reference's CPU expression moved to the GPU, which is what a loop without this kernel would run);
* call_ms: host clock around --iters whole ``RandomErasing.__call__`` (draws, table, pinned upload, launch) ending in a device
  synchronise, against the same for the torch-expression path.
The two paths alternate round by round in one process; the best round of each is reported.  ``launches`` counts the device launches
of one call (1 + the table copy against two per box and frame); ``erased_MB`` is the bytes a call writes.

usage: python tools/bench_erasing.py [--iters 50] [--rounds 3] [--batch 32]
"""
import argparse
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from simple_tad_amd import kernels as K  # noqa: E402
from simple_tad_amd._lib import ERASE_PIXEL  # noqa: E402
from simple_tad_amd.random_erasing import RandomErasing  # noqa: E402

PLAN_SEED = 1


def _gpu_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _wall_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / iters


def _alternate(variants, timer, iters, rounds):
    best = {k: float("inf") for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            best[k] = min(best[k], timer(fn, iters))
    return best


def figures(batch, probability, iters, rounds):
    shape = (batch, 3, 16, 224, 224)
    x = torch.randn(shape, device="cuda")
    fn = RandomErasing(probability, mode="pixel", max_count=1, num_splits=1, max_area=0.1)
    random.seed(PLAN_SEED)
    boxes = fn.plan(batch, *shape[2:])
    table = K.erase_box_table([(s, ERASE_PIXEL, *rest) for s, *rest in boxes], batch, *shape[2:]).cuda()
    frames = lambda s, t: x[s, :, t]

    def call_kernel():
        random.seed(PLAN_SEED)
        fn(x)

    def call_torch():
        random.seed(PLAN_SEED)
        with torch.no_grad():
            fn._erase_torch(frames, fn.plan(batch, *shape[2:]))

    dev = _alternate({"kernel": lambda: K.erase_clips(x, table, 7), "torch": lambda: fn._erase_torch(frames, boxes)}, _gpu_ms, iters,
                     rounds)
    wall = _alternate({"kernel": call_kernel, "torch": call_torch}, _wall_ms, iters, rounds)
    elements = sum(3 * (t1 - t0) * (y1 - y0) * (x1 - x0) for _, t0, t1, y0, y1, x0, x1 in boxes)
    frames_erased = sum(t1 - t0 for _, t0, t1, *_ in boxes)
    return {"boxes": len(boxes), "erased_MB": round(4e-6 * elements, 3),
            "launches": {"kernel": 2 if boxes else 0, "torch": 2 * frames_erased},
            "device_ms": {k: round(v, 4) for k, v in dev.items()}, "call_ms": {k: round(v, 4) for k, v in wall.items()},
            "device_speedup": round(dev["torch"] / dev["kernel"], 1) if boxes else None,
            "call_speedup": round(wall["torch"] / wall["kernel"], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_erasing needs a GPU"
    res = {f"p{p}": figures(args.batch, p, args.iters, args.rounds) for p in (0.25, 1.0)}
    print(json.dumps({"bench": "erasing", "shape": [args.batch, 3, 16, 224, 224], "mode": "pixel", "iters": args.iters,
                      "rounds": args.rounds, **res}))


if __name__ == "__main__":
    main()
