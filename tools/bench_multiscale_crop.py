#!/usr/bin/env python3
"""The MAE pre-training crop at the workload's shapes (32 clips x 16 frames): device time and host time per call of
``transforms.GroupMultiScaleCrop`` with the fused f32 output, for
  pretrain     320 x 568 -> 224, scales [1, .875, .75, .66]          (the reference's pre-training datasets: short side 320, 16:9)
  lightcrop    224 x 224 -> 224, scales [1, 1, .975, .95, .9, .875, .85]   (the "finetune-align" route)
and -- where PIL is importable -- the host time of the SAME crops through PIL (crop, BILINEAR resize, the f32 normalisation in
numpy) on one core and on a pool of worker processes (``--workers``, default 16: the CPUs a job owns), measured in the same
process, alternating with the device calls.  The pool is started (spawn) before the GPU is initialised; its workers never touch the
GPU.  Each worker builds the same seeded frames once when it starts, receives a clip's index and crop, and returns one checksum.

``engine_loop``: ms per step of engine_pretrain.train_one_epoch for pretrain_videomae_base_patch16_224 at --batch clips: the parent's
loop on f32 clips [B,3,T,224,224] and masks without ``augment_fn``, against the loop on uint8 frames [B,T,320,568,3] with
``augment_fn`` = DataAugmentationForVideoMAE, alternating in one process, best round of each.

usage: python tools/bench_multiscale_crop.py [--batch 32] [--frames 16] [--rounds 5] [--calls 10] [--workers 16] [--pil-clips 32]
                                             [--steps 10] [--loop-rounds 3] [--skip-loop]
Prints one JSON line.
"""
import argparse
import json
import os
import random
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
S = 224
SHAPES = {"pretrain": ((320, 568), [1, .875, .75, .66]), "lightcrop": ((224, 224), [1, 1, .975, .95, .9, .875, .85])}

_FRAMES = {}


def make_frames(B, T, Hs, Ws):
    """the seeded input frames uint8 [B,T,Hs,Ws,3]: a diagonal gradient plus noise"""
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    base = ((xx + yy) * 255.0 / (Hs + Ws - 2))[None, None, :, :, None]
    return np.clip(base + rng.normal(0, 25, (B, T, Hs, Ws, 3)), 0, 255).astype(np.uint8)


def worker_init(B, T):
    for name, ((Hs, Ws), _) in SHAPES.items():
        _FRAMES[name] = make_frames(B, T, Hs, Ws)


def pil_clip(clip, crop):
    """one clip [T,Hs,Ws,3] through its crop (w, h, x0, y0) with PIL, then the normalisation: the f32 clip [3,T,S,S]"""
    from PIL import Image
    w, h, x0, y0 = crop
    out = np.stack([np.asarray(Image.fromarray(f).crop((x0, y0, x0 + w, y0 + h)).resize((S, S), Image.BILINEAR)) for f in clip])
    v = (out.astype(np.float32) / np.float32(255) - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32)
    return np.ascontiguousarray(v.transpose(3, 0, 1, 2))


def pil_job(job):
    name, b, crop = job
    return float(pil_clip(_FRAMES[name][b], crop).sum())


def engine_loop(frames, B, T, steps, rounds):
    import torch
    import simple_tad_amd as TAD
    from simple_tad_amd import engine as E, engine_pretrain as EP
    from simple_tad_amd import transforms as TF
    from simple_tad_amd.parallel import DataParallel
    torch.manual_seed(0)
    dev = torch.device("cuda")
    model = TAD.create_model("pretrain_videomae_base_patch16_224", pretrained=False).to(dev)
    dp = DataParallel(model, bucket_mb=64.0)
    opt = E.create_optimizer(dp, lr=1e-3, weight_decay=0.05)
    scaler = E.NativeScalerWithGradNormCount(dp)
    aug = TF.DataAugmentationForVideoMAE(SimpleNamespace(input_size=S, mask_type="tube", window_size=(T // 2, S // 16, S // 16),
                                                         mask_ratio=0.9))
    clips, masks = aug(frames)                             # what the parent's loop is fed: normalised f32 clips and masks
    nel = 2 + steps
    lr = E.cosine_scheduler(1e-4, 1e-6, 1, nel, warmup_epochs=0)

    def run(batch, augment_fn):
        t1 = [None]

        def log(epoch, i, stats):
            if i == 1:  # two warm-up iterations
                torch.cuda.synchronize()
                t1[0] = time.perf_counter()
        kw = {} if augment_fn is None else {"augment_fn": augment_fn}
        EP.train_one_epoch(dp, [batch] * nel, opt, dev, 0, scaler, lr_schedule_values=lr, log=log, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t1[0]) / (nel - 2)

    best = {"without": float("inf"), "with": float("inf")}
    for _ in range(rounds):
        best["without"] = min(best["without"], run((clips, masks), None))
        best["with"] = min(best["with"], run((frames,), aug))
    out = {k: {"clips_per_s": round(B / v, 2), "ms_per_step": round(1e3 * v, 3)} for k, v in best.items()}
    out["cost_ms_per_step"] = round(1e3 * (best["with"] - best["without"]), 3)
    out["cost_pct"] = round(100.0 * (best["with"] / best["without"] - 1.0), 2)
    out.update(batch=B, steps=steps, rounds=rounds)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="device calls per round")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--pil-clips", type=int, default=32, help="clips per round on the PIL side (times are scaled to --batch)")
    ap.add_argument("--steps", type=int, default=10, help="timed steps per engine-loop round")
    ap.add_argument("--loop-rounds", type=int, default=3)
    ap.add_argument("--skip-loop", action="store_true")
    a = ap.parse_args()
    B, T = a.batch, a.frames
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    pool = None
    if have_pil and a.workers > 1:
        import multiprocessing as mp
        pool = mp.get_context("spawn").Pool(a.workers, initializer=worker_init, initargs=(B, T))
        pool.map(abs, range(4 * a.workers))              # (workers up, their frames built, before the GPU is opened)

    import torch
    from simple_tad_amd import transforms as TF
    if not torch.cuda.is_available():
        raise SystemExit("bench_multiscale_crop: no GPU (a measurement does not fall back)")
    res = {"bench": "multiscale_crop", "batch": B, "frames": T, "output": S}
    ev = lambda: torch.cuda.Event(enable_timing=True)
    med = lambda v: float(np.median(v)) if len(v) else None
    x_pretrain = None
    for name, ((Hs, Ws), scales) in SHAPES.items():
        host = make_frames(B, T, Hs, Ws)
        x = torch.from_numpy(host).cuda()
        if name == "pretrain":
            x_pretrain = x
        tf = TF.GroupMultiScaleCrop(S, scales)
        out = torch.empty((B, 3, T, S, S), device="cuda")
        random.seed(0)
        for _ in range(3):                               # warm-up: library load, allocator, the kernel
            tf(x, out=out, normalize=(MEAN, STD))
        torch.cuda.synchronize()
        dev_ms, host_ms, pil1_s, pilN_s = [], [], [], []
        for r in range(a.rounds):
            t0 = time.perf_counter()
            plans = [tf.plan(B, (Ws, Hs)) for _ in range(a.calls)]
            plan_s = time.perf_counter() - t0
            torch.cuda.synchronize()
            e0, e1 = ev(), ev()
            t0 = time.perf_counter()
            e0.record()
            for plan in plans:
                tf.apply(x, plan, out=out, normalize=(MEAN, STD))
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            host_ms.append((t1 - t0 + plan_s) * 1e3 / a.calls)      # plan, coefficient sets, table, upload, launch
            dev_ms.append(e0.elapsed_time(e1) / a.calls)
            if have_pil:
                n = min(a.pil_clips, B)
                crops = [tuple(plans[0][b][1:]) for b in range(n)]
                t0 = time.perf_counter()
                for b in range(max(1, n // 4)):
                    pil_clip(host[b], crops[b])
                pil1_s.append((time.perf_counter() - t0) * B / max(1, n // 4))
                if pool is not None:
                    t0 = time.perf_counter()
                    pool.map(pil_job, [(name, b, crops[b]) for b in range(n)], chunksize=1)
                    pilN_s.append((time.perf_counter() - t0) * B / n)
        nbytes = x.numel() + out.numel() * 4
        res[name] = {"source": [Hs, Ws], "scales": scales, "device_ms_per_call": med(dev_ms), "device_ms_rounds": [round(v, 3) for v in dev_ms],
                     "device_gb_per_s": nbytes / (med(dev_ms) * 1e-3) / 1e9, "host_ms_per_call": med(host_ms),
                     "device_clips_per_s": B / (med(dev_ms) * 1e-3),
                     "pil_one_core_s_per_batch": med(pil1_s), "pil_one_core_clips_per_s": (B / med(pil1_s)) if pil1_s else None,
                     "pil_workers": a.workers if pilN_s else None, "pil_workers_s_per_batch": med(pilN_s),
                     "pil_workers_clips_per_s": (B / med(pilN_s)) if pilN_s else None}
        del x, out
    if pool is not None:
        pool.close()
        pool.join()
    if not a.skip_loop:
        res["engine_loop"] = engine_loop(x_pretrain, B, T, a.steps, a.loop_rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
