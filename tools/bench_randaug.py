#!/usr/bin/env python3
"""RandAugment at the workload's shape (32 clips x 16 frames x 224 x 224 x 3, --aa rand-m6-n3-mstd0.5-inc1, bicubic,
DRIVE_TRANSFORMS): device time and host time per call of ``rand_augment.RandAugment`` and of ``frames_to_clip``, and -- where PIL is
importable -- the host time of the SAME plans through PIL on one core and on a pool of worker processes (``--workers``, default 16: the
CPUs a job owns), measured in the same process, alternating with the device calls.

The PIL side restates each plan row with PIL's public functions (ImageOps, ImageEnhance, Image.transform / rotate), frame by frame,
as the reference's dataset workers do.  The pool is started (spawn) before the GPU is initialised; its workers never touch the GPU.
Each worker builds the same seeded frames once when it starts, receives a clip's index and plan rows, and returns one checksum: no
clip crosses a process boundary inside the timed window, as a loader worker decodes in place.

``engine_loop``: ms per step of engine.train_one_epoch for ViT-B at --batch clips (DataParallel + FusedAdamW, as bench.py's
engine_loop): the parent's loop on f32 clips [B,3,T,H,W] without ``augment_fn``, against the loop on uint8 frames [B,T,H,W,3] with
``augment_fn`` = RandAugment + frames_to_clip, alternating in one process, best round of each.

usage: python tools/bench_randaug.py [--batch 32] [--frames 16] [--size 224] [--rounds 5] [--workers 16] [--pil-clips 32]
                                     [--steps 10] [--loop-rounds 3] [--skip-loop]
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
POLICY = "rand-m6-n3-mstd0.5-inc1"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


_FRAMES = None


def make_frames(B, T, S):
    """the seeded input frames uint8 [B,T,S,S,3]: a diagonal gradient plus noise"""
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:S, 0:S]
    base = ((xx + yy) * 255.0 / (2 * S - 2))[None, None, :, :, None]
    return np.clip(base + rng.normal(0, 25, (B, T, S, S, 3)), 0, 255).astype(np.uint8)


def worker_init(B, T, S):
    global _FRAMES
    _FRAMES = make_frames(B, T, S)


def pil_job(job):
    """a pool worker's task: clip ``b`` of its own copy of the frames through ``rows``; returns a checksum"""
    b, rows = job
    return int(pil_clip((_FRAMES[b], rows)).sum())


def pil_clip(job):
    """one clip [T,H,W,3] through its plan rows (name, arg, resample per frame) with PIL; returns the augmented clip"""
    from PIL import Image, ImageEnhance, ImageOps
    clip, rows = job
    imgs = [Image.fromarray(f) for f in clip]
    w, h = imgs[0].size
    fill = (128, 128, 128)
    for name, arg, resample in rows:
        base = name.replace("Increasing", "")
        out = []
        for t, im in enumerate(imgs):
            if base == "AutoContrast":
                im = ImageOps.autocontrast(im)
            elif base == "Equalize":
                im = ImageOps.equalize(im)
            elif base == "Invert":
                im = ImageOps.invert(im)
            elif base == "Posterize":
                im = im if arg >= 8 else ImageOps.posterize(im, arg)
            elif base == "Solarize":
                im = ImageOps.solarize(im, arg)
            elif base == "SolarizeAdd":
                im = im.point([min(255, i + arg) if i < 128 else i for i in range(256)] * 3)
            elif base in ("Color", "Contrast", "Brightness", "Sharpness"):
                im = getattr(ImageEnhance, base)(im).enhance(arg)
            elif base == "Rotate":
                im = im.rotate(arg, resample=resample[t], fillcolor=fill)
            else:
                m = {"ShearX": (1, arg, 0, 0, 1, 0), "ShearY": (1, 0, 0, arg, 1, 0), "TranslateXRel": (1, 0, arg * w, 0, 1, 0),
                     "TranslateYRel": (1, 0, 0, 0, 1, arg * h)}[base]
                im = im.transform(im.size, Image.AFFINE, m, resample=resample[t], fillcolor=fill)
            out.append(im)
        imgs = out
    return np.stack([np.asarray(im) for im in imgs])


def engine_loop(ra, frames, steps, rounds):
    import torch
    import simple_tad_amd as TAD
    from simple_tad_amd import engine as E
    from simple_tad_amd import rand_augment as RA
    from simple_tad_amd.loss import LabelSmoothingCrossEntropy
    from simple_tad_amd.parallel import DataParallel
    torch.manual_seed(0)
    dev = torch.device("cuda")
    B, T = frames.shape[:2]
    model = TAD.create_model("vit_base_patch16_224", pretrained=False, num_classes=400, all_frames=T, tubelet_size=2,
                             final_reduction="fc_norm", init_scale=0.001, use_flash_attn=True).to(dev)
    model.train()
    dp = DataParallel(model, bucket_mb=64.0)
    opt = E.create_optimizer(dp, lr=1e-3, weight_decay=0.05, layer_decay=0.75)
    scaler = E.NativeScalerWithGradNormCount(dp)
    clips = RA.frames_to_clip(frames, MEAN, STD)          # what the parent's loop is fed: normalised f32 clips
    y = torch.randint(0, 400, (B,), device=dev)
    nel = 2 + steps
    lr = E.cosine_scheduler(1e-4, 1e-6, 1, nel, warmup_epochs=0)
    crit = LabelSmoothingCrossEntropy(0.1)
    augment = lambda u: RA.frames_to_clip(ra(u), MEAN, STD)

    def run(samples, augment_fn):
        t1 = [None]

        def log(epoch, i, stats):
            if i == 1:  # two warm-up iterations
                torch.cuda.synchronize()
                t1[0] = time.perf_counter()
        kw = {} if augment_fn is None else {"augment_fn": augment_fn}
        E.train_one_epoch(dp, crit, [(samples, y)] * nel, opt, dev, 0, scaler, lr_schedule_values=lr, num_training_steps_per_epoch=nel,
                          log=log, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t1[0]) / (nel - 2)

    best = {"without": float("inf"), "with": float("inf")}
    for _ in range(rounds):
        best["without"] = min(best["without"], run(clips, None))
        best["with"] = min(best["with"], run(frames, augment))
    out = {k: {"clips_per_s": round(B / v, 2), "ms_per_step": round(1e3 * v, 3)} for k, v in best.items()}
    out["cost_ms_per_step"] = round(1e3 * (best["with"] - best["without"]), 3)
    out["cost_pct"] = round(100.0 * (best["with"] / best["without"] - 1.0), 2)
    out.update(batch=B, steps=steps, rounds=rounds)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="device calls per round")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--pil-clips", type=int, default=32, help="clips per round on the PIL side (times are scaled to --batch)")
    ap.add_argument("--steps", type=int, default=10, help="timed steps per engine-loop round")
    ap.add_argument("--loop-rounds", type=int, default=3)
    ap.add_argument("--skip-loop", action="store_true")
    a = ap.parse_args()
    B, T, S = a.batch, a.frames, a.size
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    pool = None
    if have_pil and a.workers > 1:
        import multiprocessing as mp
        pool = mp.get_context("spawn").Pool(a.workers, initializer=worker_init, initargs=(B, T, S))
        pool.map(abs, range(4 * a.workers))              # (workers up, their frames built, before the GPU is opened)

    import torch
    from simple_tad_amd import rand_augment as RA
    if not torch.cuda.is_available():
        raise SystemExit("bench_randaug: no GPU (a measurement does not fall back)")
    host = make_frames(B, T, S)
    x = torch.from_numpy(host).cuda()
    ra = RA.create_random_augment((S, S), POLICY, "bicubic", RA.DRIVE_TRANSFORMS)
    random.seed(0)
    np.random.seed(0)
    for _ in range(3):                                   # warm-up: library load, allocator, every kernel
        RA.frames_to_clip(ra(x), MEAN, STD)
    torch.cuda.synchronize()

    dev_ms, f2c_ms, host_ms, pil1_s, pilN_s, applied = [], [], [], [], [], []
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for r in range(a.rounds):
        t0 = time.perf_counter()
        plans = [ra.plan(B, T) for _ in range(a.calls)]
        plan_s = time.perf_counter() - t0
        applied.append(np.mean([sum(p.applied for p in rows) / B for rows in plans]))
        torch.cuda.synchronize()
        e0, e1, e2 = ev(), ev(), ev()
        t0 = time.perf_counter()
        e0.record()
        outs = [ra.apply(x, rows) for rows in plans]
        t1 = time.perf_counter()
        e1.record()
        for o in outs:
            RA.frames_to_clip(o, MEAN, STD)
        e2.record()
        torch.cuda.synchronize()
        host_ms.append((t1 - t0 + plan_s) * 1e3 / a.calls)      # plan, table, upload, launches
        dev_ms.append(e0.elapsed_time(e1) / a.calls)
        f2c_ms.append(e1.elapsed_time(e2) / a.calls)
        if have_pil:
            n = min(a.pil_clips, B)
            jobs = [(host[b], [(RA.OP_NAMES[p.op], p.arg, p.resample) for p in plans[0] if p.clip == b and p.applied]) for b in range(n)]
            t0 = time.perf_counter()
            for j in jobs[:max(1, n // 4)]:
                pil_clip(j)
            pil1_s.append((time.perf_counter() - t0) * B / max(1, n // 4))
            if pool is not None:
                t0 = time.perf_counter()
                pool.map(pil_job, [(b, rows) for b, (_, rows) in enumerate(jobs)], chunksize=1)
                pilN_s.append((time.perf_counter() - t0) * B / n)
    if pool is not None:
        pool.close()
        pool.join()
    med = lambda v: float(np.median(v)) if len(v) else None
    res = {"bench": "randaug", "shape": [B, T, S, S, 3], "policy": POLICY, "applied_ops_per_clip": med(applied),
           "device_ms_per_call": med(dev_ms), "device_ms_rounds": [round(v, 3) for v in dev_ms],
           "host_ms_per_call": med(host_ms), "frames_to_clip_device_ms": med(f2c_ms),
           "device_clips_per_s": B / (med(dev_ms) * 1e-3),
           "pil_one_core_s_per_batch": med(pil1_s), "pil_one_core_clips_per_s": (B / med(pil1_s)) if pil1_s else None,
           "pil_workers": a.workers if pilN_s else None, "pil_workers_s_per_batch": med(pilN_s),
           "pil_workers_clips_per_s": (B / med(pilN_s)) if pilN_s else None}
    if not a.skip_loop:
        res["engine_loop"] = engine_loop(ra, x, a.steps, a.loop_rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
