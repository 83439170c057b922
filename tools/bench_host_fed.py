"""Does the training rate survive a loader?  engine.train_one_epoch for ViT-B/16, 16 x 224^2, --batch clips (forward + backward + AdamW,
DataParallel + FusedAdamW: the loop shape of bench.py's engine_loop) fed six ways, interleaved in one process:

  resident              one device batch reused (what bench.py times)
  naive_f32             a fresh pageable host tensor per step: the engine's own .to(device) copies it on the compute stream
  naive_u8              the same as uint8 frames [B,T,H,W,3] into the model's uint8 input stage
  prefetch_f32          f32 clips through prefetch.ClipPrefetcher (pinned ring, side stream)
  prefetch_f32_operand  f32 clips with wire="operand": rounded to the 16-bit operand format in the staging pass, half the wire bytes
  prefetch_u8           uint8 frames through the prefetcher

"Fresh per step" = the loader rotates through --buffers (>= 4) distinct pageable tensors, as a DataLoader hands them over.  Every leg is
warmed up once (its shapes, its kernels, the prefetcher's pinned slots) before anything is timed; then --rounds (>= 3) rounds, each running
every leg once for --steps timed steps after two un-timed ones.  Per leg: median and spread (min, max) of clips/s over the rounds and the
host-to-device bytes per step.  ``copies``: what moving one batch costs by itself on an idle device -- the pinned H2D copy (HIP events)
and the host staging pass (pageable -> pinned, with the rounding for the operand wire) -- so that a missed target can be read against
bytes / time.  Target (not an assertion): prefetch_u8 >= 0.98 x resident in the same run.

Writes ONE JSON object to --out (default profiles/host_fed.json) and prints it on one line.

usage: python tools/bench_host_fed.py [--batch 32] [--steps 10] [--rounds 3] [--depth 2] [--buffers 4] [--out profiles/host_fed.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import simple_tad_amd as T  # noqa: E402
from simple_tad_amd import ClipPrefetcher, engine as E  # noqa: E402
from simple_tad_amd.parallel import DataParallel  # noqa: E402

LEGS = ("resident", "naive_f32", "naive_u8", "prefetch_f32", "prefetch_f32_operand", "prefetch_u8")
FRAMES, SIZE = 16, 224


class Rotating:
    """a loader of ``n`` batches that hands over ``buffers`` distinct host tensors in turn"""

    def __init__(self, clips, targets, n):
        self.clips, self.targets, self.n = clips, targets, n

    def __len__(self):
        return self.n

    def __iter__(self):
        for i in range(self.n):
            yield self.clips[i % len(self.clips)], self.targets[i % len(self.targets)]


def copy_costs(batch, dev, iters=5):
    """ms and GB/s of one batch's pinned H2D copy and of its host staging pass, per wire format, nothing else running"""
    out = {}
    src32 = torch.randn(batch, 3, FRAMES, SIZE, SIZE)
    for name, host, wire in (("f32", src32, torch.float32), ("operand16", src32, torch.bfloat16),
                             ("u8", torch.randint(0, 256, (batch, FRAMES, SIZE, SIZE, 3), dtype=torch.uint8), torch.uint8)):
        pinned = torch.empty(host.shape, dtype=wire, pin_memory=True)
        dst = torch.empty(host.shape, dtype=wire, device=dev)
        pinned.copy_(host)
        t = time.perf_counter()
        for _ in range(iters):
            pinned.copy_(host)
        stage_ms = (time.perf_counter() - t) * 1e3 / iters
        dst.copy_(pinned, non_blocking=True)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            dst.copy_(pinned, non_blocking=True)
        b.record()
        b.synchronize()
        h2d_ms = a.elapsed_time(b) / iters
        nbytes = pinned.numel() * pinned.element_size()
        out[name] = {"bytes": nbytes, "h2d_pinned_ms": round(h2d_ms, 3), "h2d_pinned_GBps": round(nbytes / h2d_ms / 1e6, 1),
                     "staging_host_ms": round(stage_ms, 3), "staging_host_GBps_written": round(nbytes / stage_ms / 1e6, 1)}
        del pinned, dst
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "host_fed.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_host_fed needs a GPU"
    assert args.rounds >= 3 and args.buffers >= 4, "at least three rounds and four distinct host buffers"
    torch.manual_seed(0)
    dev = torch.device("cuda", torch.cuda.current_device())
    B = args.batch
    model = T.create_model("vit_base_patch16_224", pretrained=False, num_classes=2, all_frames=FRAMES, tubelet_size=2,
                           final_reduction="fc_norm", init_scale=0.001, use_flash_attn=True).to(dev)
    model.train()
    dp = DataParallel(model, bucket_mb=64.0)
    opt = E.create_optimizer(dp, lr=1e-3, weight_decay=0.05, layer_decay=0.75)
    scaler = E.NativeScalerWithGradNormCount(dp)
    crit = torch.nn.CrossEntropyLoss()
    nel = 2 + args.steps
    lr = E.cosine_scheduler(1e-4, 1e-6, 1, nel, warmup_epochs=0)

    base = torch.randn(B, 3, FRAMES, SIZE, SIZE)
    f32 = [base] + [base + 0.01 * i for i in range(1, args.buffers)]      # pageable, distinct
    u8 = [torch.randint(0, 256, (B, FRAMES, SIZE, SIZE, 3), dtype=torch.uint8) for _ in range(args.buffers)]
    ys = [torch.randint(0, 2, (B,)) for _ in range(args.buffers)]
    assert not any(t.is_pinned() for t in f32 + u8)
    x_dev, y_dev = f32[0].to(dev), ys[0].to(dev)
    pf = {"prefetch_f32": ClipPrefetcher(Rotating(f32, ys, nel), dev, depth=args.depth),
          "prefetch_f32_operand": ClipPrefetcher(Rotating(f32, ys, nel), dev, depth=args.depth, wire="operand"),
          "prefetch_u8": ClipPrefetcher(Rotating(u8, ys, nel), dev, depth=args.depth)}
    loaders = {"resident": [(x_dev, y_dev)] * nel, "naive_f32": Rotating(f32, ys, nel), "naive_u8": Rotating(u8, ys, nel), **pf}
    tgt = ys[0].numel() * ys[0].element_size()
    h2d = {"resident": 0, "naive_f32": 4 * base.numel() + tgt, "naive_u8": u8[0].numel() + tgt, "prefetch_f32": 4 * base.numel() + tgt,
           "prefetch_f32_operand": 2 * base.numel() + tgt, "prefetch_u8": u8[0].numel() + tgt}

    def run(leg):
        t1 = [None]

        def log(epoch, i, stats):
            if i == 1:  # two un-timed iterations
                torch.cuda.synchronize()
                t1[0] = time.perf_counter()
        E.train_one_epoch(dp, crit, loaders[leg], opt, dev, 0, scaler, lr_schedule_values=lr, num_training_steps_per_epoch=nel, log=log)
        torch.cuda.synchronize()
        return B * (nel - 2) / (time.perf_counter() - t1[0])

    for leg in LEGS:  # warm-up: every shape, every kernel route, the pinned slots
        run(leg)
    rates = {leg: [] for leg in LEGS}
    for _ in range(args.rounds):
        for leg in LEGS:
            rates[leg].append(run(leg))
    for p in pf.values():
        p.close()
    legs = {}
    for leg in LEGS:
        med = statistics.median(rates[leg])
        legs[leg] = {"clips_per_s_median": round(med, 2), "clips_per_s_min": round(min(rates[leg]), 2), "clips_per_s_max": round(max(rates[leg]), 2),
                     "spread_pct": round(100.0 * (max(rates[leg]) - min(rates[leg])) / med, 2), "ms_per_step_median": round(1e3 * B / med, 3),
                     "h2d_bytes_per_step": h2d[leg], "rounds": [round(v, 2) for v in rates[leg]]}
    res = legs["resident"]["clips_per_s_median"]
    for leg in LEGS:
        legs[leg]["vs_resident"] = round(legs[leg]["clips_per_s_median"] / res, 4)
    out = {"bench": "host_fed", "device": torch.cuda.get_device_name(dev), "model": "vit_base_patch16_224", "batch": B, "frames": FRAMES,
           "steps": args.steps, "rounds": args.rounds, "depth": args.depth, "host_buffers": args.buffers, "precision": T.get_precision(),
           "through": "simple_tad_amd.engine.train_one_epoch (two host syncs per step)", "legs": legs,
           "target": {"what": "prefetch_u8 >= 0.98 x resident", "ratio": legs["prefetch_u8"]["vs_resident"],
                      "met": legs["prefetch_u8"]["vs_resident"] >= 0.98},
           "copies": copy_costs(B, dev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
