"""Mixup / CutMix and soft-target loss cost on the GPU (mixup.Mixup, loss.SoftTargetCrossEntropy): prints ONE JSON line.

* clips: device time of one ``tad_mixup_clips`` launch at --batch x 3 x 16 x 224^2 for a blend in each mode and a batch-mode paste,
  against the reference's torch expression for the same plan (mixup.py:159-207; the parent of this feature has no mixup, so that
  expression is the baseline), the two alternating round by round in one process, best round of each.  GB/s from the algorithmic
  bytes: one read and one write of every element a plan touches (8 B per blended element, 8 B per pasted one).  ``vs_ema_stream`` =
  that rate over the 5.29 TB/s the EMA kernel streams at on this chip.
* host: host time of one ``Mixup.__call__`` (draws, table, upload, two launches) on a small clip, where the GPU is never in the way,
  and of one soft-target loss forward + backward, against their torch expressions.
* loss: device time of forward + backward of the soft-target loss at [--batch, 400] logits, kernel against torch expression.
* engine_loop: ms per step of engine.train_one_epoch for ViT-B at --batch clips (DataParallel + FusedAdamW, as bench.py's
  engine_loop) without mixup (LabelSmoothingCrossEntropy) and with it (Mixup 0.8 / 1.0 + SoftTargetCrossEntropy), alternating.

usage: python tools/bench_mixup.py [--iters 20] [--rounds 3] [--steps 10] [--batch 32] [--skip-loop]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simple_tad_amd as T  # noqa: E402
from simple_tad_amd import engine as E  # noqa: E402
from simple_tad_amd import kernels as K  # noqa: E402
from simple_tad_amd.loss import LabelSmoothingCrossEntropy, SoftTargetCrossEntropy  # noqa: E402
from simple_tad_amd.mixup import Mixup  # noqa: E402
from simple_tad_amd.parallel import DataParallel  # noqa: E402

EMA_STREAM_GBPS = 5290.0


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


def _host_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    ms = (time.perf_counter() - t) * 1e3 / iters
    torch.cuda.synchronize()
    return ms


def _alternate(variants, iters, rounds):
    best = {k: float("inf") for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            best[k] = min(best[k], _gpu_ms(fn, iters))
    return best


def clip_figures(batch, iters, rounds):
    shape = (batch, 3, 16, 224, 224)
    x = torch.randn(shape, device="cuda")
    T_, H, W = shape[2:]
    f32 = np.float32
    lam = 0.3
    lam32 = f32(lam)
    whole = (0, T_, 0, H, 0, W)
    box = (0, T_, 33, 191, 33, 191)           # lam 0.5: edges inside a float4 on both sides
    plans = {
        "blend_batch": [(1, lam, 1. - lam, None)] * batch,
        "blend_pair": [(1, lam32, 1 - lam32, None)] * batch,
        "blend_elem": [(1, f32(0.1 + 0.8 * i / batch), 1 - f32(0.1 + 0.8 * i / batch), None) for i in range(batch)],
        "paste_batch": [(2, 0., 1., box)] * batch,
    }
    fn = Mixup()
    out = {}
    for name, rows in plans.items():
        table = K.mixup_plan_table([(k, f32(a), f32(b), whole if bx is None else bx, f32(0.5), f32(0.5)) for k, a, b, bx in rows], T_, H, W)
        plan = table.cuda()
        if name == "blend_batch":
            def ref():
                flipped = x.flip(0).mul_(1. - lam)
                x.mul_(lam).add_(flipped)
        elif name == "paste_batch":
            def ref():
                x[..., box[2]:box[3], box[4]:box[5]] = x.flip(0)[..., box[2]:box[3], box[4]:box[5]]
        else:
            def ref(rows=rows):
                fn._mix_torch(x, rows)
        best = _alternate({"kernel": lambda: K.mixup_clips(x, plan), "torch": ref}, iters, rounds)
        touched = x.numel() if rows[0][0] == 1 else batch * 3 * T_ * (box[3] - box[2]) * (box[5] - box[4])
        nbytes = 8.0 * touched
        gbps = nbytes / best["kernel"] / 1e6
        out[name] = {"kernel_ms": round(best["kernel"], 4), "torch_ms": round(best["torch"], 4), "MB": round(nbytes / 1e6, 1),
                     "kernel_GBps": round(gbps, 1), "vs_ema_stream": round(gbps / EMA_STREAM_GBPS, 3),
                     "speedup_vs_torch": round(best["torch"] / best["kernel"], 2)}
        x.normal_()
    del x
    torch.cuda.empty_cache()
    return out


def host_figures(batch, iters):
    x = torch.randn(batch, 3, 2, 16, 16, device="cuda")
    y = torch.randint(0, 400, (batch,), device="cuda")
    xs = x.transpose(3, 4)          # a non-contiguous view takes the torch expressions
    out = {}
    for mode in ("batch", "pair", "elem"):
        fn = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, num_classes=400)
        np.random.seed(0)
        out[f"mixup_call_{mode}_ms"] = round(_host_ms(lambda: fn(x, y), iters), 4)
        np.random.seed(0)
        out[f"mixup_call_{mode}_torch_ms"] = round(_host_ms(lambda: fn(xs, y), iters), 4)
    return out


def loss_figures(batch, iters, rounds):
    z = torch.randn(batch, 400, device="cuda", requires_grad=True)
    t = torch.softmax(torch.randn(batch, 400, device="cuda"), -1)
    crit = SoftTargetCrossEntropy()

    def kernel():
        z.grad = None
        crit(z, t).backward()

    def ref():
        z.grad = None
        torch.sum(-t * torch.log_softmax(z, -1), -1).mean().backward()
    best = _alternate({"kernel": kernel, "torch": ref}, iters, rounds)
    return {"fwd_bwd_kernel_ms": round(best["kernel"], 4), "fwd_bwd_torch_ms": round(best["torch"], 4),
            "host_kernel_ms": round(_host_ms(kernel, iters), 4), "host_torch_ms": round(_host_ms(ref, iters), 4)}


def engine_loop(batch, steps, rounds):
    torch.manual_seed(0)
    dev = torch.device("cuda")
    model = T.create_model("vit_base_patch16_224", pretrained=False, num_classes=400, all_frames=16, tubelet_size=2,
                           final_reduction="fc_norm", init_scale=0.001, use_flash_attn=True).to(dev)
    model.train()
    dp = DataParallel(model, bucket_mb=64.0)
    opt = E.create_optimizer(dp, lr=1e-3, weight_decay=0.05, layer_decay=0.75)
    scaler = E.NativeScalerWithGradNormCount(dp)
    x = torch.randn(batch, 3, 16, 224, 224, device=dev)
    y = torch.randint(0, 400, (batch,), device=dev)
    nel = 2 + steps
    lr = E.cosine_scheduler(1e-4, 1e-6, 1, nel, warmup_epochs=0)
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=400)

    def run(mixup_fn):
        t1 = [None]

        def log(epoch, i, stats):
            if i == 1:  # two warm-up iterations
                torch.cuda.synchronize()
                t1[0] = time.perf_counter()
        crit = SoftTargetCrossEntropy() if mixup_fn is not None else LabelSmoothingCrossEntropy(0.1)
        E.train_one_epoch(dp, crit, [(x, y)] * nel, opt, dev, 0, scaler, lr_schedule_values=lr, num_training_steps_per_epoch=nel, log=log,
                          mixup_fn=mixup_fn)
        torch.cuda.synchronize()
        return (time.perf_counter() - t1[0]) / (nel - 2)

    best = {"without": float("inf"), "with": float("inf")}
    for _ in range(rounds):
        best["without"] = min(best["without"], run(None))
        best["with"] = min(best["with"], run(mix))
    out = {k: {"clips_per_s": round(batch / v, 2), "ms_per_step": round(1e3 * v, 3)} for k, v in best.items()}
    out["cost_ms_per_step"] = round(1e3 * (best["with"] - best["without"]), 3)
    out["cost_pct"] = round(100.0 * (best["with"] / best["without"] - 1.0), 2)
    out.update(batch=batch, steps=steps, rounds=rounds)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--skip-loop", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mixup needs a GPU"
    res = {"clips": clip_figures(args.batch, args.iters, args.rounds), "host": host_figures(args.batch, 50),
           "loss": loss_figures(args.batch, 50, args.rounds)}
    if not args.skip_loop:
        res["engine_loop_vit_b"] = engine_loop(args.batch, args.steps, 2)
    print(json.dumps({"bench": "mixup", **res}))


if __name__ == "__main__":
    main()
