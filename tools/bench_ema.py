"""Weight EMA cost on the GPU (ema.ModelEma): prints ONE JSON line.

* kernel_ms / kernel_GBps: the one launch of an update alone, back to back (12 B per element: read ema, read model, write ema);
  update_ms / effective GB/s: ModelEma.update calls back to back (bounded by host_ms when the walk is slower than the kernel);
  both for the ViT-B and ViT-L states, against the reference's per-tensor torch expression (timm.utils.ModelEma.update);
* host_ms: host time per update() call (state-dict walk + one launch), measured with the GPU queue not in the way;
* engine_loop: clips/s of engine.train_one_epoch for ViT-B at --batch clips (DataParallel + FusedAdamW, as bench.py's engine_loop)
  without and with model_ema, alternating, best of --rounds.

usage: python tools/bench_ema.py [--iters 50] [--steps 10] [--batch 32] [--rounds 2] [--skip-loop]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simple_tad_amd as T  # noqa: E402
from simple_tad_amd import engine as E  # noqa: E402
from simple_tad_amd.ema import ModelEma  # noqa: E402
from simple_tad_amd.parallel import DataParallel  # noqa: E402


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


def state_figures(name, iters):
    m = T.create_model(name, pretrained=False, num_classes=2, all_frames=16, tubelet_size=2).cuda()
    e = ModelEma(m, decay=0.9999)
    nel = sum(v.numel() for v in e.ema.state_dict().values())
    ms = _gpu_ms(lambda: e.update(m), iters)
    plan = next(iter(e._plans.values()))
    kernel_ms = _gpu_ms(lambda: plan.run(0.9999), iters)  # the launch alone, back to back: what the GPU spends per update
    pairs = [(v, m.state_dict()[k]) for k, v in e.ema.state_dict().items()]

    def torch_ref():
        for ev, mv in pairs:
            ev.copy_(ev * 0.9999 + (1. - 0.9999) * mv)
    ref_ms = _gpu_ms(torch_ref, max(3, iters // 5))
    # host time: the GPU side of one update is far shorter than its host side, so the queue never blocks this loop
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        e.update(m)
    host_ms = (time.perf_counter() - t) * 1e3 / iters
    torch.cuda.synchronize()
    out = {"tensors": len(pairs), "elements": nel, "kernel_ms": round(kernel_ms, 4), "kernel_GBps": round(12.0 * nel / kernel_ms / 1e6, 1),
           "update_ms": round(ms, 4), "effective_GBps": round(12.0 * nel / ms / 1e6, 1),
           "torch_reference_ms": round(ref_ms, 4), "torch_reference_GBps": round(12.0 * nel / ref_ms / 1e6, 1),
           "speedup_vs_torch": round(ref_ms / ms, 2), "host_ms": round(host_ms, 4)}
    del e, m, pairs
    torch.cuda.empty_cache()
    return out


def engine_loop(batch, steps, rounds):
    torch.manual_seed(0)
    dev = torch.device("cuda")
    model = T.create_model("vit_base_patch16_224", pretrained=False, num_classes=2, all_frames=16, tubelet_size=2,
                           final_reduction="fc_norm", init_scale=0.001, use_flash_attn=True).to(dev)
    ema = ModelEma(model, decay=0.9999)  # the reference's order: the EMA before the optimizer
    model.train()
    dp = DataParallel(model, bucket_mb=64.0)
    opt = E.create_optimizer(dp, lr=1e-3, weight_decay=0.05, layer_decay=0.75)
    scaler = E.NativeScalerWithGradNormCount(dp)
    crit = torch.nn.CrossEntropyLoss()
    x = torch.randn(batch, 3, 16, 224, 224, device=dev)
    y = torch.randint(0, 2, (batch,), device=dev)
    nel = 2 + steps
    lr = E.cosine_scheduler(1e-4, 1e-6, 1, nel, warmup_epochs=0)

    def run(model_ema):
        t1 = [None]

        def log(epoch, i, stats):
            if i == 1:  # two warm-up iterations
                torch.cuda.synchronize()
                t1[0] = time.perf_counter()
        E.train_one_epoch(dp, crit, [(x, y)] * nel, opt, dev, 0, scaler, lr_schedule_values=lr, num_training_steps_per_epoch=nel, log=log,
                          model_ema=model_ema)
        torch.cuda.synchronize()
        return (time.perf_counter() - t1[0]) / (nel - 2)

    best = {"without": float("inf"), "with": float("inf")}
    for _ in range(rounds):
        best["without"] = min(best["without"], run(None))
        best["with"] = min(best["with"], run(ema))
    out = {k: {"clips_per_s": round(batch / v, 2), "ms_per_step": round(1e3 * v, 3)} for k, v in best.items()}
    out["overhead_pct"] = round(100.0 * (best["with"] / best["without"] - 1.0), 2)
    out.update(batch=batch, steps=steps, rounds=rounds)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--skip-loop", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ema needs a GPU"
    res = {"vit_base_patch16_224": state_figures("vit_base_patch16_224", args.iters),
           "vit_large_patch16_224": state_figures("vit_large_patch16_224", args.iters)}
    if not args.skip_loop:
        res["engine_loop_vit_b"] = engine_loop(args.batch, args.steps, args.rounds)
    print(json.dumps({"bench": "ema_update", **res}))


if __name__ == "__main__":
    main()
