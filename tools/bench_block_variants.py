"""Step time of the layer-scale / proj-MLP-dropout Block variants, fused route (ops.BlockVariantFn) against the composed one: prints ONE
JSON line.

ViT-B/16, 16 x 224 x 224, --batch clips (32): forward + CE loss + backward + fused AdamW (engine.create_optimizer, the headline's step),
drop_path 0.1.  Configurations: init_values = 0.1; drop_rate = 0.1; both; and init_values = 0, drop_rate = 0 (the plain fused block: the
floor, on which the switch has no effect -- its two columns measure the noise of the run).  Every configuration runs with
ops.set_block_variants(False) and (True) ALTERNATED in the same process, --repeats windows of --steps steps each after --warmup steps
per route, the host clock around windows that end in a device synchronise.  Reported per route: the median window (ms per step) and the
spread (max - min over its windows); per configuration: composed / fused of the medians.

usage: python tools/bench_block_variants.py [--batch 32] [--steps 6] [--warmup 3] [--repeats 3] [--precision fast]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simple_tad_amd as T  # noqa: E402
from simple_tad_amd import engine as E  # noqa: E402
from simple_tad_amd import ops  # noqa: E402

CONFIGS = (("plain", 0.0, 0.0), ("layer_scale", 0.1, 0.0), ("dropout", 0.0, 0.1), ("layer_scale+dropout", 0.1, 0.1))


def make_step(name, init_values, drop_rate, batch, dev):
    torch.manual_seed(0)
    model = T.create_model("vit_base_patch16_224", pretrained=False, num_classes=2, all_frames=16, tubelet_size=2,
                           final_reduction="fc_norm", drop_path_rate=0.1, init_scale=0.001, use_flash_attn=True, init_values=init_values,
                           drop_rate=drop_rate).to(dev).train()
    opt = E.create_optimizer(model, lr=1e-3, weight_decay=0.05, layer_decay=0.75)
    scaler = E.NativeScalerWithGradNormCount(model)
    crit = torch.nn.CrossEntropyLoss()
    params = list(model.parameters())
    x = torch.randn(batch, 3, 16, 224, 224, device=dev)
    y = torch.randint(0, 2, (batch,), device=dev)
    opt.zero_grad()

    def step():
        loss = crit(model(x), y)
        scaler(loss, opt, parameters=params)
        opt.zero_grad()
        return loss

    return step


def window(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        last = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return 1e3 * dt, float(last.detach())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--precision", default="fast", choices=("fast", "half"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_block_variants needs a GPU"
    dev = torch.device("cuda:0")
    T.set_precision(args.precision)
    out = {"bench": "block_variants", "model": "vit_base_patch16_224", "batch": args.batch, "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "precision": args.precision, "drop_path": 0.1, "configs": {}}
    for name, iv, dr in CONFIGS:
        step = make_step(name, iv, dr, args.batch, dev)
        ms = {False: [], True: []}
        loss = {}
        calls = {}
        for on in (False, True):  # warm every shape and route the timed windows use
            ops.set_block_variants(on)
            for _ in range(args.warmup):
                step()
        for _ in range(args.repeats):
            for on in (False, True):
                ops.set_block_variants(on)
                n0 = ops.block_variant_calls
                t, l = window(step, args.steps)
                ms[on].append(t)
                loss[on] = l
                calls[on] = ops.block_variant_calls - n0
        ops.set_block_variants(True)
        med = {on: statistics.median(v) for on, v in ms.items()}
        out["configs"][name] = {
            "init_values": iv, "drop_rate": dr,
            "composed_ms": round(med[False], 3), "fused_ms": round(med[True], 3),
            "composed_spread_ms": round(max(ms[False]) - min(ms[False]), 3), "fused_spread_ms": round(max(ms[True]) - min(ms[True]), 3),
            "composed_over_fused": round(med[False] / med[True], 4),
            "windows_ms": {"composed": [round(v, 3) for v in ms[False]], "fused": [round(v, 3) for v in ms[True]]},
            "variant_calls_per_window": {"composed": calls[False], "fused": calls[True]},
            "last_loss": {"composed": loss[False], "fused": loss[True]}}
        del step
        ops.invalidate_weight_cache()
        torch.cuda.empty_cache()
    plain = out["configs"]["plain"]["fused_ms"]
    for name in ("layer_scale", "dropout", "layer_scale+dropout"):
        out["configs"][name]["fused_over_plain"] = round(out["configs"][name]["fused_ms"] / plain, 4)
    T.set_precision("fast")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
