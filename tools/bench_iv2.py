"""A/B of the two InternVideo2 norm kernels inside the training step: internvideo2_small_patch14_224, 8 x 224 x 224, --batch clips (16),
fast mode, forward + CE loss + backward + fused AdamW (engine.create_optimizer with layer decay), with ops.set_iv2_kernels(True) -- RMSNorm
and the q / k normalisation through csrc/rmsnorm.hip -- and (False) -- the same two norms as torch expressions, everything else
unchanged.  Writes profiles/iv2.json and prints ONE JSON line.  No ratio is promised: what is measured is written down.

One process, one model, one optimizer; the two settings are interleaved window by window (A B B A A B ...), so both see the same drift
of the machine.  A window is --steps steps between two device synchronisations, timed on the host clock; per setting the median over
--windows windows, their spread, the peak memory over its windows, and the launches of the four norm wrappers in one further step.

usage: python tools/bench_iv2.py [--batch 16] [--steps 10] [--windows 7] [--warmup 5] [--out profiles/iv2.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NORM_WRAPPERS = ("rmsnorm_fwd", "rmsnorm_bwd", "qk_rmsnorm_fwd", "qk_rmsnorm_bwd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iv2.json"))
    args = ap.parse_args()
    import torch
    import simple_tad_amd as T
    from simple_tad_amd import engine as E, kernels as K, ops
    assert torch.cuda.is_available(), "bench_iv2 needs a GPU"
    dev = torch.device("cuda:0")
    T.set_precision("fast")
    torch.manual_seed(0)
    model = T.create_model("internvideo2_small_patch14_224", num_classes=2, drop_path_rate=0.1).to(dev).train()
    opt = E.create_optimizer(model, lr=1e-3, weight_decay=0.05, layer_decay=0.75)
    scaler = E.NativeScalerWithGradNormCount(model)
    crit = torch.nn.CrossEntropyLoss()
    params = [p for p in model.parameters() if p.requires_grad]
    x = torch.randn(args.batch, 3, 8, 224, 224, device=dev)
    y = torch.randint(0, 2, (args.batch,), device=dev)
    opt.zero_grad()

    def step():
        loss = crit(model(x), y)
        scaler(loss, opt, parameters=params)
        opt.zero_grad()
        return loss

    def window(on):
        ops.set_iv2_kernels(on)
        step()  # (the setting's first step is not timed)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            last = step()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps, torch.cuda.max_memory_allocated(), float(last.detach())

    for on in (True, False):
        ops.set_iv2_kernels(on)
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    runs = {True: [], False: []}
    for w in range(args.windows):
        for on in ((True, False) if w % 2 == 0 else (False, True)):
            runs[on].append(window(on))
            print(f"window {w} kernels={on}: {runs[on][-1][0]:.2f} ms", file=sys.stderr)
    launches = {}
    for on in (True, False):
        ops.set_iv2_kernels(on)
        counts, orig = {k: 0 for k in NORM_WRAPPERS}, {k: getattr(K, k) for k in NORM_WRAPPERS}
        for k, f in orig.items():
            def rec(*a, _k=k, _f=f, **kw):
                counts[_k] += 1
                return _f(*a, **kw)
            setattr(K, k, rec)
        try:
            step()
            torch.cuda.synchronize()
        finally:
            for k, f in orig.items():
                setattr(K, k, f)
        launches[on] = counts
    ops.set_iv2_kernels(True)
    out = {"bench": "iv2", "model": "internvideo2_small_patch14_224", "clip": [8, 224, 224], "tokens": 8 * 16 * 16 + 1, "batch": args.batch,
           "precision": "fast", "steps": args.steps, "windows": args.windows, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "settings": {}}
    for on, name in ((True, "kernels"), (False, "torch_norms")):
        ms = [r[0] for r in runs[on]]
        out["settings"][name] = {"ms": round(statistics.median(ms), 3), "spread_ms": round(max(ms) - min(ms), 3), "windows_ms": [round(v, 3) for v in ms],
                                 "peak_MB": round(max(r[1] for r in runs[on]) / 1e6, 1), "last_loss": runs[on][-1][2], "norm_wrapper_calls": launches[on]}
    a, b = out["settings"]["kernels"]["ms"], out["settings"]["torch_norms"]["ms"]
    out["torch_norms_over_kernels"] = round(b / a, 4)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
