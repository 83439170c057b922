"""A/B of the visible-token kernels inside the MAE pre-training step: pretrain_videomae_internvideo2_patch14_224, 8 x 224 x 224, --batch
clips (16), tube mask 0.75 (512 of 2048 tokens visible), fast mode, forward + MSE loss against the normalised pixel target + backward
+ fused AdamW, with ops.set_visible_token_kernels(True) -- the encoder's entry through csrc/visible_tokens.hip -- and (False) -- the
same arithmetic as torch expressions (a dense add, the index, and on the way back the index_put into zeros and the dense sum over the
batch), everything else unchanged.  Writes profiles/iv2_pretrain.json and prints ONE JSON line.  No ratio is promised: what is measured
is written down.

The protocol of tools/bench_iv2.py: one process, one model, one optimizer; the two settings are interleaved window by window (A B B A
A B ...), so both see the same drift of the machine.  A window is --steps steps between two device synchronisations, timed on the host
clock; per setting the median over --windows windows, their spread, the peak memory over its windows, and the launches of the two
wrappers in one further step.

usage: python tools/bench_iv2_pretrain.py [--batch 16] [--steps 10] [--windows 7] [--warmup 5] [--out profiles/iv2_pretrain.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WRAPPERS = ("visible_tokens_fwd", "visible_tokens_bwd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iv2_pretrain.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import simple_tad_amd as T
    from simple_tad_amd import engine as E, engine_pretrain as EP, kernels as K, ops
    from simple_tad_amd.masking_generator import TubeMaskingGenerator
    assert torch.cuda.is_available(), "bench_iv2_pretrain needs a GPU"
    dev = torch.device("cuda:0")
    T.set_precision("fast")
    torch.manual_seed(0)
    np.random.seed(0)
    model = T.create_model("pretrain_videomae_internvideo2_patch14_224").to(dev).train()
    opt = E.create_optimizer(model, lr=1e-3, weight_decay=0.05)
    scaler = E.NativeScalerWithGradNormCount(model)
    params = [p for p in model.parameters() if p.requires_grad]
    x = torch.randn(args.batch, 3, 8, 224, 224, device=dev)
    gen = TubeMaskingGenerator((8, 16, 16), 0.75)
    mask = torch.from_numpy(np.stack([gen() for _ in range(args.batch)])).to(dev).flatten(1).to(torch.bool)
    num_masked = int(mask[0].sum())
    opt.zero_grad()

    def step():
        with torch.no_grad():
            labels = EP.reconstruction_target(x, mask, 14, 1, True, num_masked)
        loss = ops.MseLossFn.apply(model(x, mask, num_masked=num_masked), labels)
        scaler(loss, opt, parameters=params)
        opt.zero_grad()
        return loss

    def window(on):
        ops.set_visible_token_kernels(on)
        step()  # (the setting's first step is not timed)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            last = step()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps, torch.cuda.max_memory_allocated(), float(last.detach())

    for on in (True, False):
        ops.set_visible_token_kernels(on)
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
        ops.set_visible_token_kernels(on)
        counts, orig = {k: 0 for k in WRAPPERS}, {k: getattr(K, k) for k in WRAPPERS}
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
    ops.set_visible_token_kernels(True)
    out = {"bench": "iv2_pretrain", "model": "pretrain_videomae_internvideo2_patch14_224", "clip": [8, 224, 224], "tokens": 8 * 16 * 16,
           "visible_tokens": 8 * 16 * 16 - num_masked, "mask_ratio": 0.75, "batch": args.batch, "precision": "fast", "steps": args.steps,
           "windows": args.windows, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "settings": {}}
    for on, name in ((True, "kernels"), (False, "torch_ops")):
        ms = [r[0] for r in runs[on]]
        out["settings"][name] = {"ms": round(statistics.median(ms), 3), "spread_ms": round(max(ms) - min(ms), 3), "windows_ms": [round(v, 3) for v in ms],
                                 "peak_MB": round(max(r[1] for r in runs[on]) / 1e6, 1), "last_loss": runs[on][-1][2], "wrapper_calls": launches[on]}
    a, b = out["settings"]["kernels"]["ms"], out["settings"]["torch_ops"]["ms"]
    out["torch_ops_over_kernels"] = round(b / a, 4)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
