"""A/B of the InternVideo2 serving kernels (csrc/iv2_serve.hip) on the scoring path: internvideo2_small_patch14_224, 8 x 224 x 224, fast
mode, evaluation under no_grad, with ops.set_iv2_serve_kernels(True) -- the class-token entry as one kernel pass and the blocks as one
loop of fused residual + RMSNorm launches -- and (False) -- torch ``cat`` + add and the per-block module route, the code before the
switch existed.  Three legs:

  store    --batch windows (32) per forward from a frame_store.FrameStore (what inference.score_video runs)
  sliding  inference.SlidingWindow at batch 1, eager and HIP-graph replay (a push of one frame + a prediction per step)
  float    the float-clip evaluation forward at batch 1 and at --batch

Writes profiles/iv2_serve.json and prints ONE JSON line.  No ratio is promised: what is measured is written down.

One process, one model; per leg the two settings are interleaved window by window (A B B A A B ...), so both see the same drift of the
machine.  A window is --steps forwards between two device synchronisations, timed on the host clock; per setting the median over
--windows windows and their spread (max - min), and the calls of the wrappers concerned in one further forward.  ``keeps_default``: the
fused loop stays the default for a leg if its median is not above the switch-off median by more than the larger of the two spreads.

usage: python tools/bench_iv2_serve.py [--batch 32] [--steps 10] [--windows 7] [--warmup 3] [--out profiles/iv2_serve.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WRAPPERS = ("class_token_entry_fwd", "residual_rmsnorm", "rmsnorm_fwd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iv2_serve.json"))
    args = ap.parse_args()
    import torch
    import simple_tad_amd as T
    from simple_tad_amd import FrameStore, kernels as K, ops
    from simple_tad_amd.inference import SlidingWindow
    assert torch.cuda.is_available(), "bench_iv2_serve needs a GPU"
    dev = torch.device("cuda:0")
    T.set_precision("fast")
    torch.manual_seed(0)
    model = T.create_model("internvideo2_small_patch14_224", num_classes=2).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    nf = args.batch + 7
    frames = torch.randint(0, 256, (nf, 224, 224, 3), generator=g, dtype=torch.uint8)
    store = FrameStore(nf, 224, 224, dev)
    store.append(frames)
    fw = store.windows([[s + t for t in range(8)] for s in range(args.batch)])
    x1 = torch.randn(1, 3, 8, 224, 224, device=dev)
    xb = torch.randn(args.batch, 3, 8, 224, 224, device=dev)

    def make_sliding(use_graph):
        """per setting its own SlidingWindow, filled once (a graph is captured under the setting that first meets its ring offset)"""
        objs = {}

        def step(on):
            sw = objs.get(on)
            if sw is None:
                sw = objs[on] = SlidingWindow(model, device=dev, use_graph=use_graph)
                for i in range(8):
                    sw.push(frames[i])
            sw.push(frames[step.n % nf])
            step.n += 1
            return sw.predict()
        step.n = 8
        return step

    def no_grad(f):
        def step(on):
            with torch.no_grad():
                return f()
        return step

    legs = {
        "store_b%d" % args.batch: no_grad(lambda: model(fw)),
        "sliding_eager_b1": make_sliding(False),
        "sliding_graph_b1": make_sliding(True),
        "float_b1": no_grad(lambda: model(x1)),
        "float_b%d" % args.batch: no_grad(lambda: model(xb)),
    }

    def window(step, on):
        ops.set_iv2_serve_kernels(on)
        step(on)  # (the setting's first forward is not timed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            last = step(on)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps, last

    out = {"bench": "iv2_serve", "model": "internvideo2_small_patch14_224", "clip": [8, 224, 224], "tokens": 8 * 16 * 16 + 1, "batch": args.batch,
           "precision": "fast", "steps": args.steps, "windows": args.windows, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "legs": {}}
    for name, step in legs.items():
        for on in (True, False):
            ops.set_iv2_serve_kernels(on)
            for _ in range(max(args.warmup, 9) if "sliding" in name else args.warmup):  # (a lap of the ring: every offset's graph is captured)
                step(on)
        torch.cuda.synchronize()
        runs, last = {True: [], False: []}, {}
        for w in range(args.windows):
            for on in ((True, False) if w % 2 == 0 else (False, True)):
                ms, last[on] = window(step, on)
                runs[on].append(ms)
                print(f"{name} window {w} serve_kernels={on}: {ms:.3f} ms", file=sys.stderr)
        calls = {}
        for on in (True, False):
            ops.set_iv2_serve_kernels(on)
            counts, orig = {k: 0 for k in WRAPPERS}, {k: getattr(K, k) for k in WRAPPERS}
            for k, f in orig.items():
                def rec(*a, _k=k, _f=f, **kw):
                    counts[_k] += 1
                    return _f(*a, **kw)
                setattr(K, k, rec)
            try:
                if "graph" not in name:  # (a replayed graph calls no wrapper)
                    step(on)
                torch.cuda.synchronize()
            finally:
                for k, f in orig.items():
                    setattr(K, k, f)
            calls[on] = counts
        leg = {}
        for on, key in ((True, "fused"), (False, "module_route")):
            ms = runs[on]
            leg[key] = {"ms": round(statistics.median(ms), 4), "spread_ms": round(max(ms) - min(ms), 4), "windows_ms": [round(v, 4) for v in ms],
                        "wrapper_calls": calls[on]}
        a, b = leg["fused"], leg["module_route"]
        leg["module_route_over_fused"] = round(b["ms"] / a["ms"], 4)
        leg["keeps_default"] = bool(a["ms"] <= b["ms"] + max(a["spread_ms"], b["spread_ms"]))
        leg["logits_equal"] = bool(torch.equal(last[True], last[False])) if "sliding" not in name else None  # (sliding: the two objects hold different windows)
        out["legs"][name] = leg
    ops.set_iv2_serve_kernels(True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
