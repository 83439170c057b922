"""What frozen layers save: step time, peak memory and weight-gradient launches of the fine-tuning step with the first N blocks frozen,
this tree against a checkout of its parent commit.  Writes profiles/freeze.json and prints ONE JSON line.

ViT-B/16, 16 x 224 x 224, --batch clips (32), drop_path 0.1: forward + CE loss + backward + fused AdamW (engine.create_optimizer over
the trainable parameters), precisions fast and half, N in {0, 6, 12} of the reference's rule `--freeze_layers "first N blocks;N"`
(run_frame_finetuning.py:465-485).  The parent has no engine.freeze_layers, so the rule is restated here and sets the same flags in
both trees; in the parent they change nothing but what the optimizer holds.

Legs: every leg is a fresh child process (--worker) over ONE tree that measures all six configurations; the legs alternate
parent / this / this / parent / ... for --rounds rounds, so that both trees see the same drift of the machine.  Per configuration a leg
warms --warmup steps, then times --windows windows of --steps steps each (host clock around windows that end in a device
synchronise) and reports the median window; torch.cuda.max_memory_allocated is taken over the timed windows, and one further step
counts the weight-gradient launches (kernels.linear_bwd_weight / _qkv / _pair, layerscale_grads; the pair counts once: it is one launch).
Reported per tree and configuration: the median over the rounds, the spread (max - min over the rounds), peak memory, launches.
The one requirement: at N = 0 this tree lies within twice the parent's round-to-round spread of the parent (an all-trainable model
pays nothing); the exit status is 1 if it does not.

usage: python tools/bench_freeze.py --parent-tree DIR [--rounds 3] [--steps 20] [--windows 3] [--warmup 5] [--batch 32]
       DIR: a checkout of the parent commit with its library built (git worktree add DIR HEAD~1; python DIR/__graft_entry__.py).
       Without --parent-tree only this tree is measured and the N = 0 comparison is reported as not measured.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREEZE = (0, 6, 12)
PRECISIONS = ("fast", "half")
WGRAD = ("linear_bwd_weight", "linear_bwd_weight_qkv", "linear_bwd_weight_pair", "layerscale_grads")


def apply_rule(model, n_blocks):
    """run_frame_finetuning.py:465-485, restated with its substring tests (engine.freeze_layers of this tree is the same rule)"""
    frozen = 0
    for name, param in model.named_parameters():
        if "blocks" in name:
            param.requires_grad = not (int(name.split(".")[1]) < n_blocks and "norm" not in name)
        elif "patch_embed" in name:
            param.requires_grad = False
        else:
            param.requires_grad = True
        frozen += not param.requires_grad
    return frozen


def worker(args):
    sys.path.insert(0, args.tree)
    import torch
    import simple_tad_amd as T
    from simple_tad_amd import engine as E, kernels as K, ops
    assert os.path.dirname(os.path.dirname(os.path.abspath(T.__file__))) == os.path.abspath(args.tree), T.__file__
    assert torch.cuda.is_available(), "bench_freeze needs a GPU"
    dev = torch.device("cuda:0")
    out = {"tree": args.tree, "has_skip_frozen": hasattr(ops, "set_skip_frozen"), "configs": {}}
    for precision in PRECISIONS:
        T.set_precision(precision)
        for n in FREEZE:
            torch.manual_seed(0)
            model = T.create_model("vit_base_patch16_224", pretrained=False, num_classes=2, all_frames=16, tubelet_size=2,
                                   final_reduction="fc_norm", drop_path_rate=0.1, init_scale=0.001, use_flash_attn=True).to(dev).train()
            frozen = apply_rule(model, n) if n else 0  # (N = 0 is the model as built: the patch embedding trains too)
            opt = E.create_optimizer(model, lr=1e-3, weight_decay=0.05, layer_decay=0.75)
            scaler = E.NativeScalerWithGradNormCount(model)
            crit = torch.nn.CrossEntropyLoss()
            params = [p for p in model.parameters() if p.requires_grad]
            x = torch.randn(args.batch, 3, 16, 224, 224, device=dev)
            y = torch.randint(0, 2, (args.batch,), device=dev)
            opt.zero_grad()

            def step():
                loss = crit(model(x), y)
                scaler(loss, opt, parameters=params)
                opt.zero_grad()
                return loss

            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            wins = []
            for _ in range(args.windows):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    last = step()
                torch.cuda.synchronize()
                wins.append(1e3 * (time.perf_counter() - t0) / args.steps)
            peak = torch.cuda.max_memory_allocated()
            counts, orig = {k: 0 for k in WGRAD}, {k: getattr(K, k) for k in WGRAD}
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
            out["configs"][f"{precision}/N{n}"] = {"ms": round(statistics.median(wins), 3), "windows_ms": [round(v, 3) for v in wins],
                                                  "peak_bytes": int(peak), "wgrad_launches": sum(counts.values()), "wgrad_by_wrapper": counts,
                                                  "frozen_tensors": frozen, "last_loss": float(last.detach())}
            del step, model, opt, scaler, params, x, y
            ops.invalidate_weight_cache()
            torch.cuda.empty_cache()
    T.set_precision("fast")
    print(json.dumps(out))


def run_leg(tree, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--tree", os.path.abspath(tree), "--steps", str(args.steps),
           "--windows", str(args.windows), "--warmup", str(args.warmup), "--batch", str(args.batch)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout)
    if r.returncode != 0:  # (a failed leg ends the run: nothing more is started on the device)
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"bench_freeze: the leg over {tree} ended with status {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--leg-timeout", type=int, default=600)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freeze.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    trees = {"this": ROOT}
    if args.parent_tree:
        trees["parent"] = args.parent_tree
    legs = {k: [] for k in trees}
    for r in range(args.rounds):
        order = list(trees) if r % 2 else list(reversed(trees))  # parent, this | this, parent | ...
        for k in order:
            legs[k].append(run_leg(trees[k], args))
            print(f"round {r} {k}: " + "  ".join(f"{c} {v['ms']:.2f}" for c, v in legs[k][-1]["configs"].items()), file=sys.stderr)
    out = {"bench": "freeze", "model": "vit_base_patch16_224", "batch": args.batch, "steps": args.steps, "windows": args.windows,
           "warmup": args.warmup, "rounds": args.rounds, "drop_path": 0.1, "rule": "first N blocks;N", "trees": {}}
    for k, runs in legs.items():
        out["trees"][k] = {}
        for c in runs[0]["configs"]:
            ms = [run["configs"][c]["ms"] for run in runs]
            one = runs[-1]["configs"][c]
            out["trees"][k][c] = {"ms": round(statistics.median(ms), 3), "spread_ms": round(max(ms) - min(ms), 3), "rounds_ms": ms,
                                  "peak_MB": round(max(run["configs"][c]["peak_bytes"] for run in runs) / 1e6, 1),
                                  "wgrad_launches": one["wgrad_launches"], "wgrad_by_wrapper": one["wgrad_by_wrapper"],
                                  "frozen_tensors": one["frozen_tensors"]}
    ok = None
    if "parent" in legs:
        ok = True
        out["n0_check"] = {}
        for p in PRECISIONS:
            a, b = out["trees"]["this"][f"{p}/N0"], out["trees"]["parent"][f"{p}/N0"]
            within = abs(a["ms"] - b["ms"]) <= 2.0 * b["spread_ms"]
            out["n0_check"][p] = {"this_ms": a["ms"], "parent_ms": b["ms"], "parent_spread_ms": b["spread_ms"], "within_2x_spread": within}
            ok = ok and within
    else:
        out["n0_check"] = "not measured (no --parent-tree)"
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0 if ok in (None, True) else 1


if __name__ == "__main__":
    sys.exit(main())
