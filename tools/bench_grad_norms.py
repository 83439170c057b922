"""Cost of the per-head gradient-norm diagnostics on the GPU (grad_norms.GradNormCollector): prints ONE JSON line.

Works on ViT-B's flat gradient buffer (flat.FlatSpace's layout of ``vit_base_patch16_224``) with random contents; no model is run
and no weight reaches the GPU.  Three figures over the same buffer, each the mean of --iters back-to-back calls between two device
events, the three alternated over --rounds rounds (best round reported, every round listed):

* collect_ms    one ``GradNormCollector.collect`` with a device coefficient (tad_grad_segnorm: reduce + finish launch);
* sumsq_ms      ``K.sumsq`` over the whole buffer: the existing one-pass yardstick (one read of the buffer);
* reference_ms  the reference's form, one ``.norm().item()`` per slot on the same views (794 of them for ViT-B; --ref-iters calls).

GB/s = 4 bytes per float of the buffer (collect: of the segments, padding and untouched tensors are not read) over the time.

usage: python tools/bench_grad_norms.py [--iters 1000] [--ref-iters 5] [--rounds 3] [--model vit_base_patch16_224]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simple_tad_amd as T  # noqa: E402
from simple_tad_amd import grad_norms as GN  # noqa: E402
from simple_tad_amd import kernels as K  # noqa: E402
from simple_tad_amd.flat import FlatSpace  # noqa: E402


class _Layout:
    """the offsets of a FlatSpace over the CPU model, with the gradient buffer alone on the GPU"""

    def __init__(self, space, flat_grad):
        self.offset, self.flat_grad = space.offset, flat_grad

    def __contains__(self, p):
        return id(p) in self.offset


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--ref-iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--model", default="vit_base_patch16_224")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_grad_norms needs a GPU"
    model = T.create_model(args.model, pretrained=False, num_classes=2, all_frames=16, tubelet_size=2)
    space = FlatSpace([p for p in model.parameters() if p.requires_grad])
    g = torch.Generator(device="cuda").manual_seed(0)
    flat = torch.randn(space.total, device="cuda", generator=g)
    col = GN.GradNormCollector(model, _Layout(space, flat))
    coef = torch.full((1,), 0.5, device="cuda")
    acc = torch.zeros(1, device="cuda")
    views = [flat[o:o + n] for o, n, _ in col.layout.segments]
    seg_floats = sum(n for _, n, _ in col.layout.segments)

    def reference():
        return [v.norm().item() for v in views]

    fns = {"collect": (lambda: col.collect(coef), args.iters), "sumsq": (lambda: K.sumsq(flat, acc), args.iters),
           "reference": (reference, args.ref_iters)}
    rounds = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, (fn, iters) in fns.items():
            rounds[k].append(_gpu_ms(fn, iters))
    # the two forms agree (the timed loops computed the same table)
    col.reset()
    col.collect()
    got = col.last_step()
    want = torch.tensor(reference(), dtype=torch.float64)
    mine = torch.cat([torch.from_numpy(got[k]).reshape(-1) for k in GN.KEYS])[[s for _, _, s in col.layout.segments]]
    rel = float(((mine - want).abs() / want).max())
    best = {k: min(v) for k, v in rounds.items()}
    out = {"bench": "grad_norms", "model": args.model, "buffer_floats": space.total, "segment_floats": seg_floats,
           "segments": len(col.layout.segments), "work_items": int(col.work.shape[0]),
           "collect_ms": round(best["collect"], 4), "collect_GBps": round(4.0 * seg_floats / best["collect"] / 1e6, 1),
           "sumsq_ms": round(best["sumsq"], 4), "sumsq_GBps": round(4.0 * space.total / best["sumsq"] / 1e6, 1),
           "reference_ms": round(best["reference"], 3), "collect_over_sumsq": round(best["collect"] / best["sumsq"], 3),
           "reference_over_collect": round(best["reference"] / best["collect"], 1), "max_rel_difference_to_reference": rel,
           "rounds_ms": {k: [round(x, 4) for x in v] for k, v in rounds.items()}, "iters": args.iters, "ref_iters": args.ref_iters}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
