"""Cost of the frame fine-tuning losses on the GPU (loss.FocalLoss / FocalLoss2 / DoubleBCELoss / SmoothAPLoss /
TemporalExponentialLoss): prints ONE JSON line.

Per ``--loss`` name of run_frame_finetuning.py, at [--batch, 2] f32 logits (56 = the batch of the reference's job scripts), forward +
backward of the criterion through the HIP route (``tad_frame_loss``) and through the reference's own expression run eagerly on the same
device (restated here: FocalLoss2 with its per-call ``torch.tensor(alpha, device=...)``, SmoothAPLoss with its sort and its Python loop
over the positives), the two alternating round by round in one process, best round of each:

* ``gpu_ms``: device time per call, HIP events around --iters calls queued back to back;
* ``host_ms``: host time per call over the same loop (both routes are launch-bound at this size, so this is what a step pays);
* ``launches``: kernels launched by one forward + backward, counted by torch.profiler (null where it is not available).

usage: python tools/bench_frame_loss.py [--iters 50] [--rounds 3] [--batch 56]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from simple_tad_amd import loss as L  # noqa: E402


def reference_expression(name):
    """the reference's class of a --loss name as an eager torch function (criterion arguments as the HIP route's)"""
    crit = L.build_criterion(name)
    if name in ("focal", "focal6x100"):
        def fn(z, y):
            ce = F.cross_entropy(z, y, reduction="none")
            return torch.mean(crit.multiplier * crit.alpha * ((1 - torch.exp(-ce)) ** crit.gamma) * ce)
    elif name in ("focal2_6", "focal2_2"):
        def fn(z, y):
            ce = F.cross_entropy(z, y, reduction="none")
            pt = torch.exp(-ce)
            ce = torch.tensor(crit.alpha, dtype=z.dtype, device=z.device)[y] * ce
            return torch.mean(((1 - pt) ** crit.gamma) * ce * crit.multiplier)
    elif name == "2bce":
        bce = torch.nn.BCEWithLogitsLoss(reduction="none")

        def fn(z, s):
            return (bce(z[:, 0], s[:, 0]) + bce(z[:, 1], s[:, 1])).mean()
    elif name == "smoothap":
        def fn(z, y):
            p = F.softmax(z, dim=1)[:, 1]
            pos, neg = p[y == 1], torch.sort(p[y == 0])[0]
            loss = 0.0
            for pp in pos:
                loss += torch.sum(torch.relu(neg - pp + crit.delta))
            return loss / (pos.shape[0] if pos.shape[0] > 0 else 1.0)
    else:
        def fn(z, y, t):
            base = F.cross_entropy(z, y, reduction="none")
            w = torch.ones_like(y, dtype=torch.float)
            w[t < 0] = torch.exp(crit.alpha_pre * t[t < 0])
            w[t > 0] = torch.exp(-crit.alpha_post * t[t > 0])
            return (base * torch.clamp(w, max=1.0)).mean()
    return crit, fn


def _times(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = time.perf_counter()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    host = (time.perf_counter() - t) * 1e3 / iters
    b.synchronize()
    return a.elapsed_time(b) / iters, host


def _launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception as e:  # noqa: BLE001  (a build without the profiler: the times are still worth having)
        print(f"launch count unavailable: {e}", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=56)
    ap.add_argument("--no-launch-count", action="store_true")
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    z = (2.0 * torch.randn(a.batch, 2, device="cuda", generator=g)).requires_grad_()
    y = torch.randint(0, 2, (a.batch,), device="cuda", generator=g)
    anomaly = torch.sigmoid(2.0 * torch.randn(a.batch, device="cuda", generator=g))
    soft = torch.stack((1 - anomaly, anomaly), dim=-1)
    ttc = torch.randn(a.batch, device="cuda", generator=g, dtype=torch.float64)       # float64, as compute_time_vector delivers it
    out = {"batch": a.batch, "classes": 2, "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    for name in L.LOSS_NAMES:
        if name == "crossentropy":
            continue
        crit, ref = reference_expression(name)
        args_hip = (soft,) if name == "2bce" else (y, ttc) if name == "exponential1" else (y,)
        args_ref = (soft,) if name == "2bce" else (y, ttc.float()) if name == "exponential1" else (y,)   # (the class needs f32 there)

        def step(fn, args):
            z.grad = None
            fn(z, *args).backward()

        variants = {"hip": lambda: step(crit, args_hip), "torch": lambda: step(ref, args_ref)}
        best = {k: [float("inf"), float("inf")] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                gpu, host = _times(fn, a.iters)
                best[k] = [min(best[k][0], gpu), min(best[k][1], host)]
        row = {}
        for k, fn in variants.items():
            row[k] = {"gpu_ms": round(best[k][0], 4), "host_ms": round(best[k][1], 4),
                      "launches": None if a.no_launch_count else _launches(fn)}
        out[name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
