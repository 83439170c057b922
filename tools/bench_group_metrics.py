"""Cost of one grouped evaluation report on the GPU against the reference's scikit-learn loop on the same arrays, in the same run:
prints ONE JSON line.

The table: --frames frames (default 300 000) in clips of 100, 9 categories, ego / non-ego: the 30 groups of
anaysis/metrics_dota.show_metrics plus a night group = 31 (--groups cuts or repeats them); scores as golden_recipe.eval_probs_labels
makes them (a third on the 0.01 grid: ties).

* report_ms     ``metrics.grouped_more_metrics``, whole call on a host clock (it ends in the copies of the results): packing the
                masks, the histogram launch, the device sort and gathers, the rank-statistics launch, the host arithmetic;
* hist_ms       tad_group_threshold_histogram alone, and
* sort_rank_ms  argsort + run flags + gathers + tad_group_rank_stats (rank_ms: that launch alone), each the mean of --iters calls
                between two device events, best of --rounds rounds;
* sklearn_s     per group 101 x matthews_corrcoef + auc and one roc_auc_score (metrics_dota.get_mcc_metrics, :18-33, :116-117), once.

usage: python tools/bench_group_metrics.py [--frames 300000] [--groups 31] [--iters 20] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import golden_recipe as R  # noqa: E402
from simple_tad_amd import metrics as M  # noqa: E402


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


def table(n, n_groups):
    probs, labels = R.eval_probs_labels("bench_group_metrics", n)
    clip = np.arange(n) // 100
    cat, ego = clip % 9, (clip // 9) % 2 == 0
    groups = {"TOTAL": np.ones(n, dtype=bool)}
    for k in range(9):
        groups[f"cat{k}"] = cat == k
    for tag, sel in (("ego", ego), ("nonego", ~ego)):
        groups[tag] = sel
        for k in range(9):
            groups[f"{tag}/cat{k}"] = sel & (cat == k)
    groups["night"] = clip % 4 == 1
    names = list(groups)
    return probs, labels, {f"{names[g % len(names)]}#{g // len(names)}": groups[names[g % len(names)]] for g in range(n_groups)}


def sklearn_report(probs, labels, groups):
    from sklearn.metrics import auc, matthews_corrcoef, roc_auc_score
    out = {}
    for name, mask in groups.items():
        p, y = probs[mask], labels[mask]
        mcc = [matthews_corrcoef(y, (p >= t).astype(int)) for t in M.THRESHOLDS]
        out[name] = (roc_auc_score(y, p), auc(M.THRESHOLDS, mcc), mcc[M.THRESHOLDS.index(0.5)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300_000)
    ap.add_argument("--groups", type=int, default=31)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_group_metrics needs a GPU"
    probs, labels, groups = table(args.frames, args.groups)
    p, y = torch.from_numpy(probs).cuda(), torch.from_numpy(labels).cuda()
    dev_groups = {k: torch.from_numpy(v).cuda() for k, v in groups.items()}
    G = len(groups)
    _, member = M.pack_groups(dev_groups, args.frames, "cuda")
    y32 = y.int()
    thr = torch.tensor(M.THRESHOLDS, dtype=torch.float32, device="cuda")

    def sort_rank():
        order = torch.argsort(p, descending=True, stable=True)
        ps = p[order]
        run_end = torch.ones(p.numel(), dtype=torch.uint8, device="cuda")
        run_end[:-1] = ps[1:] != ps[:-1]
        return y32[order], member[order], run_end

    ys, ms, re = sort_rank()

    def report():
        t0 = time.perf_counter()
        out = M.grouped_more_metrics(p, y, dev_groups)
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    fns = {"hist": lambda: M.group_threshold_histogram(p, y32, member, G, thr), "rank": lambda: M.group_rank_stats(ys, ms, re, G),
           "sort_rank": lambda: M.group_rank_stats(*sort_rank(), G)}
    report()
    rounds = {k: [] for k in (*fns, "report")}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            rounds[k].append(_gpu_ms(fn, args.iters))
        rounds["report"].append(min(report()[1] for _ in range(args.iters)))
    got = report()[0]
    t0 = time.perf_counter()
    want = sklearn_report(probs, labels, groups)
    sklearn_s = time.perf_counter() - t0
    # the two reports agree (same arrays)
    i5 = M.THRESHOLDS.index(0.5)
    diff = max(max(abs(got[k][5] - want[k][0]), abs(M.trapezoid(M.THRESHOLDS, got[k][7]) - want[k][1]), abs(got[k][7][i5] - want[k][2])) for k in groups)
    best = {k: min(v) for k, v in rounds.items()}
    print(json.dumps({"bench": "group_metrics", "frames": args.frames, "groups": G, "report_ms": round(best["report"], 3),
                      "hist_ms": round(best["hist"], 4), "sort_rank_ms": round(best["sort_rank"], 4), "rank_ms": round(best["rank"], 4),
                      "sklearn_s": round(sklearn_s, 3), "sklearn_over_report": round(sklearn_s * 1e3 / best["report"], 1),
                      "max_abs_difference_to_sklearn": diff, "rounds_ms": {k: [round(x, 4) for x in v] for k, v in rounds.items()},
                      "iters": args.iters}))


if __name__ == "__main__":
    main()
