#!/usr/bin/env python3
"""Generate ``tests/golden/g24_group_metrics.npz`` and ``tests/golden/g24_group_metrics.txt``: the grouped evaluation report of the
reference on the synthetic annotation table of ``tests/group_metrics_recipe.annotations`` (6000 frames, 120 clips, 9 categories, ego
and night flags; scores from ``golden_recipe.eval_probs_labels``).

``anaysis/metrics.py`` of the reference (numpy + scikit-learn) is imported at run time and called as it is.  ``anaysis/metrics_dota.py``,
``metrics_dada.py`` and ``metrics_by_categories.py`` cannot be imported here (they import natsort, and anaysis.make_plots is not in the
checkout), so this tool calls the same scikit-learn functions in the same order on the same subsets and cites the lines; the pandas
row selections become numpy masks.  Per group ``<key>`` of ``group_metrics_recipe.golden_groups``:

  <key>.more      calculate_MORE_metrics' acc, precision, recall, f1 (of the LAST threshold), ap, auroc
  <key>.confmat   its confusion matrix at 0.5;  <key>.cm  the counts at all 101 thresholds [T,2,2] (numpy, float32 comparison)
  <key>.mcc / .precision / .recall / .acc / .f1   its five 101-vectors
  <key>.show      roc_auc_score, auc(THRESHOLDS, mcc), mcc at 0.5 as metrics_dota.get_mcc_metrics returns them;  <key>.len  distinct clips
  <key>.pnu       P, N and U2 = 2 x (positive, negative) pairs ranked right + tied pairs, counted with integer searches
and ``cat.<k>`` = calculate_fn_group_thresholds of the frames of category k (1 - that for k != 0), ``group_rows`` the group_stats.csv
rows (ego, noego, night, day x acc, p, r, f1, map, auc).  The text file holds the report lines of show_metrics, DoTA then DADA form.
The fixtures hold numbers and report text only.

usage: python tools/make_goldens_group_metrics.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_goldens as MG  # noqa: E402  (REF, save; it puts tests/ on sys.path)
import group_metrics_recipe as GR  # noqa: E402

sys.path.insert(0, MG.REF)
from anaysis import metrics as am  # noqa: E402
from sklearn.metrics import auc, matthews_corrcoef, roc_auc_score  # noqa: E402


def get_mcc_metrics(labels, probs):
    """metrics_dota.get_mcc_metrics (:18-33)"""
    mcc_t_vals = [matthews_corrcoef(labels, (probs >= t).astype(int)) for t in am.THRESHOLDS]
    return auc(am.THRESHOLDS, mcc_t_vals), mcc_t_vals[am.THRESHOLDS.index(0.5)]


def show_line(a, mask):
    """one group of show_metrics (metrics_dota.py:115-119 and its repetitions): the line and its three values"""
    labels, probs = a["labels"][mask], a["probs"][mask]
    clips = set(a["clip"][mask].tolist())
    auroc = roc_auc_score(labels, probs)
    mcc_auc, mcc_05 = get_mcc_metrics(labels, probs)
    return f"\tlen: {len(clips)} | auroc: {100*auroc:.1f} | aucmcc: {100*mcc_auc:.1f} | mcc05: {100*mcc_05:.1f}", (auroc, mcc_auc, mcc_05), len(clips)


def counts(probs, labels, thr):
    cm = np.zeros((len(thr), 2, 2), dtype=np.int64)
    for i, t in enumerate(thr):
        pred = (probs >= t).astype(np.int64)
        np.add.at(cm[i], (labels, pred), 1)
    return cm


def pair_count(probs, labels):
    pos, neg = probs[labels == 1], np.sort(probs[labels == 0])
    less, leq = np.searchsorted(neg, pos, side="left"), np.searchsorted(neg, pos, side="right")
    return len(pos), len(neg), int(2 * less.sum() + (leq - less).sum())


def main():
    a = GR.annotations()
    probs, labels = a["probs"], a["labels"]
    assert probs.dtype == np.float32 and len(probs) == GR.N_FRAMES and len(set(a["clip"].tolist())) == GR.N_CLIPS
    assert am.THRESHOLDS == GR.THRESHOLDS
    arrs, lines = {}, {}
    for key, mask in GR.golden_groups(a).items():
        p, y = probs[mask], labels[mask]
        assert 0 < y.sum() < len(y), f"group {key} must keep both classes"
        (acc, precision, recall, f1, ap, auroc, confmat, _, _, mcc, p_t, r_t, acc_t, f1_t) = am.calculate_MORE_metrics(p, y)
        cm = counts(p, y, [np.float32(t) for t in am.THRESHOLDS])
        # the fixture must not depend on NumPy's promotion of a Python float against a float32 array
        assert np.array_equal(cm, counts(p, y, am.THRESHOLDS)) and np.array_equal(cm[GR.I5], np.array(confmat))
        lines[key], show, n_clips = show_line(a, mask)
        P, N, u2 = pair_count(p, y)
        assert abs(u2 / (2 * P * N) - auroc) < 1e-12 and show[0] == auroc
        arrs.update({f"{key}.more": np.array([acc, precision, recall, f1, ap, auroc]), f"{key}.confmat": np.array(confmat), f"{key}.cm": cm,
                     f"{key}.mcc": np.array(mcc), f"{key}.precision": np.array(p_t), f"{key}.recall": np.array(r_t),
                     f"{key}.acc": np.array(acc_t), f"{key}.f1": np.array(f1_t), f"{key}.show": np.array(show),
                     f"{key}.len": np.array(n_clips), f"{key}.pnu": np.array([P, N, u2], dtype=np.int64)})
    # metrics_by_categories.save_metrics (:86-92): the per-category rows, and (:94-122) the group_stats rows
    for k in sorted(set(a["cat"].tolist())):
        sel = a["cat"] == k
        res = np.array(am.calculate_fn_group_thresholds(probs=probs[sel], labels=labels[sel]))
        arrs[f"cat.{k}"] = res if k == 0 else 1. - res
    arrs["group_rows"] = np.stack([arrs[f"stats.{k}.more"] for k in ("ego", "noego", "night", "day")])
    arrs["all_samples.thresh"] = np.concatenate([np.array(v) for v in am.calculate_MORE_metrics(preds=probs, labels=labels)[-5:]])
    MG.save("g24_group_metrics", **arrs)
    dota = GR.dota_lines(a, {k[5:]: v for k, v in lines.items() if k.startswith("dota.")})
    dada = GR.dada_lines(a, {"TOTAL": lines["dota.TOTAL"], "ego": lines["dada.ego"], "nonego": lines["dada.nonego"]})
    path = os.path.join(ROOT, "tests", "golden", "g24_group_metrics.txt")
    with open(path, "w") as f:
        f.write("\n".join(["# dota"] + dota + ["# dada"] + dada) + "\n")
    print("wrote", path, os.path.getsize(path), "bytes;", len(arrs), "arrays")


if __name__ == "__main__":
    main()
