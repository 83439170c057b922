"""Evaluation metrics of the frame-level fine-tuning engine.

``calculate_metrics`` mirrors engine_for_frame_finetuning.calculate_metrics (:593-636): same inputs ([n,2] logits, [n] labels),
same return tuple.  Everything thresholded (accuracy / precision / recall / F1 / confusion matrix at 0.5, the 101-threshold MCC /
precision / recall / accuracy / F1 curves of anaysis/metrics.calculate_MORE_metrics :127-208, and the *binned* AUROC / AP / ROC / PR
of torchmetrics with ``thresholds=THRESHOLDS``) derives from ONE pass of a HIP kernel over the predictions
(``tad_threshold_histogram``: exact integer counts); the exact (sort-based) AUROC / AP that the published tables use
(anaysis/metrics.py:52-54, scikit-learn definitions) run as a device sort + prefix sums.  No CPU path for the counting.

torchmetrics is neither vendored nor version-pinned by the reference (INSTALL.md:27); the binned curves restate its published
algorithm (``_binary_precision_recall_curve_update/_compute``, ``_binary_roc_compute``, ``_auc_compute_without_check``):
parity for those is pinned only against this package's own oracle restatement, not against torchmetrics itself.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import check

THRESHOLDS = np.arange(0.00, 1.001, 0.01).tolist()  # anaysis/metrics.py:16


def threshold_confusion(probs: torch.Tensor, labels: torch.Tensor, thresholds=THRESHOLDS) -> np.ndarray:
    """int64 [T,2,2]: confmat[t][label][pred] with pred = (p >= thresholds[t]) compared in float32 (as numpy / torch compare a
    float32 array with Python-float thresholds)."""
    if not probs.is_cuda:
        raise _lib.TadError("threshold_confusion: predictions must be on the GPU (the counting runs as a HIP kernel; no CPU path)")
    p = probs.detach().reshape(-1).float().contiguous()
    y = labels.detach().reshape(-1).to(device=p.device, dtype=torch.int32).contiguous()
    if p.numel() != y.numel() or p.numel() == 0:
        raise _lib.TadError("threshold_confusion: predictions and labels must be non-empty and of equal length")
    thr = torch.tensor(thresholds, dtype=torch.float32, device=p.device)
    if thr.numel() > 1 and not bool((thr[1:] >= thr[:-1]).all()):
        raise _lib.TadError("threshold_confusion: thresholds must be ascending")
    T = thr.numel()
    hist = torch.empty((2, T + 1), dtype=torch.int64, device=p.device)
    check(_lib.load().tad_threshold_histogram(p.data_ptr(), y.data_ptr(), thr.data_ptr(), T, p.numel(), hist.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "tad_threshold_histogram")
    h = hist.cpu().numpy()
    total = h.sum(axis=1, keepdims=True)                       # samples per label
    below = np.cumsum(h, axis=1)[:, :T]                        # k <= i  -> predicted negative at threshold i
    cm = np.zeros((T, 2, 2), dtype=np.int64)
    cm[:, 0, 0], cm[:, 0, 1] = below[0], total[0] - below[0]   # TN, FP
    cm[:, 1, 0], cm[:, 1, 1] = below[1], total[1] - below[1]   # FN, TP
    return cm


def _safe_div(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.divide(a, b, out=np.zeros_like(a), where=b != 0)


def thresholded_scores(cm: np.ndarray):
    """per-threshold (mcc, precision, recall, accuracy, f1) with scikit-learn's definitions and zero_division=0
    (anaysis/metrics.py:190-204)"""
    tn, fp, fn, tp = (cm[:, 0, 0].astype(np.float64), cm[:, 0, 1].astype(np.float64), cm[:, 1, 0].astype(np.float64),
                      cm[:, 1, 1].astype(np.float64))
    mcc = _safe_div(tp * tn - fp * fn, np.sqrt((tp + fp) * (tp + fn) * (tn + fp) * (tn + fn)))
    return mcc, _safe_div(tp, tp + fp), _safe_div(tp, tp + fn), _safe_div(tp + tn, tp + tn + fp + fn), _safe_div(2 * tp, 2 * tp + fp + fn)


def trapezoid(x, y) -> float:
    """sklearn.metrics.auc for monotonic x"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return float(np.sum((x[1:] - x[:-1]) * (y[1:] + y[:-1]) / 2.0))


def binned_curves(cm: np.ndarray, thresholds=THRESHOLDS):
    """torchmetrics' binned ROC / PR curves and their areas from the per-threshold confusion matrices (see module docstring)"""
    thr = np.asarray(thresholds, dtype=np.float32)
    tn, fp, fn, tp = cm[:, 0, 0], cm[:, 0, 1], cm[:, 1, 0], cm[:, 1, 1]
    tpr, fpr = _safe_div(tp, tp + fn)[::-1], _safe_div(fp, fp + tn)[::-1]
    auroc = trapezoid(fpr, tpr)
    precision = np.concatenate([_safe_div(tp, tp + fp), [1.0]])
    recall = np.concatenate([_safe_div(tp, tp + fn), [0.0]])
    ap = float(-np.sum((recall[1:] - recall[:-1]) * precision[:-1]))
    return auroc, ap, (precision, recall, thr), (fpr, tpr, thr[::-1].copy())


def exact_auroc_ap(probs: torch.Tensor, labels: torch.Tensor):
    """scikit-learn's roc_auc_score / average_precision_score (distinct-score thresholds, ties grouped) on the device"""
    p = probs.detach().reshape(-1).float()
    y = labels.detach().reshape(-1).to(p.device).double()
    order = torch.argsort(p, descending=True, stable=True)
    ps, ys = p[order], y[order]
    last = torch.ones_like(ps, dtype=torch.bool)
    last[:-1] = ps[1:] != ps[:-1]                                # last element of every run of equal scores
    tps = torch.cumsum(ys, 0)[last]
    fps = torch.cumsum(1.0 - ys, 0)[last]
    n_pos, n_neg = tps[-1], fps[-1]
    if float(n_pos) == 0 or float(n_neg) == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    z = torch.zeros(1, dtype=tps.dtype, device=tps.device)
    tpr, fpr = torch.cat([z, tps]) / n_pos, torch.cat([z, fps]) / n_neg
    auroc = torch.sum((fpr[1:] - fpr[:-1]) * (tpr[1:] + tpr[:-1]) / 2.0)
    precision, recall = tps / (tps + fps), tps / n_pos
    ap = torch.sum((recall - torch.cat([z, recall[:-1]])) * precision)
    return float(auroc), float(ap)


def calculate_more_metrics(probs: torch.Tensor, labels: torch.Tensor):
    """anaysis/metrics.calculate_MORE_metrics (:127-208) without the two sklearn curve objects: returns
    (acc, precision, recall, f1, ap, auroc, confmat, mcc[T], precision[T], recall[T], acc[T], f1[T]).
    NOTE the 4th value: the reference's threshold loop re-uses the name ``f1_val`` (:199 overwrites :173), so what it returns as
    "F1 at 0.5" is the F1 at the LAST threshold (1.0).  Reproduced as is; the real F1 at 0.5 is ``f1[T][50]``."""
    cm = threshold_confusion(probs, labels)
    mcc, pr, rc, acc, f1 = thresholded_scores(cm)
    i5 = THRESHOLDS.index(0.5)
    auroc, ap = exact_auroc_ap(probs, labels)
    return (acc[i5], pr[i5], rc[i5], f1[-1], ap, auroc, cm[i5].tolist(), mcc.tolist(), pr.tolist(), rc.tolist(), acc.tolist(), f1.tolist())


def calculate_metrics(preds: torch.Tensor, labels: torch.Tensor, do_softmax: bool = True):
    """engine_for_frame_finetuning.calculate_metrics (:593-636): returns
    (acc, recall, precision, f1, confmat, auroc, ap, pr_curve, roc_curve, (mcc_auc, mcc_max, mcc_max_threshold, mcc_05));
    accuracy / recall / precision / F1 / confusion matrix use the arg-max class (``torch.max(preds, 1)``), the curves the class-1
    probability binned at THRESHOLDS."""
    if do_softmax:
        preds = torch.nn.functional.softmax(preds, dim=1)
    values = preds[:, 1].contiguous()
    hard = torch.max(preds, 1)[1]
    y = labels.to(preds.device)
    tp = int(((hard == 1) & (y == 1)).sum()); fp = int(((hard == 1) & (y == 0)).sum())
    fn = int(((hard == 0) & (y == 1)).sum()); tn = int(((hard == 0) & (y == 0)).sum())
    acc = float(_safe_div(tp + tn, tp + tn + fp + fn)); recall = float(_safe_div(tp, tp + fn)); precision = float(_safe_div(tp, tp + fp))
    f1 = float(_safe_div(2 * tp, 2 * tp + fp + fn))
    confmat = [[tn, fp], [fn, tp]]
    cm = threshold_confusion(values, y)
    auroc, ap, pr_curve, roc_curve = binned_curves(cm)
    mcc = thresholded_scores(cm)[0].tolist()
    mcc_max = max(mcc)
    return (acc, recall, precision, f1, confmat, auroc, ap, pr_curve, roc_curve,
            (trapezoid(THRESHOLDS, mcc), mcc_max, THRESHOLDS[mcc.index(mcc_max)], mcc[THRESHOLDS.index(0.5)]))


# ---------------------------------------------------------------------------------------------- grouped evaluation report
# anaysis/metrics_dota.py, metrics_dada.py and metrics_by_categories.py score up to 30 subsets of the test frames (TOTAL, the accident
# categories, ego / non-ego, their intersections, night / day), each with 101 x matthews_corrcoef + roc_auc_score on the host.  Here a
# sample carries a bit mask of the groups it belongs to, and all groups share ONE histogram launch (csrc/group_metrics.hip:
# tad_group_threshold_histogram) and ONE device sort followed by one scan launch (tad_group_rank_stats).
DOTA_CAT_CODES = ["ST", "AH", "LA", "OC", "TC", "VP", "VO", "OO", "UK"]  # anaysis/metrics_dota.py:15
GROUP_MAX = _lib.GROUP_MAX
GROUP_RANK_TILE = _lib.GROUP_RANK_TILE  # samples per scan tile of tad_group_rank_stats (tests place run boundaries around it)
_RULE, _DASH = "=" * 59, "-" * 59


def pack_groups(groups, n: int, device=None):
    """``groups``: mapping name -> bool mask of length n (numpy array or tensor, on either device).  Returns ``(names, member)``:
    the names in the mapping's order and an int64 tensor [n] on ``device`` (default: the GPU) whose bit g, read as uint64, says that
    the sample belongs to ``names[g]`` (group 63 is the sign bit).  At most 64 groups."""
    names = list(groups)
    if not 1 <= len(names) <= GROUP_MAX:
        raise _lib.TadError(f"pack_groups: {len(names)} groups, need 1..{GROUP_MAX}")
    device = torch.device("cuda" if device is None else device)
    member = torch.zeros(int(n), dtype=torch.int64, device=device)
    for g, name in enumerate(names):
        mask = torch.as_tensor(groups[name]).reshape(-1)
        if mask.numel() != n:
            raise _lib.TadError(f"pack_groups: the mask of group {name!r} has {mask.numel()} entries, expected {n}")
        bit = (1 << g) if g < 63 else -(1 << 63)
        member |= torch.where(mask.to(device=device, dtype=torch.bool), bit, 0)
    return names, member


def _group_operands(what, probs, labels, member, n_groups):
    if not probs.is_cuda:
        raise _lib.TadError(f"{what}: predictions must be on the GPU (the counting runs as a HIP kernel; no CPU path)")
    p = probs.detach().reshape(-1).float().contiguous()
    y = labels.detach().reshape(-1).to(device=p.device, dtype=torch.int32).contiguous()
    m = member.detach().reshape(-1).to(device=p.device).contiguous()
    if m.dtype != torch.int64 or not (p.numel() == y.numel() == m.numel()) or p.numel() == 0:
        raise _lib.TadError(f"{what}: predictions, labels and the int64 membership masks must be non-empty and of equal length")
    if not 1 <= int(n_groups) <= GROUP_MAX:
        raise _lib.TadError(f"{what}: n_groups={n_groups}, need 1..{GROUP_MAX}")
    return p, y, m


def _device_operands(what, *operands):
    """the launches take raw pointers: every operand a contiguous GPU tensor of the stated dtype and length"""
    for t, dtype, numel in operands:
        if not (t.is_cuda and t.dtype == dtype and t.numel() == numel and t.is_contiguous()):
            raise _lib.TadError(f"{what}: expected a contiguous GPU tensor of {numel} x {dtype}, got {tuple(t.shape)} {t.dtype} on {t.device}")


def group_threshold_histogram(p, y, member, n_groups, thr, out=None):
    """the launch: f32 ``p``, int32 ``y``, int64 ``member``, f32 ``thr`` [T] on one GPU -> int64 [G,2,T+1] on it (``out`` if given)"""
    G, T = int(n_groups), thr.numel()
    hist = torch.empty((G, 2, T + 1), dtype=torch.int64, device=p.device) if out is None else out
    _device_operands("group_threshold_histogram", (p, torch.float32, p.numel()), (y, torch.int32, p.numel()), (member, torch.int64, p.numel()),
                     (thr, torch.float32, T), (hist, torch.int64, G * 2 * (T + 1)))
    check(_lib.load().tad_group_threshold_histogram(p.data_ptr(), y.data_ptr(), member.data_ptr(), G, thr.data_ptr(), T, p.numel(),
                                                    hist.data_ptr(), torch.cuda.current_stream().cuda_stream), "tad_group_threshold_histogram")
    return hist


def grouped_confusion(probs, labels, member, n_groups, thresholds=THRESHOLDS) -> np.ndarray:
    """int64 [G,T,2,2]: ``threshold_confusion`` of every group's members (``member`` from ``pack_groups``), one launch"""
    p, y, m = _group_operands("grouped_confusion", probs, labels, member, n_groups)
    thr = torch.tensor(thresholds, dtype=torch.float32, device=p.device)
    if thr.numel() > 1 and not bool((thr[1:] >= thr[:-1]).all()):
        raise _lib.TadError("grouped_confusion: thresholds must be ascending")
    T = thr.numel()
    h = group_threshold_histogram(p, y, m, n_groups, thr).cpu().numpy()
    total = h.sum(axis=2, keepdims=True)                       # [G,2,1] samples per label
    below = np.cumsum(h, axis=2)[:, :, :T]                     # k <= i  -> predicted negative at threshold i
    cm = np.zeros((int(n_groups), T, 2, 2), dtype=np.int64)
    cm[:, :, 0, 0], cm[:, :, 0, 1] = below[:, 0], total[:, 0] - below[:, 0]   # TN, FP
    cm[:, :, 1, 0], cm[:, :, 1, 1] = below[:, 1], total[:, 1] - below[:, 1]   # FN, TP
    return cm


def group_rank_stats(labels_sorted, member_sorted, run_end, n_groups, out_int=None, out_ap=None):
    """the launch: int32 labels and int64 masks in descending score order, uint8 run-end flags -> (int64 [G,3] = P, N, U2; f64 [G] = AP)"""
    G, n = int(n_groups), labels_sorted.numel()
    out_int = torch.empty((G, 3), dtype=torch.int64, device=labels_sorted.device) if out_int is None else out_int
    out_ap = torch.empty((G,), dtype=torch.float64, device=labels_sorted.device) if out_ap is None else out_ap
    _device_operands("group_rank_stats", (labels_sorted, torch.int32, n), (member_sorted, torch.int64, n), (run_end, torch.uint8, n),
                     (out_int, torch.int64, G * 3), (out_ap, torch.float64, G))
    check(_lib.load().tad_group_rank_stats(labels_sorted.data_ptr(), member_sorted.data_ptr(), run_end.data_ptr(), G, n, out_int.data_ptr(),
                                           out_ap.data_ptr(), torch.cuda.current_stream().cuda_stream), "tad_group_rank_stats")
    return out_int, out_ap


def auroc_from_counts(n_pos: int, n_neg: int, u2: int) -> float:
    """U2 / (2 P N), one correctly rounded division of integers; a single-class group gives the reference's codes (anaysis/metrics.py:
    56-62: -10 = only normal frames, -11 = only abnormal ones), an empty group NaN"""
    if n_pos == 0 or n_neg == 0:
        return float("nan") if n_pos == n_neg else (-11.0 if n_neg == 0 else -10.0)
    return int(u2) / (2 * int(n_pos) * int(n_neg))


def grouped_auroc_ap(probs, labels, member, n_groups):
    """scikit-learn's roc_auc_score / average_precision_score of every group: one device sort, one gather of labels and masks into
    that order, one ``tad_group_rank_stats`` launch.  Returns numpy ``(auroc[G], ap[G], n_pos[G], n_neg[G])``; see
    ``auroc_from_counts`` for single-class and empty groups (their AP: 0 without positives, as scikit-learn).  Non-finite
    predictions raise ValueError, as scikit-learn does."""
    p, y, m = _group_operands("grouped_auroc_ap", probs, labels, member, n_groups)
    if not bool(torch.isfinite(p).all()):
        raise ValueError("grouped_auroc_ap: predictions contain NaN or infinity")
    order = torch.argsort(p, descending=True, stable=True)
    ps = p[order]
    run_end = torch.ones(p.numel(), dtype=torch.uint8, device=p.device)
    run_end[:-1] = ps[1:] != ps[:-1]                             # f32 comparison: -0.0 and 0.0 tie
    out_int, out_ap = group_rank_stats(y[order].contiguous(), m[order].contiguous(), run_end, n_groups)
    oi, ap = out_int.cpu().numpy(), out_ap.cpu().numpy()
    auroc = np.array([auroc_from_counts(int(P), int(N), int(U)) for P, N, U in oi], dtype=np.float64)
    return auroc, ap, oi[:, 0].copy(), oi[:, 1].copy()


def _grouped_tuples(probs, labels, names, member):
    cm = grouped_confusion(probs, labels, member, len(names))
    auroc, ap, _, _ = grouped_auroc_ap(probs, labels, member, len(names))
    i5 = THRESHOLDS.index(0.5)
    out = {}
    for g, name in enumerate(names):
        mcc, pr, rc, acc, f1 = thresholded_scores(cm[g])
        out[name] = (acc[i5], pr[i5], rc[i5], f1[-1], float(ap[g]), float(auroc[g]), cm[g, i5].tolist(), mcc.tolist(), pr.tolist(),
                     rc.tolist(), acc.tolist(), f1.tolist())
    return out, cm


def grouped_more_metrics(probs, labels, groups):
    """``calculate_more_metrics`` of every group of ``groups`` (name -> bool mask): dict name -> the same 12-tuple, the reference's
    "F1 of the last threshold" slot included.  Where the reference raises (a group with one class only) the AUROC slot holds the
    code of ``auroc_from_counts``."""
    n = probs.numel()
    names, member = pack_groups(groups, n, probs.device)
    return _grouped_tuples(probs, labels, names, member)[0]


def _clip_index(clip_ids, device):
    """per-frame clip ids (integers or names) -> (int64 tensor on the device of dense clip numbers, number of clips)"""
    if isinstance(clip_ids, torch.Tensor):
        _, inv = torch.unique(clip_ids.reshape(-1).to(device), return_inverse=True)
    else:
        _, inv = np.unique(np.asarray(clip_ids).reshape(-1), return_inverse=True)
        inv = torch.from_numpy(inv.astype(np.int64)).to(device)
    return inv, int(inv.max()) + 1 if inv.numel() else 0


def _mask(v, device):
    return torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).reshape(-1).to(device) != 0


def _clip_counts(clip, n_clips, masks):
    """number of distinct clips among the frames of every mask (device ops, one copy back)"""
    lens = []
    for mk in masks:
        seen = torch.zeros(n_clips, dtype=torch.int32, device=clip.device).index_add_(0, clip, mk.to(torch.int32))
        lens.append((seen > 0).sum())
    return torch.stack(lens).cpu().tolist()


def _report_line(n_clips, t):
    mcc = t[7]
    auroc = f"{100 * t[5]:.1f}" if t[5] >= 0 else f"{t[5]:.0f}"  # a single-class group: the -10 / -11 code itself; empty: nan
    return f"\tlen: {n_clips} | auroc: {auroc} | aucmcc: {100 * trapezoid(THRESHOLDS, mcc):.1f} | mcc05: {100 * mcc[THRESHOLDS.index(0.5)]:.1f}"


def _report(probs, labels, clip_ids, groups):
    clip, n_clips = _clip_index(clip_ids, probs.device)
    tuples = grouped_more_metrics(probs, labels, groups)
    lens = _clip_counts(clip, n_clips, list(groups.values()))
    return {name: _report_line(k, tuples[name]) for name, k in zip(groups, lens)}


def group_report(probs, labels, clip_ids, *, clip_lvl_cat, clip_lvl_ego, cat_codes=DOTA_CAT_CODES):
    """The lines anaysis/metrics_dota.show_metrics (:111-181) writes into group_metrics.txt from the first ``=====`` line on (the header
    lines about files and missing values are omitted): TOTAL, every category, GROUP EGO and GROUP NON-EGO each with its categories --
    31 groups for DoTA -- as ``len: <distinct clips> | auroc | aucmcc | mcc05`` in percent with one decimal.
    Per frame: ``probs`` (class-1 probability, on the GPU), ``labels``, ``clip_ids`` (integers or names), ``clip_lvl_cat`` (the
    category code of the frame's clip, or its index in ``cat_codes``), ``clip_lvl_ego`` (bool).
    A group with one class only makes the reference raise (roc_auc_score); here its auroc field prints the code -10 (only normal
    frames) or -11 (only abnormal ones) of anaysis/metrics.calculate_metrics, unscaled, and an empty group prints nan."""
    dev = probs.device
    cat = np.asarray(clip_lvl_cat.cpu() if isinstance(clip_lvl_cat, torch.Tensor) else clip_lvl_cat).reshape(-1)
    if cat.dtype.kind in "iu":
        cat_idx = cat.astype(np.int64)
    else:
        lookup = {c: k for k, c in enumerate(cat_codes)}
        if not set(cat.tolist()) <= set(lookup):
            raise _lib.TadError(f"group_report: categories {sorted(set(cat.tolist()) - set(lookup))} are not in cat_codes")
        cat_idx = np.array([lookup[c] for c in cat.tolist()], dtype=np.int64)
    cat_idx = torch.from_numpy(cat_idx).to(dev)
    ego = _mask(clip_lvl_ego, dev)
    groups = {"TOTAL": torch.ones_like(ego)}
    for k, c in enumerate(cat_codes):
        groups[f"cat/{c}"] = cat_idx == k
    for tag, sel in (("ego", ego), ("nonego", ~ego)):
        groups[tag] = sel
        for k, c in enumerate(cat_codes):
            groups[f"{tag}/{c}"] = sel & (cat_idx == k)
    line = _report(probs, labels, clip_ids, groups)
    out = [_RULE, "  General", _DASH, "TOTAL", line["TOTAL"], _RULE, "  General by categories", _DASH]
    for c in cat_codes:
        out += [f"category {c}", line[f"cat/{c}"]]
    for tag, title, head in (("ego", "  EGO by categories", "GROUP EGO"), ("nonego", "  NON-EGO by categories", "GROUP NON-EGO")):
        out += [_RULE, title, _DASH, head, line[tag], _DASH]
        for c in cat_codes:
            out += [f"category {c}", line[f"{tag}/{c}"]]
    return out


def group_report_dada(probs, labels, clip_ids, *, ego):
    """The lines of anaysis/metrics_dada.show_metrics (:108-135) from the first ``=====`` line on: TOTAL, GROUP EGO = every frame of
    the clips that have at least one ego frame (``ego``: per-frame flags), GROUP NON-EGO = the frames of all other clips.
    Single-class and empty groups print as in ``group_report``."""
    clip, n_clips = _clip_index(clip_ids, probs.device)
    ego = _mask(ego, probs.device)
    ego_clip = torch.zeros(n_clips, dtype=torch.int32, device=clip.device).index_add_(0, clip, ego.to(torch.int32)) > 0
    in_ego = ego_clip[clip]
    line = _report(probs, labels, clip, {"TOTAL": torch.ones_like(ego), "ego": in_ego, "nonego": ~in_ego})
    return [_RULE, "  General", _DASH, "TOTAL", line["TOTAL"], _DASH, "GROUP EGO", line["ego"], _DASH, "GROUP NON-EGO", line["nonego"], _DASH]


def group_stats_tables(probs, labels, *, cat, ego, night):
    """The rows of the two tables anaysis/metrics_by_categories.save_metrics (:73-122) writes, from per-frame ``cat`` (integer
    category, 0 = normal driving), ``ego`` and ``night`` flags.  Returns ``(group_rows, thresh_rows)``:
    group_rows (group_stats.csv)   [name, acc, p, r, f1, map, auc] for ego, noego, night, day (the first six values of
                                   ``calculate_more_metrics``; f1 is the reference's last-threshold F1);
    thresh_rows (thresh_stats.csv) [name] + mcc[101] + p[101] + r[101] + acc[101] + f1[101] for all_samples, cat_<k> (ascending k),
                                   ego, noego, night, day.  A cat_<k> row carries ``calculate_fn_group_thresholds`` in the recall slot
                                   (the share of its frames predicted negative at every threshold; 1 - that for k != 0), -1 elsewhere.
    At most 59 categories (64 groups in one pass).  Single-class groups: see ``grouped_more_metrics``."""
    dev = probs.device
    cat = torch.as_tensor(np.asarray(cat) if not isinstance(cat, torch.Tensor) else cat).reshape(-1).to(dev).long()
    ego, night = _mask(ego, dev), _mask(night, dev)
    cats = sorted(int(c) for c in torch.unique(cat).cpu().tolist())
    groups = {"all_samples": torch.ones_like(ego)}
    for k in cats:
        groups[f"cat_{k}"] = cat == k
    groups.update({"ego": ego, "noego": ~ego, "night": night, "day": ~night})
    names, member = pack_groups(groups, probs.numel(), dev)
    tuples, cm = _grouped_tuples(probs, labels, names, member)
    empty = [-1 for _ in THRESHOLDS]
    group_rows = [[name] + list(tuples[name][:6]) for name in ("ego", "noego", "night", "day")]
    thresh_rows = []
    for g, name in enumerate(names):
        if name.startswith("cat_"):
            res = (cm[g, :, 0, 0] + cm[g, :, 1, 0]) / cm[g, 0].sum()    # anaysis/metrics.calculate_fn_group_thresholds (:95-124)
            res = res if name == "cat_0" else 1. - res
            thresh_rows.append([name] + empty + empty + list(res) + empty + empty)
        else:
            t = tuples[name]
            thresh_rows.append([name] + t[7] + t[8] + t[9] + t[10] + t[11])
    return group_rows, thresh_rows
