"""Numpy restatement of the grouped evaluation report (simple_tad_amd.metrics: pack_groups .. group_stats_tables), and the seeded
annotation table golden G24 is generated from (tools/make_goldens_group_metrics.py runs scikit-learn and the reference's
anaysis/metrics.py on the same table).  Used by tests/test_group_metrics_cpu.py and tests/test_group_metrics_gpu.py."""
import numpy as np

import golden_recipe as R

THRESHOLDS = np.arange(0.00, 1.001, 0.01).tolist()
THR32 = np.asarray(THRESHOLDS, dtype=np.float32)
I5 = THRESHOLDS.index(0.5)
CAT_CODES = ["ST", "AH", "LA", "OC", "TC", "VP", "VO", "OO", "UK"]
RULE, DASH = "=" * 59, "-" * 59
N_FRAMES, N_CLIPS = 6000, 120


def annotations():
    """The synthetic table of G24: 6000 frames in 120 clips of 50; clip c has category c % 9 and is an ego clip when (c // 9) is even
    (every category x ego cell holds 6 or 7 clips); night clips are c % 4 == 1.  Per frame: the ``ego`` flag is set in the second
    half of ego clips whose number is not a multiple of 3 (so the DADA rule "a clip with any ego frame" differs from the clip-level
    flag), ``cat`` is 0 on normal frames and the clip's category + 1 on abnormal ones.  Scores: golden_recipe.eval_probs_labels."""
    probs, labels = R.eval_probs_labels("g24", N_FRAMES)
    clip = np.repeat(np.arange(N_CLIPS), N_FRAMES // N_CLIPS)
    pos = np.tile(np.arange(N_FRAMES // N_CLIPS), N_CLIPS)
    clip_lvl_cat = clip % 9
    clip_lvl_ego = (clip // 9) % 2 == 0
    ego = clip_lvl_ego & (clip % 3 != 0) & (pos >= 25)
    night = clip % 4 == 1
    cat = np.where(labels == 1, clip_lvl_cat + 1, 0)
    return dict(probs=probs, labels=labels.astype(np.int64), clip=clip, clip_lvl_cat=clip_lvl_cat, clip_lvl_ego=clip_lvl_ego, ego=ego,
                night=night, cat=cat)


def dota_groups(a):
    """name -> mask of the 31 groups of anaysis/metrics_dota.show_metrics, in its order"""
    g = {"TOTAL": np.ones(len(a["labels"]), dtype=bool)}
    for k, c in enumerate(CAT_CODES):
        g[f"cat/{c}"] = a["clip_lvl_cat"] == k
    for tag, sel in (("ego", a["clip_lvl_ego"]), ("nonego", ~a["clip_lvl_ego"])):
        g[tag] = sel
        for k, c in enumerate(CAT_CODES):
            g[f"{tag}/{c}"] = sel & (a["clip_lvl_cat"] == k)
    return g


def dada_groups(a):
    ego_clips = np.unique(a["clip"][a["ego"]])
    in_ego = np.isin(a["clip"], ego_clips)
    return {"TOTAL": np.ones(len(a["labels"]), dtype=bool), "ego": in_ego, "nonego": ~in_ego}


def stats_groups(a):
    g = {"all_samples": np.ones(len(a["labels"]), dtype=bool)}
    for k in sorted(set(a["cat"].tolist())):
        g[f"cat_{k}"] = a["cat"] == k
    g.update({"ego": a["ego"], "noego": ~a["ego"], "night": a["night"], "day": ~a["night"]})
    return g


def golden_groups(a):
    """every group G24 holds, under the key the fixture uses"""
    out = {f"dota.{k}": v for k, v in dota_groups(a).items()}
    out.update({f"dada.{k}": v for k, v in dada_groups(a).items() if k != "TOTAL"})
    out.update({f"stats.{k}": v for k, v in stats_groups(a).items() if not k.startswith("cat_") and k != "all_samples"})
    return out


def pack(masks):
    """list of bool masks -> uint64 [n], bit g = masks[g]"""
    member = np.zeros(len(masks[0]), dtype=np.uint64)
    for g, m in enumerate(masks):
        member |= np.asarray(m, dtype=bool).astype(np.uint64) << np.uint64(g)
    return member


def in_group(member, g):
    return ((member >> np.uint64(g)) & np.uint64(1)).astype(bool)


def group_hist(probs, labels, member, n_groups, thr):
    """int64 [G,2,T+1]: per group and label the histogram of k(p) = #{t : p >= thr[t]} (float32 comparison; NaN: k = 0)"""
    probs, thr = np.asarray(probs, dtype=np.float32), np.asarray(thr, dtype=np.float32)
    k = np.zeros(len(probs), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for t in thr:
            k += probs >= t
    row = len(thr) + 1
    slot = (np.asarray(labels) != 0).astype(np.int64) * row + k
    hist = np.zeros((n_groups, 2, row), dtype=np.int64)
    for g in range(n_groups):
        hist[g] = np.bincount(slot[in_group(member, g)], minlength=2 * row).reshape(2, row)
    return hist


def confusion_from_hist(hist):
    """int64 [G,T,2,2], confmat[g][t][label][pred]"""
    T = hist.shape[2] - 1
    total = hist.sum(axis=2, keepdims=True)
    below = np.cumsum(hist, axis=2)[:, :, :T]
    cm = np.zeros((hist.shape[0], T, 2, 2), dtype=np.int64)
    cm[:, :, 0, 0], cm[:, :, 0, 1] = below[:, 0], total[:, 0] - below[:, 0]
    cm[:, :, 1, 0], cm[:, :, 1, 1] = below[:, 1], total[:, 1] - below[:, 1]
    return cm


def sort_order(probs):
    """(stable descending order, run_end flags of the sorted array); float32 comparison, so -0.0 and 0.0 tie"""
    probs = np.asarray(probs, dtype=np.float32)
    order = np.argsort(-probs, kind="stable")
    ps = probs[order]
    run_end = np.ones(len(ps), dtype=bool)
    run_end[:-1] = ps[1:] != ps[:-1]
    return order, run_end


def rank_stats_sorted(labels_sorted, member_sorted, run_end, n_groups):
    """per group (P, N, U2 as Python ints) and the fp64 AP, from the sorted arrays: cumulative positives T / negatives F of the group
    at the run ends e of the WHOLE array, U2 = sum (F_e - F_s)(T_e + T_s), AP = sum (T_e - T_s) / P * T_e / (T_e + F_e)"""
    lab = np.asarray(labels_sorted) != 0
    ints, aps = [], []
    for g in range(n_groups):
        sel = in_group(member_sorted, g)
        Te = np.cumsum(sel & lab)[run_end].astype(np.int64)
        Fe = np.cumsum(sel & ~lab)[run_end].astype(np.int64)
        Ts, Fs = np.concatenate([[0], Te[:-1]]), np.concatenate([[0], Fe[:-1]])
        P, N = (int(Te[-1]), int(Fe[-1])) if len(Te) else (0, 0)
        u2 = sum(int(v) for v in (Fe - Fs) * (Te + Ts))
        live = Te > Ts
        ap = float(np.sum((Te[live] - Ts[live]) / P * (Te[live] / (Te[live] + Fe[live])))) if P else 0.0
        ints.append((P, N, u2))
        aps.append(ap)
    return ints, aps


def rank_stats(probs, labels, member, n_groups):
    order, run_end = sort_order(probs)
    return rank_stats_sorted(np.asarray(labels)[order], member[order], run_end, n_groups), int(run_end.sum())


def auroc_from_counts(P, N, u2):
    if P == 0 or N == 0:
        return float("nan") if P == N else (-11.0 if N == 0 else -10.0)
    return u2 / (2 * P * N)


def thresholded(cm):
    """(mcc, precision, recall, acc, f1), each [T], scikit-learn's definitions with zero_division=0"""
    tn, fp, fn, tp = (cm[:, i, j].astype(np.float64) for i, j in ((0, 0), (0, 1), (1, 0), (1, 1)))

    def div(a, b):
        return np.divide(a, b, out=np.zeros_like(a), where=b != 0)
    return (div(tp * tn - fp * fn, np.sqrt((tp + fp) * (tp + fn) * (tn + fp) * (tn + fn))), div(tp, tp + fp), div(tp, tp + fn),
            div(tp + tn, tp + tn + fp + fn), div(2 * tp, 2 * tp + fp + fn))


def trapezoid(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return float(np.sum((x[1:] - x[:-1]) * (y[1:] + y[:-1]) / 2.0))


def more_metrics(probs, labels, groups):
    """name -> dict(cm [T,2,2], P, N, U2, auroc, ap, mcc, precision, recall, acc, f1, mcc_auc, at05 = the reference's first four values)"""
    names = list(groups)
    member = pack([groups[k] for k in names])
    cm = confusion_from_hist(group_hist(probs, labels, member, len(names), THR32))
    (ints, aps), _ = rank_stats(probs, labels, member, len(names))
    out = {}
    for g, name in enumerate(names):
        mcc, pr, rc, acc, f1 = thresholded(cm[g])
        P, N, u2 = ints[g]
        out[name] = dict(cm=cm[g], P=P, N=N, U2=u2, auroc=auroc_from_counts(P, N, u2), ap=aps[g], mcc=mcc, precision=pr, recall=rc, acc=acc,
                         f1=f1, mcc_auc=trapezoid(THRESHOLDS, mcc), at05=np.array([acc[I5], pr[I5], rc[I5], f1[-1]]))
    return out


def n_clips(clip, mask):
    return len(np.unique(np.asarray(clip)[mask]))


def report_line(k, m):
    auroc = f"{100 * m['auroc']:.1f}" if m["auroc"] >= 0 else f"{m['auroc']:.0f}"
    return f"\tlen: {k} | auroc: {auroc} | aucmcc: {100 * m['mcc_auc']:.1f} | mcc05: {100 * m['mcc'][I5]:.1f}"


def dota_lines(a, line):
    """the layout of anaysis/metrics_dota.show_metrics (:111-181); ``line``: group name -> its "len: ..." line"""
    out = [RULE, "  General", DASH, "TOTAL", line["TOTAL"], RULE, "  General by categories", DASH]
    for c in CAT_CODES:
        out += [f"category {c}", line[f"cat/{c}"]]
    for tag, title, head in (("ego", "  EGO by categories", "GROUP EGO"), ("nonego", "  NON-EGO by categories", "GROUP NON-EGO")):
        out += [RULE, title, DASH, head, line[tag], DASH]
        for c in CAT_CODES:
            out += [f"category {c}", line[f"{tag}/{c}"]]
    return out


def dada_lines(a, line):
    """anaysis/metrics_dada.show_metrics (:108-135)"""
    return [RULE, "  General", DASH, "TOTAL", line["TOTAL"], DASH, "GROUP EGO", line["ego"], DASH, "GROUP NON-EGO", line["nonego"], DASH]


def report(a, groups, layout):
    m = more_metrics(a["probs"], a["labels"], groups)
    return layout(a, {k: report_line(n_clips(a["clip"], groups[k]), m[k]) for k in groups})


def stats_tables(a):
    """(group_rows, thresh_rows) of anaysis/metrics_by_categories.save_metrics (:73-122)"""
    groups = stats_groups(a)
    m = more_metrics(a["probs"], a["labels"], groups)
    empty = [-1 for _ in THRESHOLDS]
    group_rows = [[k] + list(m[k]["at05"]) + [m[k]["ap"], m[k]["auroc"]] for k in ("ego", "noego", "night", "day")]
    thresh_rows = []
    for k in groups:
        if k.startswith("cat_"):
            res = (m[k]["cm"][:, 0, 0] + m[k]["cm"][:, 1, 0]) / m[k]["cm"][0].sum()
            thresh_rows.append([k] + empty + empty + list(res if k == "cat_0" else 1. - res) + empty + empty)
        else:
            thresh_rows.append([k] + [v for key in ("mcc", "precision", "recall", "acc", "f1") for v in m[k][key].tolist()])
    return group_rows, thresh_rows


def read_report(path):
    """the two sections of tests/golden/g24_group_metrics.txt: {"dota": lines, "dada": lines}"""
    out, cur = {}, None
    for ln in open(path).read().split("\n"):
        if ln.startswith("# "):
            cur = out.setdefault(ln[2:], [])
        elif cur is not None:
            cur.append(ln)
    return {k: (v[:-1] if v and v[-1] == "" else v) for k, v in out.items()}
