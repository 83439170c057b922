"""Grouped evaluation report on the GPU: tad_group_threshold_histogram and tad_group_rank_stats against the numpy recipe
(tests/group_metrics_recipe.py) at the sizes where a histogram or a scan can go wrong, the report functions against golden G24
(scikit-learn and the reference's anaysis/metrics.py), consistency with calculate_more_metrics on host-sliced subsets, guard bands,
and final_test's group_metrics.txt."""
import os

import numpy as np
import pytest
import torch

import group_metrics_recipe as GR
from guarded import GuardedArena, same_bits

pytestmark = pytest.mark.gpu

GOLDEN_TXT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g24_group_metrics.txt")
EPS = 2.0 ** -52


def M():
    from simple_tad_amd import metrics
    return metrics


TILE = 4096


def test_tile_constant():
    assert M().GROUP_RANK_TILE == TILE


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def member_tensor(member_u64):
    return cuda(member_u64.view(np.int64))


# ------------------------------------------------------------------------------------------------ 1. histogram
def hist_case(n, G, seed):
    """probabilities with a third on the 0.01 grid, the values 0.29 / 0.57 / 0.0 / 1.0 exactly on thresholds and a NaN; masks with
    samples in no group and in all groups, bits 0 and G - 1 in use, and (G > 2) one empty group"""
    rng = np.random.RandomState(seed)
    probs = rng.rand(n).astype(np.float32)
    grid = rng.rand(n) < 0.33
    probs[grid] = (np.round(probs[grid] * 100) / 100).astype(np.float32)
    special = np.array([0.29, 0.57, 0.0, 1.0, np.nan, 0.5], dtype=np.float32)
    k = min(n, len(special))
    probs[:k] = special[:k]
    labels = (rng.rand(n) < 0.3).astype(np.int32)
    member = rng.randint(0, 1 << 32, n).astype(np.uint64) << np.uint64(32) | rng.randint(0, 1 << 32, n).astype(np.uint64)
    allbits = np.uint64((1 << G) - 1)
    member &= allbits
    idx = np.arange(n)
    member[idx % 7 == 3] = 0
    member[idx % 7 == 5] = allbits
    member[idx % 7 == 6] |= np.uint64(1) | np.uint64(1 << (G - 1))
    if G > 2:
        member &= ~np.uint64(1 << (G // 2))
    return probs, labels, member


HIST_CASES = [(1, 1, 101), (1, 64, 1), (255, 2, 1), (255, 33, 255), (257, 1, 255), (257, 33, 101), (257, 64, 1), (4099, 2, 101),
              (4099, 64, 255), ((1 << 20) + 3, 33, 101), ((1 << 20) + 3, 64, 1), ((1 << 20) + 3, 2, 255)]


@pytest.mark.parametrize("n,G,T", HIST_CASES)
def test_group_histogram_equals_recipe(n, G, T):
    probs, labels, member = hist_case(n, G, n + G + T)
    thr = GR.THR32 if T == 101 else np.linspace(0.0, 1.0, T, dtype=np.float32) if T > 1 else np.array([0.29], dtype=np.float32)
    got = M().group_threshold_histogram(cuda(probs), cuda(labels), member_tensor(member), G, cuda(thr))
    want = GR.group_hist(probs, labels, member, G, thr)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    if G > 2:
        assert int(got[G // 2].sum()) == 0                                           # the empty group
    if G == 64 and n > 7:
        assert int(got[0].sum()) > 0 and int(got[63].sum()) > 0                      # bits 0 and 63
    cm = M().grouped_confusion(cuda(probs), cuda(labels), member_tensor(member), G, thr.tolist())
    assert cm.shape == (G, T, 2, 2) and np.array_equal(cm, GR.confusion_from_hist(want))


@pytest.mark.parametrize("n", [1, 257, 4099, (1 << 20) + 3])
def test_one_group_of_everything_is_threshold_confusion(n):
    probs, labels, _ = hist_case(n, 1, n)
    p, y = cuda(probs), cuda(labels)
    ones = torch.ones(n, dtype=torch.int64, device="cuda")
    cm = M().grouped_confusion(p, y, ones, 1)
    assert cm.shape == (1, 101, 2, 2) and np.array_equal(cm[0], M().threshold_confusion(p, y))
    # the raw tables, bit for bit
    from simple_tad_amd import _lib
    thr = cuda(GR.THR32)
    h1 = torch.empty((2, 102), dtype=torch.int64, device="cuda")
    _lib.check(_lib.load().tad_threshold_histogram(p.data_ptr(), y.data_ptr(), thr.data_ptr(), 101, n, h1.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream))
    assert torch.equal(M().group_threshold_histogram(p, y, ones, 1, thr)[0], h1)


# ------------------------------------------------------------------------------------------------ 2. rank statistics
def rank_masks(n, labels, rng, G=6):
    """everything, a random half, a sparse 3 % (most runs hold no member), positives only, negatives only, nobody; G = 64 repeats
    them over all bits"""
    base = [np.ones(n, dtype=bool), rng.rand(n) < 0.5, rng.rand(n) < 0.03, labels == 1, labels == 0, np.zeros(n, dtype=bool)]
    return [base[g % 6] if g < 6 or g % 6 else (rng.rand(n) < 0.5) for g in range(G)]


def scores(pattern, n, rng):
    if pattern == "continuous":
        return rng.rand(n).astype(np.float32)
    if pattern == "equal":                       # one run spanning every tile
        return np.full(n, 0.37, dtype=np.float32)
    if pattern == "levels4":
        return (rng.randint(0, 4, n) / 4).astype(np.float32)
    if pattern == "signed_zero":                 # -0.0 and 0.0 tie (f32 comparison), below a few positive scores
        s = np.where(rng.rand(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        s[rng.rand(n) < 0.2] = 0.5
        return s
    if pattern == "long_run":                    # distinct scores but for ONE run, ranks TILE - 10 .. 2 TILE + 9: it starts in tile 0, ends in tile 2
        order = rng.permutation(n)               # order[k]: the sample of rank k
        s = np.empty(n, dtype=np.float32)
        s[order] = np.linspace(3.0, 2.0, n, dtype=np.float32)
        s[order[TILE - 10:2 * TILE + 10]] = s[order[TILE - 10]]
        return s
    raise ValueError(pattern)


def check_rank(probs, labels, masks):
    G, n = len(masks), len(probs)
    member = GR.pack(masks)
    p, y, m = cuda(probs), cuda(labels.astype(np.int64)), member_tensor(member)
    auroc, ap, n_pos, n_neg = M().grouped_auroc_ap(p, y, m, G)
    (ints, aps), runs = GR.rank_stats(probs, labels, member, G)
    # the integers straight from the launch
    order, run_end = GR.sort_order(probs)
    out_int, out_ap = M().group_rank_stats(cuda(labels[order].astype(np.int32)), member_tensor(member[order]), cuda(run_end.astype(np.uint8)), G)
    oi = out_int.cpu().numpy()
    for g in range(G):
        P, N, u2 = ints[g]
        assert (int(n_pos[g]), int(n_neg[g])) == (P, N) == (int(masks[g][labels == 1].sum()), int(masks[g][labels == 0].sum())), g
        assert oi[g].tolist() == [P, N, u2], (g, oi[g].tolist(), ints[g])                      # U2 exact
        want = GR.auroc_from_counts(P, N, u2)
        assert auroc[g] == want or (np.isnan(want) and np.isnan(auroc[g])), (g, auroc[g], want)   # bit for bit
        assert abs(ap[g] - aps[g]) <= (runs + 4) * EPS, (g, ap[g], aps[g], runs)
    assert np.array_equal(out_ap.cpu().numpy().view(np.int64), ap.view(np.int64))             # same sort, same bits
    again = M().grouped_auroc_ap(p, y, m, G)
    assert all(np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64)) for a, b in zip(again, (auroc, ap, n_pos, n_neg)))
    return auroc, ap, n_pos, n_neg


@pytest.mark.parametrize("pattern", ["continuous", "equal", "levels4", "signed_zero"])
@pytest.mark.parametrize("n", [1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_rank_stats_equal_recipe(n, pattern):
    rng = np.random.RandomState(n + len(pattern))
    labels = (rng.rand(n) < 0.3).astype(np.int64)
    if n == 2:
        labels[:] = [1, 0]
    probs = scores(pattern, n, rng)
    masks = rank_masks(n, labels, rng)
    auroc, ap, n_pos, n_neg = check_rank(probs, labels, masks)
    if n_pos[3]:
        assert auroc[3] == -11.0                                # positives only
    if n_neg[4]:
        assert auroc[4] == -10.0 and ap[4] == 0.0               # negatives only: scikit-learn's AP is 0
    assert np.isnan(auroc[5]) and ap[5] == 0.0                  # nobody
    if pattern == "equal" and n_pos[0] and n_neg[0]:
        assert auroc[0] == 0.5 and abs(ap[0] - n_pos[0] / n) <= 5 * EPS


def test_rank_stats_run_across_three_tiles_and_64_groups():
    n = 3 * TILE + 5
    rng = np.random.RandomState(11)
    labels = (rng.rand(n) < 0.4).astype(np.int64)
    probs = scores("long_run", n, rng)
    order, run_end = GR.sort_order(probs)
    ends = np.flatnonzero(run_end)
    assert ends[TILE - 10] == 2 * TILE + 9 and ends[TILE - 11] == TILE - 11       # the run starts in tile 0 and ends in tile 2
    check_rank(probs, labels, rank_masks(n, labels, rng, G=64))


def test_rank_stats_refuse_nan_and_cpu():
    n = 100
    p = torch.rand(n, device="cuda")
    y = (torch.rand(n, device="cuda") < 0.5).long()
    ones = torch.ones(n, dtype=torch.int64, device="cuda")
    M().grouped_auroc_ap(p, y, ones, 1)
    p[17] = float("nan")
    with pytest.raises(ValueError):
        M().grouped_auroc_ap(p, y, ones, 1)
    from simple_tad_amd._lib import TadError
    with pytest.raises(TadError, match="GPU"):
        M().grouped_confusion(p.cpu(), y.cpu(), ones.cpu(), 1)
    with pytest.raises(TadError, match="n_groups"):
        M().grouped_confusion(p, y, ones, 65)
    # the launches refuse what is not a contiguous GPU tensor of the right type and length
    flags = torch.ones(n, dtype=torch.uint8, device="cuda")
    for bad in ((y.int().cpu(), ones, flags), (y, ones, flags), (y.int(), ones[:-1], flags), (y.int(), ones, flags.bool())):
        with pytest.raises(TadError, match="contiguous GPU tensor"):
            M().group_rank_stats(*bad, 1)
    with pytest.raises(TadError, match="contiguous GPU tensor"):
        M().group_threshold_histogram(p.double(), y.int(), ones, 1, torch.tensor([0.5], device="cuda"))


# ------------------------------------------------------------------------------------------------ 3. golden G24, consistency
@pytest.fixture(scope="module")
def g24():
    a = GR.annotations()
    groups = GR.golden_groups(a)
    dev = {k: cuda(v) for k, v in groups.items()}
    return a, groups, M().grouped_more_metrics(cuda(a["probs"]), cuda(a["labels"]), dev)


def test_grouped_more_metrics_vs_sklearn(golden, g24):
    g = golden("g24_group_metrics")
    a, groups, got = g24
    assert list(got) == list(groups) and len(got) == 36
    for key, t in got.items():
        acc, precision, recall, f1, ap, auroc, confmat, mcc, p_t, r_t, acc_t, f1_t = t
        want = g[f"{key}.more"]
        assert np.array_equal(np.array(confmat), g[f"{key}.confmat"]), key
        assert np.allclose([acc, precision, recall, f1], want[:4], rtol=0, atol=1e-12), key
        assert abs(ap - want[4]) < 1e-9 and abs(auroc - want[5]) < 1e-9, key
        for vals, k in ((mcc, "mcc"), (p_t, "precision"), (r_t, "recall"), (acc_t, "acc"), (f1_t, "f1")):
            assert np.allclose(vals, g[f"{key}.{k}"], rtol=0, atol=1e-12), (key, k)
        assert abs(M().trapezoid(M().THRESHOLDS, mcc) - g[f"{key}.show"][1]) < 1e-12, key


def test_reports_reproduce_the_golden_lines_and_rows(golden, g24):
    g = golden("g24_group_metrics")
    a = g24[0]
    want = GR.read_report(GOLDEN_TXT)
    p, y = cuda(a["probs"]), cuda(a["labels"])
    codes = [GR.CAT_CODES[k] for k in a["clip_lvl_cat"]]
    assert M().DOTA_CAT_CODES == GR.CAT_CODES
    assert M().group_report(p, y, a["clip"], clip_lvl_cat=codes, clip_lvl_ego=a["clip_lvl_ego"]) == want["dota"]
    names = [f"clip_{c:03d}" for c in a["clip"]]                                       # names, integer categories, device tensors
    assert M().group_report(p, y, names, clip_lvl_cat=cuda(a["clip_lvl_cat"]), clip_lvl_ego=cuda(a["clip_lvl_ego"])) == want["dota"]
    assert M().group_report_dada(p, y, cuda(a["clip"]), ego=a["ego"]) == want["dada"]
    group_rows, thresh_rows = M().group_stats_tables(p, y, cat=a["cat"], ego=a["ego"], night=cuda(a["night"]))
    assert [r[0] for r in group_rows] == ["ego", "noego", "night", "day"]
    rows = np.array([r[1:] for r in group_rows], dtype=np.float64)
    assert np.allclose(rows[:, :4], g["group_rows"][:, :4], rtol=0, atol=1e-12) and np.allclose(rows[:, 4:], g["group_rows"][:, 4:], rtol=0, atol=1e-9)
    want_rows = GR.stats_tables(a)[1]
    assert [r[0] for r in thresh_rows] == [r[0] for r in want_rows] == ["all_samples"] + [f"cat_{k}" for k in range(10)] + ["ego", "noego", "night", "day"]
    n = len(GR.THRESHOLDS)
    for row in thresh_rows:
        vals = np.array(row[1:], dtype=np.float64)
        assert vals.shape == (5 * n,)
        if row[0].startswith("cat_"):
            assert np.allclose(vals[2 * n:3 * n], g["cat." + row[0][4:]], rtol=0, atol=1e-12) and (np.delete(vals, np.s_[2 * n:3 * n]) == -1).all()
        elif row[0] == "all_samples":
            assert np.allclose(vals, g["all_samples.thresh"], rtol=0, atol=1e-12)
        else:
            assert np.allclose(vals, np.concatenate([g[f"stats.{row[0]}.{k}"] for k in ("mcc", "precision", "recall", "acc", "f1")]), rtol=0, atol=1e-12)


def test_every_group_equals_calculate_more_metrics_on_its_slice(g24):
    a, groups, got = g24
    for key, mask in groups.items():
        one = M().calculate_more_metrics(cuda(a["probs"][mask]), cuda(a["labels"][mask]))
        t = got[key]
        assert t[6] == one[6] and all(t[i] == one[i] for i in (0, 1, 2, 3, 7, 8, 9, 10, 11)), key   # from equal integer counts
        assert abs(t[4] - one[4]) < 1e-12 and abs(t[5] - one[5]) < 1e-12, key


# ------------------------------------------------------------------------------------------------ 4. guard bands
@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("n,G", [(257, 33), (TILE + 1, 64)])
def test_group_launches_inside_guard_bands(n, G, poison):
    T = 101
    probs, labels, member = hist_case(n, G, 5)
    probs[np.isnan(probs)] = 0.25
    probs[::3] = probs[0]                                                               # ties
    order, run_end = GR.sort_order(probs)
    plain_hist = M().group_threshold_histogram(cuda(probs), cuda(labels), member_tensor(member), G, cuda(GR.THR32))
    plain_int, plain_ap = M().group_rank_stats(cuda(labels[order]), member_tensor(member[order]), cuda(run_end.astype(np.uint8)), G)
    arena = GuardedArena(16 << 20, "cuda", poison=poison)
    everyone = (torch.tensor([-1]), torch.tensor([-1]))                                 # a guard "sample" belongs to every group
    nan64 = (torch.tensor([float("nan")], dtype=torch.float64),) * 2
    p = arena.place(cuda(probs), role="input", name="probs")
    y = arena.place(cuda(labels), role="input", name="labels", index_range=2)
    m = arena.place(member_tensor(member), role="input", name="member", guard_pattern=everyone)
    thr = arena.place(cuda(GR.THR32), role="input", name="thresholds")
    hist = arena.place((G, 2, T + 1), torch.int64, role="output", name="hist", index_range=1 << 20)
    ys = arena.place(cuda(labels[order]), role="input", name="labels_sorted", index_range=2)
    ms = arena.place(member_tensor(member[order]), role="input", name="member_sorted", guard_pattern=everyone)
    re = arena.place(cuda(run_end.astype(np.uint8)), role="input", name="run_end")
    out_int = arena.place((G, 3), torch.int64, role="output", name="out_int", index_range=1 << 20)
    out_ap = arena.place((G,), torch.float64, role="output", name="out_ap", guard_pattern=nan64)
    M().group_threshold_histogram(p, y, m, G, thr, out=hist)
    M().group_rank_stats(ys, ms, re, G, out_int=out_int, out_ap=out_ap)
    arena.verify()
    assert np.array_equal(hist.cpu().numpy(), GR.group_hist(probs, labels, member, G, GR.THR32))
    assert torch.equal(hist, plain_hist) and torch.equal(out_int, plain_int) and same_bits(out_ap, plain_ap)
    ints, aps = GR.rank_stats_sorted(labels[order], member[order], run_end, G)
    assert out_int.cpu().numpy().tolist() == [list(t) for t in ints]
    assert np.all(np.abs(out_ap.cpu().numpy() - np.array(aps)) <= (int(run_end.sum()) + 4) * EPS)


# ------------------------------------------------------------------------------------------------ 5. final_test
def test_final_test_writes_group_metrics(tmp_path):
    import simple_tad_amd as T
    from simple_tad_amd import engine as E
    torch.manual_seed(0)
    model = T.VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2, qkv_bias=True, num_classes=2, all_frames=4,
                                init_scale=1.0).cuda()
    g = torch.Generator().manual_seed(1)
    data = []
    for b in range(5):
        clips = [f"clip{(6 * b + i) // 5}" for i in range(6)]                           # 6 clips of 5 windows
        info = {"ttc": torch.zeros(6), "clip": clips, "frame": [f"{6 * b + i:04d}.jpg" for i in range(6)]}
        data.append((torch.randn(6, 3, 4, 32, 32, generator=g), torch.randint(0, 2, (6,), generator=g), None, info))
    anno = {"clip_lvl_cat": {f"clip{c}": ["ST", "AH"][c % 2] for c in range(6)}, "clip_lvl_ego": {f"clip{c}": c < 3 for c in range(6)},
            "cat_codes": ["ST", "AH"]}
    preds, stats = tmp_path / "predictions.csv", tmp_path / "stats.txt"
    plain = E.final_test(data, model, torch.device("cuda"), str(preds), str(stats))
    assert not (tmp_path / "group_metrics.txt").exists()
    before = (open(preds).read(), open(stats).read())
    res = E.final_test(data, model, torch.device("cuda"), str(preds), str(stats), group_annotations=anno)
    assert res == plain and (open(preds).read(), open(stats).read()) == before          # nothing else changes
    lines = open(tmp_path / "group_metrics.txt").read().split("\n")
    assert lines[0] == GR.RULE and lines[3] == "TOTAL" and len(lines) == 8 + 4 + 2 * (6 + 4)
    assert [ln for ln in lines if ln.startswith("category")] == ["category ST", "category AH"] * 3
    assert lines[4].startswith("\tlen: 6 | auroc: ")
    total = float(lines[4].split("auroc: ")[1].split(" ")[0]) / 100
    # the stats file holds the AUROC binned at the 101 thresholds: a trapezoid through some vertices of the exact ROC curve, which
    # is monotone in between -- the two differ by at most half the cells' areas (plus the report's rounding to 0.1 %)
    import csv
    rows = list(csv.reader(open(preds, newline="")))[1:]
    logits = torch.tensor([[float(r[3]), float(r[4])] for r in rows], dtype=torch.float64).float().cuda()
    labels = torch.tensor([int(r[5]) for r in rows]).cuda()
    cm = M().calculate_metrics(logits, labels)
    fpr, tpr, _ = cm[8]
    stats_auroc = float(open(stats).read().split("auroc: ")[1].split(",")[0])
    assert stats_auroc == cm[5]
    assert abs(total - stats_auroc) <= 0.5 * float(np.sum(np.abs(np.diff(fpr)) * np.abs(np.diff(tpr)))) + 5.1e-4
    exact = M().exact_auroc_ap(torch.softmax(logits, 1)[:, 1], labels)[0]
    assert lines[4].split(" | ")[1] == f"auroc: {100 * exact:.1f}"
    other = tmp_path / "elsewhere.txt"
    E.final_test(data, model, torch.device("cuda"), str(preds), str(stats), group_annotations=anno, group_report_file=str(other))
    assert open(other).read().split("\n") == lines
    with pytest.raises(ValueError, match="group_annotations"):
        E.final_test(data, model, torch.device("cuda"), str(preds), str(stats), group_report_file=str(other))
