"""Grouped evaluation report, CPU side: the numpy recipe (tests/group_metrics_recipe.py) against golden G24 = scikit-learn and the
reference's anaysis/metrics.py on the same synthetic annotation table (tools/make_goldens_group_metrics.py); pack_groups; host
argument validation of the two entry points; header / binding / exports."""
import ctypes
import os

import numpy as np
import pytest
import torch

import group_metrics_recipe as GR

GOLDEN_TXT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g24_group_metrics.txt")


@pytest.fixture(scope="module")
def table():
    a = GR.annotations()
    groups = GR.golden_groups(a)
    return a, groups, GR.more_metrics(a["probs"], a["labels"], groups)


def test_recipe_matches_golden_for_every_group(golden, table):
    g = golden("g24_group_metrics")
    a, groups, m = table
    # DoTA: TOTAL + 9 categories + (EGO, NON-EGO) x (the group + 9 categories) = 30; DADA's two; ego / noego / night / day by frame
    assert len(groups) == 36 and sum(k.startswith("dota.") for k in groups) == 30
    for key, r in m.items():
        assert np.array_equal(r["cm"], g[f"{key}.cm"]) and np.array_equal(r["cm"][GR.I5], g[f"{key}.confmat"]), key   # exact counts
        assert [r["P"], r["N"], r["U2"]] == g[f"{key}.pnu"].tolist(), key
        acc, precision, recall, f1_last, ap, auroc = g[f"{key}.more"]
        assert abs(r["auroc"] - auroc) < 1e-12 and abs(r["ap"] - ap) < 1e-12, key
        assert np.allclose(r["at05"], [acc, precision, recall, f1_last], rtol=0, atol=1e-12), key
        for k in ("mcc", "precision", "recall", "acc", "f1"):
            assert np.allclose(r[k], g[f"{key}.{k}"], rtol=0, atol=1e-12), (key, k)
        show = g[f"{key}.show"]
        assert abs(r["auroc"] - show[0]) < 1e-12 and abs(r["mcc_auc"] - show[1]) < 1e-12 and abs(r["mcc"][GR.I5] - show[2]) < 1e-12, key
        assert GR.n_clips(a["clip"], groups[key]) == int(g[f"{key}.len"]), key


def test_recipe_report_lines_equal_the_golden_text(table):
    a = table[0]
    want = GR.read_report(GOLDEN_TXT)
    assert len(want["dota"]) == 8 + 18 + 2 * (6 + 18) and len(want["dada"]) == 12
    assert GR.report(a, GR.dota_groups(a), GR.dota_lines) == want["dota"]
    assert GR.report(a, GR.dada_groups(a), GR.dada_lines) == want["dada"]


def test_recipe_stats_tables_match_golden(golden, table):
    g = golden("g24_group_metrics")
    group_rows, thresh_rows = GR.stats_tables(table[0])
    assert [r[0] for r in group_rows] == ["ego", "noego", "night", "day"]
    assert np.allclose(np.array([r[1:] for r in group_rows], dtype=np.float64), g["group_rows"], rtol=0, atol=1e-12)
    names = [r[0] for r in thresh_rows]
    assert names == ["all_samples"] + [f"cat_{k}" for k in range(10)] + ["ego", "noego", "night", "day"]
    n = len(GR.THRESHOLDS)
    for row in thresh_rows:
        assert len(row) == 1 + 5 * n
        vals = np.array(row[1:], dtype=np.float64)
        if row[0].startswith("cat_"):
            assert np.allclose(vals[2 * n:3 * n], g["cat." + row[0][4:]], rtol=0, atol=1e-12), row[0]
            assert (np.delete(vals, np.s_[2 * n:3 * n]) == -1).all()
        elif row[0] == "all_samples":
            assert np.allclose(vals, g["all_samples.thresh"], rtol=0, atol=1e-12)
        else:
            want = np.concatenate([g[f"stats.{row[0]}.{k}"] for k in ("mcc", "precision", "recall", "acc", "f1")])
            assert np.allclose(vals, want, rtol=0, atol=1e-12), row[0]


def test_recipe_tie_runs_are_the_groups_runs():
    """a group's AUROC / AP from the runs of the WHOLE array equal those from the runs of its own members (scores on 4 levels)"""
    rng = np.random.RandomState(3)
    n = 500
    probs = (rng.randint(0, 4, n) / 4).astype(np.float32)
    labels = rng.randint(0, 2, n)
    masks = [rng.rand(n) < q for q in (1.0, 0.5, 0.1)]
    (ints, aps), _ = GR.rank_stats(probs, labels, GR.pack(masks), 3)
    for g, mk in enumerate(masks):
        (own, own_ap), _ = GR.rank_stats(probs[mk], labels[mk], GR.pack([np.ones(int(mk.sum()), dtype=bool)]), 1)
        assert ints[g] == own[0] and abs(aps[g] - own_ap[0]) < 1e-15


def test_pack_groups_bit_layout_and_errors():
    from simple_tad_amd import _lib, metrics as M
    n = 5
    groups = {f"g{k}": np.zeros(n, dtype=bool) for k in range(64)}
    groups["g0"] = np.array([1, 0, 0, 1, 1], dtype=bool)
    groups["g1"] = torch.tensor([0, 1, 0, 1, 0], dtype=torch.bool)
    groups["g63"] = np.array([0, 0, 1, 1, 0], dtype=bool)
    names, member = M.pack_groups(groups, n, device="cpu")
    assert names == [f"g{k}" for k in range(64)] and member.dtype == torch.int64 and member.shape == (n,)
    assert member.numpy().view(np.uint64).tolist() == [1, 2, 1 << 63, (1 << 63) | 3, 1]
    assert np.array_equal(member.numpy().view(np.uint64), GR.pack([np.asarray(groups[k]) for k in names]))
    with pytest.raises(_lib.TadError, match="65 groups"):
        M.pack_groups({**groups, "one more": np.zeros(n, dtype=bool)}, n, device="cpu")
    with pytest.raises(_lib.TadError, match="'b' has 4 entries"):
        M.pack_groups({"a": np.zeros(n, dtype=bool), "b": np.zeros(4, dtype=bool)}, n, device="cpu")
    with pytest.raises(_lib.TadError):
        M.pack_groups({}, n, device="cpu")
    assert M.auroc_from_counts(3, 0, 0) == -11.0 and M.auroc_from_counts(0, 2, 0) == -10.0 and np.isnan(M.auroc_from_counts(0, 0, 0))
    assert M.auroc_from_counts(2, 3, 7) == 7 / 12


def test_group_entry_points_validate_on_the_host():
    """argument checks run before any launch (no GPU here): null pointers, n <= 0, group and threshold counts out of range"""
    from simple_tad_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    hist = lib.tad_group_threshold_histogram
    assert hist(None, p, p, 1, p, 1, 1, p, None) == -1 and b"null" in lib.tad_last_error_string()
    assert hist(p, p, None, 1, p, 1, 1, p, None) == -1 and b"null" in lib.tad_last_error_string()
    assert hist(p, p, p, 1, p, 1, 1, None, None) == -1 and b"null" in lib.tad_last_error_string()
    for G in (0, 65, -1):
        assert hist(p, p, p, G, p, 1, 1, p, None) == -1 and b"n_groups" in lib.tad_last_error_string()
    for T in (0, 256):
        assert hist(p, p, p, 1, p, T, 1, p, None) == -1 and b"thresholds" in lib.tad_last_error_string()
    assert hist(p, p, p, 1, p, 1, 0, p, None) == -1 and b"n > 0" in lib.tad_last_error_string()
    rank = lib.tad_group_rank_stats
    assert rank(None, p, p, 1, 1, p, p, None) == -1 and b"null" in lib.tad_last_error_string()
    assert rank(p, p, p, 1, 1, p, None, None) == -1 and b"null" in lib.tad_last_error_string()
    for G in (0, 65):
        assert rank(p, p, p, G, 1, p, p, None) == -1 and b"n_groups" in lib.tad_last_error_string()
    for n in (0, -3, 1 << 31):
        assert rank(p, p, p, 1, n, p, p, None) == -1 and b"2^31" in lib.tad_last_error_string()


def test_header_binding_and_exports_still_agree():
    import test_cabi_cpu as C
    from simple_tad_amd import _lib, build
    syms = C.header_symbols()
    assert {"tad_group_threshold_histogram", "tad_group_rank_stats"} <= set(syms) and sorted(_lib.SIGNATURES) == syms
    lib = ctypes.CDLL(build.build(verbose=False))
    assert all(hasattr(lib, s) for s in syms) and _lib.load().tad_abi_version() == 5
    txt = open(C.HEADER).read()
    assert f"#define TAD_GROUP_RANK_TILE {_lib.GROUP_RANK_TILE}" in txt
    assert "group_metrics.hip" in build.SOURCES and "group_metrics.hip" not in build.F16_SOURCES
