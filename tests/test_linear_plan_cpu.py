"""The launch plans of the Linear GEMMs (csrc/gemm_plan.hip; kernels.linear_plan / linear_bwd_weight_plan) against the plans the launchers made
before the planner existed -- tests/golden/g17_linear_plans.json (how it was recorded, the settings, the field names) with its numbers in
g17_linear_plans.npz, recorded launch by launch from the previous launchers; tools/linear_plan_cases.py is its case list.  Exact, field for
field: a change to the planner shows up here as a diff of plans, on a machine without a GPU.  Every case restores the knobs it moved."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "g17_linear_plans.json")


@pytest.fixture(scope="module")
def fx():
    from simple_tad_amd import _lib, build
    build.build(verbose=False)
    import ctypes
    cus = ctypes.c_int(0)
    # with a device the plans are made for ITS compute units; the fixture is for 256 (the MI355X, and what the library assumes without a device)
    if _lib.load().tad_device_info(ctypes.byref(cus), None, None, None, 0) == 0 and cus.value != 256:
        pytest.skip(f"plans recorded for 256 CUs, this device has {cus.value}")
    return load_fixture()


def load_fixture():
    """the JSON header with the arrays of the .npz beside it put back as nested lists: nt_cases[setting][problem], nt_plans[index] ..."""
    import numpy as np
    with open(FIXTURE) as f:
        fx = json.load(f)
    z = np.load(FIXTURE[:-len("json")] + "npz")

    def ragged(name):
        flat, off = z[name].tolist(), z[name + "_off"].tolist()
        return [flat[a:b] for a, b in zip(off, off[1:])]

    fx["nt_problems"] = [[fx["nt_entries"][p[0]]] + p[1:] for p in z["nt_problems"].tolist()]
    fx["tn_problems"] = z["tn_problems"].tolist()
    fx["nt_plans"], fx["tn_plans"] = ragged("nt_plans"), ragged("tn_plans")
    for kind in ("nt", "tn"):
        flat, n = ragged(kind + "_cases"), len(fx[kind + "_problems"])
        assert len(flat) == n * len(fx[kind + "_settings"])
        fx[kind + "_cases"] = [flat[i:i + n] for i in range(0, len(flat), n)]
    return fx


def _rows(plan, fields):
    return [[step[k] for k in fields] for step in plan]


def _split(flat, n):
    return [flat[i:i + n] for i in range(0, len(flat), n)]


def _check_tn(fx, K, s):
    """the weight-gradient plans of setting s (knobs already set); returns the number of cases"""
    from simple_tad_amd import _lib
    fields = fx["tn_fields"]
    assert tuple(fields) == _lib.LINEAR_BWD_WEIGHT_PLAN_FIELDS
    n = 0
    for (M, N1, N2, Kd), ent in zip(fx["tn_problems"], fx["tn_cases"][s]):
        ws = ent[0]
        need = max(_lib.load().tad_linear_bwd_weight_workspace_bytes(M, nn, Kd) for nn in ((N1, N2, N1 + N2) if N2 else (N1,)))
        assert need == ws, ("workspace query", M, N1, N2, Kd)
        for idx, ws_bytes in zip(ent[1:], (ws, None)):
            if ws_bytes is None:  # a pair with one byte less than its one-launch form needs
                ws_bytes = _lib.load().tad_linear_bwd_weight_workspace_bytes(M, N1 + N2, Kd) - 1
            got = _rows(K.linear_bwd_weight_plan(M, N1, Kd, N2=N2, ws_bytes=ws_bytes), fields)
            assert got == _split(fx["tn_plans"][idx], len(fields)), (fx["tn_settings"][s], (M, N1, N2, Kd), ws_bytes)
            n += 1
    return n


def test_nt_plans_are_the_recorded_ones(fx):
    from simple_tad_amd import _lib, kernels as K
    fields = fx["nt_fields"]
    assert tuple(fields) == _lib.LINEAR_PLAN_FIELDS
    lib = _lib.load()
    n = 0
    for knobs, per_problem in zip(fx["nt_settings"], fx["nt_cases"]):
        saved = {k: K.linear_tuning_get(k) for k in knobs}
        try:
            K.linear_tuning(**knobs)
            for (entry, M, N, Kd, out16, epi, residual, res_mod, rowscale, rps, colscale), ent in zip(fx["nt_problems"], per_problem):
                need = ent[0]
                assert lib.tad_linear_workspace_bytes(M, N, Kd) == need, ("workspace query", knobs, M, N, Kd)
                for idx, ws_bytes in zip(ent[1:], (0, need, need - 1)):
                    got = _rows(K.linear_plan(M, N, Kd, epilogue=epi, out_16bit=out16, residual=residual, res_mod=res_mod, rowscale=rowscale,
                                              rows_per_scale=rps, colscale_cols=colscale, ws_bytes=ws_bytes), fields)
                    assert got == _split(fx["nt_plans"][idx], len(fields)), (knobs, (entry, M, N, Kd, out16, epi, residual, res_mod, rowscale, rps, colscale), ws_bytes)
                    n += 1
        finally:
            K.linear_tuning(**saved)
    assert n == sum(len(e) - 1 for per in fx["nt_cases"] for e in per) and n > 20000


def test_tn_plans_are_the_recorded_ones(fx):
    from simple_tad_amd import kernels as K
    n = 0
    for s, (knobs, env) in enumerate(fx["tn_settings"]):
        if env is not None:
            continue
        saved = {k: K.linear_tuning_get(k) for k in knobs}
        try:
            K.linear_tuning(**knobs)
            n += _check_tn(fx, K, s)
        finally:
            K.linear_tuning(**saved)
    assert n == sum(len(e) - 1 for (_, env), per in zip(fx["tn_settings"], fx["tn_cases"]) if env is None for e in per) and n > 1000


@pytest.mark.parametrize("variant", [1, 3])
def test_tn_plans_with_the_variant_forced_from_the_environment(fx, variant):
    """TAD_GEMM_TN_VARIANT has no tad_linear_tuning key: the library reads it when it is loaded, so these plans are checked in a process of
    their own (which is what this test is about)"""
    s = [i for i, (_, env) in enumerate(fx["tn_settings"]) if env == variant]
    assert len(s) == 1
    code = ("import json, sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_linear_plan_cpu as T; from simple_tad_amd import kernels as K\n"
            "print('cases', T._check_tn(T.load_fixture(), K, %d))" % (ROOT, os.path.join(ROOT, "tests"), s[0]))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TAD_GEMM_TN_VARIANT=str(variant)), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split()[-2:] == ["cases", str(sum(len(e) - 1 for e in fx["tn_cases"][s[0]]))]


def test_plan_query_refuses_what_the_entry_points_refuse(fx):
    from simple_tad_amd import _lib, kernels as K
    with pytest.raises(_lib.TadError, match="K=60"):
        K.linear_plan(4096, 768, 60)
    with pytest.raises(_lib.TadError, match="epilogue"):
        K.linear_plan(4096, 768, 64, epilogue=4)
    with pytest.raises(_lib.TadError, match="multiples of 8"):
        K.linear_bwd_weight_plan(4096, 772, 768)
    import ctypes
    buf = (ctypes.c_int32 * 11)()
    lib = _lib.load()
    assert lib.tad_linear_plan(32 * 1568, 768, 768, 0, 1, 0, 0, 0, 1, 0, 0, buf, 1) == -3  # two launches, room for one
    assert b"room for 1" in lib.tad_last_error_string()
    # a problem cut into row ranges comes back whole through the growing buffer of kernels.linear_plan
    plan = K.linear_plan(523776 + 50176, 1024, 4096, out_16bit=False)
    assert [s["r0"] for s in plan if s["r0"] in (0, 523776)] and sum(s["rows"] for s in plan) == 523776 + 50176
