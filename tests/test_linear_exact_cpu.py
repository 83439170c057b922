"""The conditions behind tests/test_linear_exact_gpu.py, proved without a GPU before any kernel is trusted (helper: tests/linear_exact.py):

  a. every case of the table is admissible: sum |x||w| + |bias| + |residual| stays below 2^24 quanta, so every partial sum in any order is
     exact in f32;
  b. every launch form the table reaches is reached by a case with >= 90 % of its outputs NOT representable in bf16, and by one with >= 90 %
     not representable in half: a 16-bit intermediate cannot hide in any of them;
  c. an independent f32 implementation -- torch's CPU matmul, its own blocking and order -- reproduces the integer reference bit for bit on
     the operands widened from bf16 and from half: "any f32 order is exact", shown;
  d. from the planner (kernels.linear_plan / linear_bwd_weight_plan, no GPU): the union of the table's plans reaches every tile configuration,
     scheduling form, split-K mode, epilogue instantiation and weight-gradient kernel -- a later planner change cannot silently empty a branch of
     the GPU file.

Run with -s to see the figures."""
import pytest
import torch

import linear_exact as X

ALL = X.CASES + X.NONPOW2_CASES
IDS = [c["id"] for c in ALL]


@pytest.fixture(scope="module")
def shares():
    """admissible() of every case, once: the whole output of the small cases, sampled rows of the tall forwards (all of a weight gradient:
    its reduction is what is large, not its output)"""
    out = {}
    for c in ALL:
        # (the residual cases whole: their first rows, which a sample takes, are the dropped clip's)
        sampled = (not X.small(c) or (c["M"] > 4096 and c["epi"] != "res")) and c["entry"] in ("fwd", "qkv", "bwd_input")
        out[c["id"]] = X.admissible(c, rows=X.sample_rows(c) if sampled else None)
    return out


def test_every_case_is_admissible(shares):
    for c in ALL:
        s = shares[c["id"]]
        print(f"{c['id']}: bound {s['bound']:.0f} quanta of 2^24 = {X.LIMIT}, max |output| {s['max']:.6g}, not representable bf16 {s['bf16']:.1%} / half {s['f16']:.1%}")
        assert s["bound"] < X.LIMIT
        if c["out"] == "16":  # the rounded output must stay finite in half (65504), or its comparison would be one of infinities
            assert s["max"] < 65504, c["id"]


def test_the_admissibility_check_refuses_an_overfull_accumulator():
    """(the check is live) 100 ... 127 x 100 ... 127 over K = 3072 passes 2^24"""
    X.FAMILIES["overfull"] = ((100, 127), (100, 127))
    try:
        with pytest.raises(AssertionError, match="2\\^24"):
            X.admissible(X._c("overfull", "fwd", 64, 64, 3072, "overfull"))
    finally:
        del X.FAMILIES["overfull"]


@pytest.mark.parametrize("case", [c for c in ALL if X.small(c)], ids=[c["id"] for c in ALL if X.small(c)])
def test_torch_f32_matmul_reproduces_the_integer_reference(case):
    """(c) the operands rounded to the 16-bit format and widened again are the integers themselves; torch's f32 matmul of them, the f32
    bias / residual adds and the f32 column sums equal the int64 reference bit for bit"""
    o = X.operands(case)
    e, s = case["entry"], 2.0 ** -case["scale_log2"]
    if case["M"] * case["N"] * case["K"] > 1 << 28:  # (torch's int64 matmul is slow; fp64 holds these integers just as exactly)
        o = {k: v.double() if v is not None and v.dtype == torch.int64 else v for k, v in o.items()}
    for fmt, dt in X.OP16.items():
        def op(t, scale=1.0):
            w = (t.double() * scale).to(dt).float()
            assert torch.equal(w.double(), t.double() * scale), f"{case['id']}: an operand is not exact in {fmt}"
            return w

        if e == "patch_embed":
            P = X.PATCH_EMBED
            cols = X.im2col(o["clip"], P["tubelet"], P["patch"])
            got = op(cols) @ op(o["w"]).t() + o["bias"].float() + o["pos"].float()
            assert torch.equal(got.double(), X.ref_patch_embed(o["clip"], o["w"], o["bias"], o["pos"]).double())
        elif e in ("fwd", "qkv"):
            got = op(o["x"], s) @ op(o["w"]).t()
            if o["bias"] is not None:
                got = got + (o["bias"].double() * s).float()
            ref = X.ref_linear(o["x"], o["w"], o["bias"]).double() * s
            if case["epi"] == "res":
                rs = o["rowscale"].repeat_interleave(case["rows_per_scale"])[:case["M"], None]
                got = got * (o["gamma"] * rs) + o["res"].float()
                ref = X.ref_residual(o["x"], o["w"], o["bias"], o["res"], o["gamma"], o["rowscale"], case["rows_per_scale"])[0]
            assert torch.equal(got.double(), ref), X.first_mismatch(got.double(), ref)
        elif e == "bwd_input":
            got = op(o["dy"]) @ op(o["wT"]).t()
            assert torch.equal(got.double(), X.ref_bwd_input(o["dy"], o["wT"]).double())
        else:
            acc = case["accumulate"]
            dW, db = X.ref_bwd_weight(o["dy"], o["x"], o["dW0"] if acc else None, o["db0"] if acc else None)
            got = op(o["dy"]).t() @ op(o["x"])
            gb = op(o["dy"]).sum(0)
            if acc:
                got, gb = got + o["dW0"].float(), gb + o["db0"].float()
            assert torch.equal(got.double(), dW.double()) and torch.equal(gb.double(), db.double())
            if e == "bwd_weight_pair":
                got2 = op(o["dy2"]).t() @ op(o["x2"]) + (o["dW02"].float() if acc else 0.0)
                assert torch.equal(got2.double(), X.ref_bwd_weight(o["dy2"], o["x2"], o["dW02"] if acc else None)[0].double())


# ---------------------------------------------------------------------------- (d), (b): what the table reaches
NT_KERNELS = (1, 2, 3, 4, 5, 7, 8, 9, 10)  # 10 = NT_SPLITK (csrc/gemm_plan.h)
EPI_NAMES = {0: "PLAIN", 1: "GELU", 2: "RESIDUAL", 3: "DGELU", 4: "RESMOD"}
TN_NAMES = {0: "TN_W4", 1: "TN_PDEEP", 2: "TN_W8", 3: "TN_W8_128"}
REQUIRED = ([f"nt kernel {k}" for k in NT_KERNELS] + ["persist 0", "persist 1", "direct 0", "direct 1", "sk_mode 0", "sk_mode 1", "sk_mode 2"]
            + ["epilogue " + n for n in EPI_NAMES.values()] + ["output 16-bit", "output f32", "more than one step"]
            + ["tn kernel " + n for n in TN_NAMES.values()] + ["tn splits = 1", "tn splits > 1", "pair in one launch", "pair as two launches"])
ENTRIES = ("fwd", "bwd_input", "qkv", "patch_embed", "bwd_weight", "bwd_weight_qkv", "bwd_weight_pair")


def forms_of(K, lib, case):
    """the launch forms of one case under every knob setting it runs with (knobs restored)"""
    forms = set()
    try:
        for _, cfg in case["knobs"]:
            K.linear_tuning(**{**K.LINEAR_TUNING_DEFAULTS, **cfg})
            if case["entry"].startswith("bwd_weight"):
                M, N, Kd, N2 = case["M"], case["N"], case["K"], case["N2"]
                need = max(lib.tad_linear_bwd_weight_workspace_bytes(M, n, Kd) for n in ((N, N2, N + N2) if N2 else (N,)))
                plan = K.linear_bwd_weight_plan(M, N, Kd, N2=N2, ws_bytes=need)
                for r in plan:
                    forms |= {"tn kernel " + TN_NAMES[r["kernel"]], "tn splits = 1" if r["splits"] == 1 else "tn splits > 1"}
                if N2:
                    assert len(plan) == (1 if plan[0]["pair"] else 2)
                    forms.add("pair in one launch" if plan[0]["pair"] else "pair as two launches")
                continue
            M, N, Kd, kw = X.nt_problem(case)
            ws = lib.tad_linear_workspace_bytes(M, N, Kd) if case["entry"] in ("fwd", "bwd_input") else 0  # (the other entry points offer none)
            plan = K.linear_plan(M, N, Kd, ws_bytes=ws, **kw)
            for s in plan:
                forms |= {f"nt kernel {s['kernel']}", f"persist {s['persistent']}", f"direct {s['direct']}", "epilogue " + EPI_NAMES[s["epilogue"]]}
                if s["kernel"] == 10:
                    forms.add(f"sk_mode {s['sk_mode']}")
            forms.add("output 16-bit" if case["out"] == "16" else "output f32")
            if len(plan) > 1:
                forms.add("more than one step")
    finally:
        K.linear_tuning(**K.LINEAR_TUNING_DEFAULTS)
    return forms


@pytest.fixture(scope="module")
def reach():
    """{launch form: [case ids]} from the planner, for 256 compute units"""
    import ctypes
    from simple_tad_amd import _lib, build, kernels as K
    build.build(verbose=False)
    lib = _lib.load()
    cus = ctypes.c_int(0)
    if lib.tad_device_info(ctypes.byref(cus), None, None, None, 0) == 0 and cus.value != 256:
        pytest.skip(f"the shapes of the table are chosen for 256 CUs, this device has {cus.value}")
    out = {}
    for c in X.CASES:
        for f in forms_of(K, lib, c):
            out.setdefault(f, []).append(c["id"])
    assert all(K.linear_tuning_get(k) == v for k, v in K.LINEAR_TUNING_DEFAULTS.items()), "a knob was left moved"
    return out


def test_the_case_table_reaches_every_launch_form(reach):
    for f in REQUIRED:
        print(f"{f}: {len(reach.get(f, []))} cases, e.g. {reach.get(f, ['-'])[0]}")
    missing = [f for f in REQUIRED if not reach.get(f)]
    assert not missing, f"no case of linear_exact.CASES reaches: {missing}"
    assert {c["entry"] for c in X.CASES} == set(ENTRIES)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_every_launch_form_and_entry_point_has_a_case_16_bits_cannot_hold(reach, shares, fmt):
    """(b) >= 90 % of the outputs of at least one case per launch form, and per entry point, are not representable in the format: an
    intermediate that passed through it shows in nine outputs of ten"""
    by_id = X.CASE_BY_ID
    groups = {f: reach[f] for f in REQUIRED}
    groups.update({"entry " + e: [c["id"] for c in X.CASES if c["entry"] == e] for e in ENTRIES})
    for name, ids in groups.items():
        best = max(ids, key=lambda i: shares[i][fmt])
        print(f"{name}: {shares[best][fmt]:.1%} of {best} not representable in {fmt}")
        assert shares[best][fmt] >= 0.9, f"{name}: the best case, {best}, has only {shares[best][fmt]:.1%} of its outputs outside {fmt}"
        assert by_id[best]["family"] != "signed"
