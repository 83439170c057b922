"""The per-element attention bounds (tests/attn_bounds.py) against the rounding-model emulation of the kernels, no GPU: the emulation stays
inside the bound at EVERY element of out, lse, dQ, dK and dV; each of four planted defects leaves it; and the masked-key leak does so while the
whole-tensor criterion of tests/test_kernels_gpu.py (ATT_TOL / ATT_TOL_MAX) still passes -- the reason the per-element yardstick exists."""
import pytest
import torch

import attn_bounds as AB
from test_kernels_gpu import ATT_TOL, ATT_TOL_F16, ATT_TOL_MAX, ATT_TOL_MAX_F16, rell2, relmax

LENGTHS = (1, 2, 5, 33, 64, 65, 129, 257)
# the probe family has one V column per key: it exists for N <= d only
CASES = [(fam, fmt, d, N) for fam in AB.FAMILIES for fmt in ("bf16", "f16") for d in (64, 80) for N in LENGTHS if fam != "probe" or N <= d]


def run_chain(x, defect=None, f32_terms=True):
    """the emulated kernels on `x` against their bounds: {name: worst error / bound over ALL elements}, the reference, the emulated out32"""
    r = AB.reference(x.qkv, x.dout, x.scale, x.B, x.N, x.H, x.d)
    fb = AB.fwd_bounds(r, x.fmt, f32_terms)
    out32, out16, out_lo, lse = AB.emulate_fwd(r, x.fmt, defect)
    w = {"out32": AB.worst(out32, r.out, fb["out32"]), "out16": AB.worst(out16, r.out, fb["out16"]),
         "out16+lo": AB.worst(out16 + out_lo, r.out, fb["sum16"]), "lse": AB.worst(lse, r.lse, fb["lse"])}
    # the backward on exact operands, then on the forward's own outputs with and without out_lo
    for tag, ops in (("exact", (r.lse, r.out, None)), ("chain+lo", (lse, out16, out_lo)), ("chain", (lse, out16, None))):
        bb = AB.bwd_bounds(r, x.fmt, *ops, f32_terms=f32_terms)
        got = AB.emulate_bwd(r, x.fmt, *ops, defect=defect)
        for nm, g in zip(("dq", "dk", "dv"), got):
            assert g.shape == r[nm].shape == bb[nm].shape
            w[f"{nm}.{tag}"] = AB.worst(g, r[nm], bb[nm])
    return {k: float(v) for k, v in w.items()}, r, out32


@pytest.mark.parametrize("family,fmt,d,N", CASES)
def test_emulation_stays_inside_the_bound_at_every_element(family, fmt, d, N):
    for prescaled in (False, True):
        x = AB.make_inputs(family, fmt, d, N, prescaled=prescaled)
        rnd = AB.rounder(fmt)
        assert torch.equal(rnd(x.opnd), x.opnd) and torch.equal(rnd(x.dout), x.dout), "operands must be exact in the format"
        w, r, _ = run_chain(x)
        over = {k: v for k, v in w.items() if not v <= AB.SLACK}
        assert not over, f"{family} {fmt} d={d} N={N} prescaled={prescaled}: error / bound {over}"
        if family == "probe":  # the columns no key writes: bound 0, exactly 0.0 (already implied by ratio <= SLACK: x / 0 = inf)
            fb = AB.fwd_bounds(r, fmt)
            assert ((fb["out16"] == 0).sum() == 2 * 2 * N * (d - N)) and (r.out[fb["out16"] == 0] == 0).all()


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_leading_terms_alone_hold_over_twenty_seeds(fmt):
    """the emulation rounds at the 16-bit points only, so the leading terms must already cover it (measured: worst ratio 0.94)"""
    worst = {}
    for seed in range(20):
        for d, N in ((64, 65), (80, 33)):
            w, _, _ = run_chain(AB.make_inputs("spread", fmt, d, N, seed=seed, prescaled=bool(seed & 1)), f32_terms=False)
            for k, v in w.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print({k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= AB.SLACK, worst


DEFECT_CASES = [("spread", fmt, d, N) for fmt in ("bf16", "f16") for d in (64, 80) for N in (5, 33, 65, 129)]
# where each defect must show: (a) the forward outputs, (b) dK / dV, (c) the chain that declares out_lo, (d) any gradient
DEFECT_SHOWS_IN = {"masked_key": ("out32", "out16", "out16+lo"), "dead_query_row": ("dk.", "dv."), "out_lo_ignored": ("chain+lo",),
                   "lse_row_off": ("dq.", "dk.", "dv.")}


@pytest.mark.parametrize("defect", AB.DEFECTS)
def test_each_planted_defect_breaks_the_bound(defect):
    broke = []
    for family, fmt, d, N in DEFECT_CASES:
        x = AB.make_inputs(family, fmt, d, N, prescaled=True)
        w, r, out32 = run_chain(x, defect=defect)
        hit = {k: v for k, v in w.items() if v > AB.SLACK and any(s in k for s in DEFECT_SHOWS_IN[defect])}
        if hit:
            broke.append((fmt, d, N, max(hit.values())))
        if defect == "masked_key":
            # ... while the whole-tensor criterion passes in EVERY case: the old yardstick cannot see this leak
            tol, tol_max = (ATT_TOL, ATT_TOL_MAX) if fmt == "bf16" else (ATT_TOL_F16, ATT_TOL_MAX_F16)
            assert relmax(out32, r.out) <= tol_max and rell2(out32, r.out) <= tol, (fmt, d, N, relmax(out32, r.out), rell2(out32, r.out))
    print(defect, broke)
    assert broke, f"{defect}: no case left the bound"
    assert {"bf16", "f16"} <= {b[0] for b in broke}, f"{defect}: not seen in both formats: {broke}"
