"""The references and inputs of the numeric edge tests, proven on the CPU: every bound tests/test_numeric_edges_gpu.py holds a HIP
kernel to is met by the reference arithmetic alone, and the inputs separate a right kernel from a subtly wrong one.

  * the GELU / GELU' polynomials of csrc/common.h are the ones tools/fit_gelu_poly.py prints, and over every finite 16-bit value and
    the f32 sweeps they stay inside the stated per-element bounds, in f64 (the approximation alone) and in f32 in the kernel's order;
  * torch's 16-bit casts round to nearest even on the rounding cases of the sweep (they are the reference of the bit-exact store tests);
  * torch's f32 LayerNorm errs by the tabulated figures per row class and D, and a one-pass variance in f32 exceeds the resulting bound
    by at least 100x on the z + offset rows.

Run with -s to see the tables."""
import numpy as np
import pytest
import torch

import edge_cases as E


# ------------------------------------------------------------------ A
def test_header_polynomials_are_the_fitters():
    hdr, fit = E.header_tables(), E.fitter_tables()
    assert set(hdr) == set(fit)
    for key, (xmax, texts) in hdr.items():
        fx, mono = fit[key]
        assert xmax == fx, (key, xmax, fx)
        assert texts == [f"{c:.9e}f" for c in mono], f"{key}: csrc/common.h differs from tools/fit_gelu_poly.py"


def _errors(fmt, x):
    """(gelu error / max(1, |x|), gelu' error) maxima over the f32 tensor x: f64 evaluation, f32 evaluation in the kernel's order"""
    xd = x.double()
    xn = x.numpy()
    scale = xd.abs().clamp_min(1.0)
    out = []
    for f32 in (False, True):
        eg = ((torch.as_tensor(E.fast_gelu_cpu(xn, fmt, f32)) - E.gelu64(xd)).abs() / scale)
        ed = (torch.as_tensor(E.fast_dgelu_cpu(xn, fmt, f32)) - E.dgelu64(xd)).abs()
        out.append((eg.max().item(), xd[eg.argmax()].item(), ed.max().item(), xd[ed.argmax()].item()))
    return out


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_polynomial_bounds_over_every_finite_16bit_value_and_the_sweeps(fmt):
    p = E.op16_patterns(fmt).float()
    finite = p[torch.isfinite(p)]
    assert finite.numel() == (65280 if fmt == "bf16" else 63488)
    sweep = E.f32_sweep(fmt)
    assert torch.isfinite(sweep).all() and sweep.numel() > finite.numel() + 40000
    for what, x in (("finite 16-bit values", finite), ("f32 sweep", sweep)):
        (g64, gx64, d64, dx64), (g32, gx32, d32, dx32) = _errors(fmt, x)
        print(f"{fmt} {what} ({x.numel()}): gelu/max(1,|x|) f64 {g64:.3e} at {gx64:.6g}, f32 {g32:.3e} at {gx32:.6g} (stated {E.STATED[(fmt, 'gelu')]:.2e}); "
              f"gelu' f64 {d64:.3e} at {dx64:.6g}, f32 {d32:.3e} at {dx32:.6g} (stated {E.STATED[(fmt, 'dgelu')]:.2e})")
        for k, e64, e32 in (("gelu", g64, g32), ("dgelu", d64, d32)):
            assert e64 <= E.STATED[(fmt, k)] and e32 <= E.STATED[(fmt, k)], (fmt, what, k, e64, e32)
            assert e32 <= E.CPU_F32[(fmt, k)] <= E.STATED[(fmt, k)], (fmt, what, k, e32)


def test_the_stated_f16_gelu_grad_bound_was_too_tight_by_rounding():
    """6.0e-6 was stated; the f32 evaluation reaches 6.02e-6 at a finite half value (the comment in csrc/common.h now says so)"""
    p = E.op16_patterns("f16").float()
    (_, _, _, _), (_, _, d32, at) = _errors("f16", p[torch.isfinite(p)])
    print(f"f16 gelu' f32 maximum over the finite half values: {d32:.4e} at {at}")
    assert 6.0e-6 < d32 <= E.STATED[("f16", "dgelu")]


def test_sweeps_hold_the_rounding_cases():
    for fmt, dt in E.OP16.items():
        x = E.f32_sweep(fmt)
        r = x.to(dt).float()
        up, down = (r.abs() > x.abs()).sum().item(), (r.abs() < x.abs()).sum().item()
        assert up > 5000 and down > 5000  # a truncating store differs on every `up` element
        drop = 16 if fmt == "bf16" else 13
        tail = torch.as_tensor(x.numpy().view(np.int32) & ((1 << drop) - 1))
        assert (tail == 1 << (drop - 1)).sum().item() >= 3000, "exact ties"
        ties = x[(tail == 1 << (drop - 1)) & (x.abs() > 1e-4) & (x.abs() < 6e4)]
        assert (ties.to(dt).view(torch.int16) & 1 == 0).all(), "ties go to the even neighbour"
        assert torch.isinf(r).any() and (r == torch.finfo(dt).max).any() and ((r != 0) & (r.abs() < torch.finfo(dt).tiny)).any()
    b = E.bias_sweep("bf16")
    assert b.numel() % 256 == 0 and b.numel() >= 385 * 256 and torch.isnan(b).sum() == 1 and torch.isinf(b).sum() == 2


# ------------------------------------------------------------------ C
def test_layernorm_reference_error_table_and_one_pass_separation():
    print("\ntorch f32 LayerNorm against fp64, class maxima (y / rstd / dx per row, relative to the row maximum); bound = 4x, floor 8 ulp")
    for D in E.LN_DIMS:
        x, gamma, beta, dy, dres, cls = E.ln_rows(D)
        assert x.shape[0] % 4 == 1 and x.shape[0] % 32 != 0
        bnd = E.ln_bounds(D)
        y_ref, mean_ref, _ = E.ln_ref(x, gamma, beta)
        one = E.row_relmax(E.ln_one_pass_f32(x, gamma, beta), y_ref)
        tmean = E.ln_torch_f32(x, gamma, beta, dy)[1]
        assert ((tmean.double() - mean_ref).abs() <= E.mean_bound(x)).all(), "torch's own f32 mean leaves the summation-tree bound"
        for c, name in enumerate(E.LN_CLASSES):
            o = one[cls == c].max().item()  # (one row over the bound fails the GPU test)
            print(f"D {D:5d} {name:10s} y {bnd['raw']['y'][c]:.2e} (bound {bnd['y'][c]:.2e})  rstd {bnd['raw']['rstd'][c]:.2e}  dx {bnd['raw']['dx'][c]:.2e}"
                  f"   one-pass variance y error {o:.2e} = {o / bnd['y'][c].item():.0f}x bound")
            if name in E.LN_OFFSET_CLASSES:
                assert o >= 100 * bnd["y"][c].item(), (D, name, o, bnd["y"][c].item())
            # the bounds are those of a right kernel: far from vacuous
            assert bnd["y"][c] <= (2e-2 if name == "tight1e3" else 4e-3), (D, name, bnd["y"][c])
        print(f"D {D:5d} dgamma {bnd['raw']['dgamma']:.2e} dbeta {bnd['raw']['dbeta']:.2e} colsum {bnd['raw']['colsum']:.2e} (per column, of the sum of magnitudes)")
        # constant rows: y is beta exactly and rstd = eps^-1/2
        const = cls == E.LN_CLASSES.index("const")
        assert torch.equal(y_ref[const], beta.double().expand(int(const.sum()), D))
