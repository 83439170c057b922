"""Input builders and fp64 references of the per-element numeric edge tests (test_numeric_edges_cpu.py proves the references and
inputs alone stay inside every bound; test_numeric_edges_gpu.py holds the HIP kernels to them).  A plain helper module.

Everything here is torch / numpy on the CPU (or on whatever device the inputs live on); nothing imports the HIP library."""
import math
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OP16 = {"bf16": torch.bfloat16, "f16": torch.float16}
F32_EPS = 2.0 ** -23  # one f32 ulp relative to the binade's lower end


# ============================================================================ A. GELU / GELU'
# Per-element absolute bounds csrc/common.h states for the fast-mode polynomials (gelu: times max(1, |x|)).  The f16 gelu' figure is the
# corrected one (6.0e-6 was stated; 6.02e-6 is reached at a finite half value in the f32 evaluation).
STATED = {("bf16", "gelu"): 2.4e-5, ("bf16", "dgelu"): 1.1e-4, ("f16", "gelu"): 1.9e-6, ("f16", "dgelu"): 6.1e-6}
# What the polynomials of csrc/common.h give on the CPU, evaluated in f32 in the kernel's own order (fma Horner in t, then 0.5 + xc r,
# then x * Phi), maximum over every sweep of this module (every finite 16-bit value of both formats, the seeded f32 sets, the dense
# sets).  test_numeric_edges_cpu.py re-measures them and asserts measured <= these <= STATED; the GPU assertion is these plus four
# f32 ulps of the value.  Measured: bf16 gelu 2.378e-05, bf16 gelu' 1.049e-04, f16 gelu 3.832e-07 (each gelu figure times max(1, |x|)), f16 gelu' 6.005e-06
# (6.02e-6 in numpy's unfused order, tools/fit_gelu_poly.py eval32).
CPU_F32 = {("bf16", "gelu"): 2.39e-5, ("bf16", "dgelu"): 1.05e-4, ("f16", "gelu"): 3.9e-7, ("f16", "dgelu"): 6.01e-6}
# precise mode (erff-based elementwise kernels).  gelu: the issue's figure.  gelu' = cdf + x pdf <= 1.13 has no stated bound; ours:
# erff to 2 ulp of a value <= 1 halved (1.2e-7), the rounding of 1 + erf halved (0.6e-7), x pdf <= 0.25 to a few ulp (0.6e-7), the
# final rounding of a value in [1, 2) (0.6e-7), their product with dy = 1 exact: 3.0e-7, held at 4e-7 (3.4 ulp at 1).
PRECISE_GELU = 1.5e-7
PRECISE_DGELU = 4e-7

_SQRT2 = math.sqrt(2.0)


def phi64(x):
    return 0.5 * torch.special.erfc(-x / _SQRT2)  # erfc: no cancellation in the negative tail


def gelu64(x):
    """x Phi(x) for a double tensor of finite x"""
    return x * phi64(x)


def dgelu64(x):
    """Phi(x) + x phi(x) for a double tensor of finite x"""
    return phi64(x) + x * torch.exp(-x * x / 2) / math.sqrt(2 * math.pi)


def ulp32(v):
    """the f32 ulp at |v| (double tensor in, double tensor out)"""
    a = v.abs().to(torch.float32)
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def header_tables():
    """{(pass, "PHI" | "DGELU"): (xmax, [coefficient texts])} parsed out of csrc/common.h"""
    src = open(os.path.join(ROOT, "simple_tad_amd", "csrc", "common.h")).read()
    src = src[src.index("fast-mode GELU for the GEMM epilogues"):]
    m = re.search(r"#ifdef TAD_OPND_F16(.*?)#else(.*?)#endif", src, re.S)
    out = {}
    for p, blk in (("f16", m.group(1)), ("bf16", m.group(2))):
        for name in ("PHI", "DGELU"):
            xmax = float(re.search(name + r"_XMAX = ([0-9.]+)f;", blk).group(1))
            n, body = re.search(name + r"_C\[(\d+)\] = \{([^}]*)\};", blk).groups()
            texts = [c.strip() for c in body.split(",")]
            assert len(texts) == int(n)
            out[(p, name)] = (xmax, texts)
    return out


def header_coefficients():
    """{(pass, name): (xmax, f32 array)}: the values the compiler sees"""
    return {k: (xmax, np.array([np.float32(t.rstrip("f")) for t in texts], np.float32)) for k, (xmax, texts) in header_tables().items()}


def fitter_tables():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import fit_gelu_poly
    finally:
        sys.path.pop(0)
    return fit_gelu_poly.tables()


def _fma32(a, b, c):
    # a, b, c f32 arrays: the product is exact in f64, the sum is rounded once to f64 and once more to f32 (a double rounding only
    # where the f64 sum lands within 2^-29 ulp of an f32 tie)
    return (a.astype(np.float64) * b.astype(np.float64) + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def half_plus_x_poly(x, xmax, c, f32):
    """0.5 + xc P(t) of csrc/common.h half_plus_x_poly2 for a numpy array x: in f64 with the f32 coefficients (the approximation's own
    error), or in f32 in the kernel's order (xc * xc rounded, t by one fma, fma Horner from the top coefficient, 0.5 + xc r by one fma)"""
    if not f32:
        x = x.astype(np.float64)
        xc = np.clip(x, -xmax, xmax)
        t = xc * xc * (2.0 / (xmax * xmax)) - 1.0
        r = np.full_like(t, np.float64(c[-1]))
        for k in c[-2::-1]:
            r = r * t + np.float64(k)
        return 0.5 + xc * r
    x = x.astype(np.float32)
    xc = np.clip(x, np.float32(-xmax), np.float32(xmax))
    t = _fma32(xc * xc, np.float32(np.float32(2.0) / (np.float32(xmax) * np.float32(xmax))), np.float32(-1.0))
    r = np.full_like(t, c[-1])
    for k in c[-2::-1]:
        r = _fma32(r, t, k)
    return _fma32(xc, r, np.float32(0.5))


def fast_gelu_cpu(x, fmt, f32=True):
    """gelu of the fast-mode epilogue on the CPU (numpy array in, f64 array out)"""
    xmax, c = header_coefficients()[(fmt, "PHI")]
    ph = half_plus_x_poly(x, xmax, c, f32)
    return (x.astype(np.float32) * ph).astype(np.float64) if f32 else x.astype(np.float64) * ph


def fast_dgelu_cpu(x, fmt, f32=True):
    xmax, c = header_coefficients()[(fmt, "DGELU")]
    return half_plus_x_poly(x, xmax, c, f32).astype(np.float64)


def op16_patterns(fmt):
    """all 65 536 bit patterns of the format: +-0, subnormals, +-inf, NaNs"""
    return torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(OP16[fmt])


def _f32_from_bits(b):
    return torch.as_tensor(np.asarray(b, dtype=np.uint32).view(np.float32).copy())


def f32_sweep(fmt, seed=20240607):
    """The f32 pre-activation sweep of one format, finite values only: (1) every finite 16-bit value; (2) seeded f32 values with full
    mantissas -- random bit patterns over all magnitudes, 3 z in the active range, log-uniform magnitudes over the half range with its
    subnormals and its overflow; (3) rounding cases for the 16-bit store -- ties, one bit below and above a tie, all-ones tails that
    round up into the next binade, the largest finite values and what lies beyond them; (4) dense sets around +-XMAX (4, 4.5, 5), +-0
    and the negative tail."""
    g = np.random.RandomState(seed)
    p = op16_patterns(fmt).float()
    parts = [p[torch.isfinite(p)]]
    bits = g.randint(0, 2 ** 32, size=16384, dtype=np.uint64).astype(np.uint32)
    parts.append(_f32_from_bits(bits))
    parts.append(torch.as_tensor((g.randn(8192) * 3).astype(np.float32)))
    mag = np.exp2(g.uniform(-27, 17.5, size=6144)).astype(np.float32) * np.where(g.rand(6144) < 0.5, -1, 1).astype(np.float32)
    parts.append(torch.as_tensor(mag))
    # (3) ties of the format: take finite 16-bit values, widen, set the dropped mantissa bits
    drop = 16 if fmt == "bf16" else 13
    base = parts[0][torch.as_tensor(g.randint(0, parts[0].numel(), size=3072))].numpy().view(np.uint32)
    half = np.uint32(1 << (drop - 1))
    for tail in (half, half - 1, half + 1, np.uint32((1 << drop) - 1), np.uint32(1)):
        parts.append(_f32_from_bits(base | tail))
    if fmt == "f16":  # ties between half subnormals (spacing 2^-24) and around the smallest one
        k = np.arange(0, 96, dtype=np.float64)
        sub = np.concatenate([(k + 0.5) * 2.0 ** -24, (k + 0.5) * 2.0 ** -24 * (1 + 2.0 ** -20), (k + 0.5) * 2.0 ** -24 * (1 - 2.0 ** -20)])
        parts.append(torch.as_tensor(np.concatenate([sub, -sub]).astype(np.float32)))
    edge = [65504.0, 65519.0, 65519.996, 65520.0, 65520.004, 65536.0, 1e5, 3.3895313892515355e38, 3.396e38, 3.4e38, 3.4028234663852886e38,
            2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0000001, 2.0 ** -126, 2.0 ** -133, 2.0 ** -134, 2.0 ** -149, 1e-40, 0.0]
    parts.append(torch.tensor(edge + [-v for v in edge], dtype=torch.float32))
    # (4)
    for x0 in (4.0, 4.5, 5.0):
        for s in (1.0, -1.0):
            c = np.float32(s * x0).view(np.uint32)
            parts.append(_f32_from_bits((c.astype(np.int64) + np.arange(-64, 65)).astype(np.uint32)))
    parts.append(torch.linspace(-9.5, -3.0, 4096))
    parts.append(torch.linspace(-6.0, 6.0, 4097))
    x = torch.cat([t.to(torch.float32) for t in parts])
    return x[torch.isfinite(x)].contiguous()


def bias_sweep(fmt, min_len=385 * 256):
    """f32_sweep plus +-inf and NaN, padded with further seeded values to at least `min_len` columns (more 256-column tiles than 1.5 per
    compute unit: the persistent plans run) and to a multiple of 256"""
    x = f32_sweep(fmt)
    x = torch.cat([x, torch.tensor([float("inf"), float("-inf"), float("nan")])])
    n = max(min_len, -(-x.numel() // 256) * 256)
    g = torch.Generator().manual_seed(99)
    return torch.cat([x, torch.randn(n - x.numel(), generator=g) * 2.5]).contiguous()


# ============================================================================ C. LayerNorm on hostile rows
LN_EPS = 1e-6
LN_DIMS = (128, 384, 768, 1024, 1280)
LN_CLASSES = ("plain", "offset1e3", "offset1e4", "tight1e3", "massive", "scale1e15", "subeps", "const")
LN_OFFSET_CLASSES = ("offset1e3", "offset1e4")  # z + offset: where a one-pass variance must exceed the bound 100-fold
LN_ROWS_PER_CLASS = 16
LN_FLOOR = 8 * F32_EPS  # 8 f32 ulps of the row scale


def ln_rows(D, seed=0):
    """x [129, D] f32 with the eight row classes interleaved (row i is class i % 8; the last row is one more plain row: a partial last
    block of the forward's four rows and of the backward's row chunks), gamma, beta, and the class index per row"""
    g = torch.Generator().manual_seed(1000 + D + seed)
    R = len(LN_CLASSES) * LN_ROWS_PER_CLASS + 1
    z = torch.randn(R, D, generator=g)
    cls = torch.arange(R) % len(LN_CLASSES)
    x = torch.empty(R, D)
    for i in range(R):
        c = LN_CLASSES[cls[i]]
        if c == "plain":
            x[i] = 2 * z[i] + 0.5
        elif c == "offset1e3":
            x[i] = z[i] + 1e3
        elif c == "offset1e4":
            x[i] = z[i] + 1e4
        elif c == "tight1e3":
            x[i] = 1e-2 * z[i] + 1e3
        elif c == "massive":
            x[i] = z[i]
            x[i, (7 * i) % D] = 3e3
            x[i, (7 * i + D // 2) % D] = -800.0
        elif c == "scale1e15":
            x[i] = 1e15 * z[i]
        elif c == "subeps":
            x[i] = 1e-20 * z[i]
        else:
            x[i] = 3.25
    gamma = 1.0 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(R, D, generator=g)
    dres = torch.randn(R, D, generator=g)
    return x, gamma, beta, dy, dres, cls


def ln_ref(x, gamma, beta, dy=None):
    """fp64 two-pass LayerNorm: y, mean, rstd (and dx, dgamma, dbeta for a given dy) of the f32 inputs as they are"""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    mean = x.mean(-1)
    xc = x - mean[:, None]
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1) + LN_EPS)
    xh = xc * rstd[:, None]
    y = xh * gamma + beta
    if dy is None:
        return y, mean, rstd
    dy = dy.double()
    t = dy * gamma
    c1, c2 = t.mean(-1, keepdim=True), (t * xh).mean(-1, keepdim=True)
    dx = rstd[:, None] * (t - c1 - xh * c2)
    return y, mean, rstd, dx, (dy * xh).sum(0), dy.sum(0), (dy * xh).abs().sum(0), dy.abs().sum(0)


def row_relmax(a, ref):
    """max |a - ref| / max |ref| per row (double tensors)"""
    return (a.double() - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-300)


def ln_torch_f32(x, gamma, beta, dy):
    """torch's own f32 LayerNorm on the CPU, forward and autograd backward"""
    xr = x.clone().requires_grad_()
    g, b = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    y, mean, rstd = torch.native_layer_norm(xr, (x.shape[-1],), g, b, LN_EPS)
    y.backward(dy)
    return y.detach(), mean.detach().reshape(-1), rstd.detach().reshape(-1), xr.grad, g.grad, b.grad


def ln_one_pass_f32(x, gamma, beta):
    """the defect the offset rows are there to catch: variance as E[x^2] - mean^2 in f32"""
    xn = x.numpy().astype(np.float32)
    D = np.float32(xn.shape[-1])
    mean = xn.sum(-1, dtype=np.float32) / D
    var = np.maximum((xn * xn).sum(-1, dtype=np.float32) / D - mean * mean, np.float32(0))
    rstd = np.float32(1) / np.sqrt(var + np.float32(LN_EPS))
    return torch.as_tensor((xn - mean[:, None]) * rstd[:, None] * gamma.numpy() + beta.numpy())


def ln_bounds(D):
    """Per-class bounds of one D from torch's f32 error on these same rows: 4x its class maximum (the order of a wave's sum differs from
    torch's -- a small constant), floored at 8 f32 ulps.  Returns {what: tensor[classes]} for y, rstd, dx (per row, relative to the row
    maximum) and scalars for dgamma / dbeta / colsum (per column, relative to the column's sum of magnitudes), plus torch's raw figures."""
    x, gamma, beta, dy, dres, cls = ln_rows(D)
    y, mean, rstd, dx, dg, db, dg_abs, db_abs = ln_ref(x, gamma, beta, dy)
    ty, tmean, trstd, tdx, tdg, tdb = ln_torch_f32(x, gamma, beta, dy)
    raw = {"y": row_relmax(ty, y), "rstd": (trstd.double() - rstd).abs() / rstd, "dx": row_relmax(tdx, dx)}
    out = {"raw": {}}
    for k, v in raw.items():
        per = torch.stack([v[cls == c].max() for c in range(len(LN_CLASSES))])
        out["raw"][k] = per
        out[k] = (4 * per).clamp_min(LN_FLOOR)
    for k, t, r, s in (("dgamma", tdg, dg, dg_abs), ("dbeta", tdb, db, db_abs)):
        e = ((t.double() - r).abs() / s).max()
        out["raw"][k] = e
        out[k] = max(4 * float(e), LN_FLOOR)
    # colsum(dx + dres): torch's f32 sum over the rows of its own f32 dx + dres
    cs_ref, cs_abs = (dx + dres.double()).sum(0), (dx + dres.double()).abs().sum(0)
    e = (((tdx + dres).sum(0).double() - cs_ref).abs() / cs_abs).max()
    out["raw"]["colsum"] = e
    out["colsum"] = max(4 * float(e), LN_FLOOR)
    return out


def mean_bound(x):
    """|mean - fp64 mean| per row: any summation tree of depth h errs by at most h u sum|x|; a wave's tree over D <= 1280 values is at most
    ceil(log2 D) + 3 deep (per-lane partial sums, six butterfly steps); plus one rounding of the quotient -- in all
    (ceil(log2 D) + 3) 2^-24 mean|x| + one f32 ulp of |mean|"""
    D = x.shape[-1]
    xd = x.double()
    return (math.ceil(math.log2(D)) + 3) * 2.0 ** -24 * xd.abs().mean(-1) + ulp32(xd.mean(-1))


# ============================================================================ D. planted non-finite values
NONFINITE = (float("inf"), float("nan"))


def plant(t, pos, value):
    """a copy of t with `value` at index tuple `pos`"""
    t = t.clone()
    t[pos] = value
    return t
