"""Per-element yardstick of the attention kernels (csrc/attn_fwd.hip, attn_bwd.hip, attn_f32.hip): the exact fp64 reference, an a-priori
error bound for EVERY output element built from the kernels' stated rounding points, a rounding-model emulation of the same dataflow
(fp64 with explicit 16-bit roundings; four planted defects), and the three input families the bound tests run on.  A plain helper next to
attn_util.py; everything is torch and runs on whatever device its inputs live on (the GPU tests keep the fp64 work on the device).

Layouts: the kernels' packed rows (qkv [B*N, 3*H*d] = [B,N,3,H,d], out / dout [B*N, H*d], lse [B,H,N]); everything in here is
[B,H,N,*] float64 (heads(), qkv_heads(), out_rows() convert).

THE BOUNDS.  u = unit roundoff of the operand format (bf16 2^-8, IEEE half 2^-11, f32 kernels 0), eta = half its smallest subnormal
(bf16 0, half 2^-25, f32 0), P = softmax, Pd = the dropped P (keep ? P / (1 - p) : 0; = P without dropout), dP = dO V^T (through the
dropout), Delta = rowsum(dO o out), dS = P o (dP - Delta).  First order in u; the tests allow 1.0625 x the bound, the 1/16 standing for
the second-order terms (u relative to the bound).

Leading (16-bit) terms, with the rounding point each comes from:
  out (f32)   2u sum_j Pd_ij |V_jc| + eta sum_j |V_jc| + eta N |out_ic|
                 P is rounded to 16 bits for the P V product (attn_fwd.hip: pf = (op16_t)pe) and the row sum is taken of the SAME rounded
                 P (the `sel` matrix product) -- u in the numerator, u in the denominator, |out| <= sum_j Pd |V|.  With dropout the
                 denominator is the f32 sum of the unrounded P: the same bound holds.  P is rounded at the running offset m_run, which
                 never lies above the row's maximum and never more than RESCALE_THR = 8 log2 units below it: the largest rounded P of a row
                 is >= 1, so the row sum is >= 1 and a half-format subnormal P (absolute error eta) costs eta per key after normalisation
                 -- in the numerator (eta sum_j |V_jc|) and in the denominator (eta N relative, i.e. eta N |out_ic|).
  out (16 bit) the above + u |out| + eta (the store's rounding);  out + out_lo: the above + u^2 |out| + eta (out_lo is the 16-bit rounding of
                 the exactly representable residual)
  lse         u (no dropout: the rounded row sum; dropout: 0) + eta N
  dV          u (sum_i Pd_ij |dO_ic| + |dV_jc|) + eta (sum_i |dO_ic| + 1)      (attn_bwd.hip, dK/dV kernel: pack8(pm), the store)
  dQ          u (scale sum_j |dS_ij| |K_jc| + |dQ_ic|) + eta (scale sum_j |K_jc| + 1)
  dK          u (scale sum_i |dS_ij| |Q_ic| + |dK_jc|) + eta (scale sum_i |Q_ic| + 1)
                 dS is rounded to 16 bits UNSCALED in both kernels (pack8(ds)); `scale` multiplies the f32 accumulator in the epilogue
                 (dQ: dq * scale; dK: dk * scale, or dk * ln2 where the staged q carries scale * log2e).  The absolute error eta of a
                 subnormal dS therefore reaches the output times scale |K_jc| (scale |Q_ic|): eta's factor carries `scale`, as u's does.
  An output element whose bound is otherwise 0 and whose exact value is 0 is a sum of exact zeros in the kernel: the store's eta is only
  charged where the rest of the bound or the exact value is non-zero, so such elements must come out as exactly 0.0.

f32 terms (e = 2^-24; all of them are the WHOLE bound of the f32 kernels, where u = eta = 0):
  accumulation   n products summed in f32 cost gamma_n = n e times the sum of the absolute products (Higham, Accuracy and Stability of
                 Numerical Algorithms, eq. 3.5 to first order).  Scores and dP: n = d plus a few for the scale factors and the initial
                 accumulator (-Delta, -lse/scale in the dK/dV kernel, which is why |lse_i| and |Delta_i| stand next to the absolute
                 products); Delta: n = d + 2; second products: n = N plus two per tile for the rescale multiplications of the online
                 softmax (the factor alpha itself multiplies numerator and denominator alike and cancels) plus the epilogue.
  exponential    v_exp_f32 is good to one ulp and its f32 argument carries half an ulp of its own magnitude: (ln2 |x| + 1) 2^-23 relative
                 for the log2-unit argument x (AMD CDNA ISA guide, V_EXP_F32: 1 ULP).  Forward: ln2 |x| <= (rowmax_i - S_ij) + 8 ln2;
                 backward: ln2 |x| = |S_ij - lse_i| = |ln P_ij|.  Results below 2^-126 flush to zero: an absolute 2^-126 per P.
  scale factors  the products with scale * log2e, lse * log2e, -lse / scale, m_run * c: 2^-22 (|S_ij| + |lse_i| or |rowmax_i|) on the
                 exponent's argument in natural units.
  lse            its logarithm (v_log_f32: one ulp, absolute 2^-21 near l = 1) and the sum m + log l: 2^-22 (|lse| + |rowmax| + 8 ln2 + ln N).
  a given lse    the backward recomputes P = exp(S - lse) from the lse it is HANDED: a row error delta_i = |lse_given - lse_exact| enters
                 every P_ij, hence dS_ij and the dropped P of dV, as a relative error delta_i.
  a given out    the backward computes Delta from the out (+ out_lo) it is handed: dDelta_i = |rowsum(dO o (out + out_lo)) - Delta_exact|
                 (+ gamma_{d+2} of its absolute products) enters dS_ij as P_ij dDelta_i.
bwd_bounds() computes delta_i and dDelta_i from the operands it is given, so one function serves the backward fed exact operands and the
production chain fed the forward kernel's own (lse, out[, out_lo]).
"""
import math
from collections import namedtuple

import torch

import golden_recipe as R
from attn_util import LOG2E, prescaled_pair

LN2 = math.log(2.0)
E24 = 2.0 ** -24
ETA32 = 2.0 ** -126
SLACK = 1.0625          # 1 + 1/16: second-order terms
RESCALE_THR = 8.0       # attn_fwd.hip: log2 units
FORMATS = {"bf16": (torch.bfloat16, 2.0 ** -8, 0.0), "f16": (torch.float16, 2.0 ** -11, 2.0 ** -25), "f32": (torch.float32, 0.0, 0.0)}
DEFECTS = ("masked_key", "dead_query_row", "out_lo_ignored", "lse_row_off")  # (a) .. (d)
LEAK = 2.0 ** -12


def gam(n):
    return n * E24


def rounder(fmt):
    """round-trip through the format (via f32, as the kernels' values are f32 before they are rounded); keeps dtype and device"""
    dt = FORMATS[fmt][0]
    return lambda t: t.to(torch.float32).to(dt).to(t.dtype)


# ------------------------------------------------------------------------------------------------------------------ layouts
def heads(x, B, N, H, d):
    """[B*N, H*d] rows -> [B,H,N,d] float64"""
    return x.double().reshape(B, N, H, d).permute(0, 2, 1, 3)


def qkv_heads(x, B, N, H, d):
    """[B*N, 3*H*d] rows -> (q, k, v) each [B,H,N,d] float64"""
    x5 = x.double().reshape(B, N, 3, H, d)
    return tuple(x5[:, :, i].permute(0, 2, 1, 3) for i in range(3))


def out_rows(x):
    """[B,H,N,d] -> [B*N, H*d]"""
    B, H, N, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * N, H * d)


# ------------------------------------------------------------------------------------------------------------------ inputs
Inputs = namedtuple("Inputs", "opnd qkv dout scale B N H d fmt prescaled")
FAMILIES = ("spread", "spike", "probe")


def _pow2(g, shape, lo, hi):
    return torch.pow(2.0, torch.randint(lo, hi + 1, shape, generator=g).float())


def make_inputs(family, fmt, d, N, seed=0, prescaled=False):
    """B = H = 2 (a clip boundary and a head stride inside the grid); every value exact in the operand format.
      opnd  [B*N, 3*H*d] f32: the kernel's qkv (its q third carries scale * log2e when `prescaled`)
      qkv   [B*N, 3*H*d] f64: what the reference sees (prescaled_pair: the same q, k, v)
      dout  [B*N, H*d] f32
    spread: Gaussians times per-token powers of two (q 2^-2..2^2: from uniform to nearly one-hot rows, k 2^-1..2^1, v and dout 2^-6..2^2)
    spike : test_attention_softmax_spike's operands in every (clip, head) (late maxima in tiles 0 and 2, rows far below 0, |lse| ~ 100);
            token indices beyond N wrap around
    probe : N <= d; V[j] = e_j in clip 0 and e_{d-1-j} in clip 1, dout one-hot the same way: out[i,c] = P[i,c] (clip 1: P[i,d-1-c]),
            columns that meet no key have bound 0 and must be exactly 0.0 (what clip 1 would leak into clip 0 lands there), dV reads
            P transposed"""
    B = H = 2
    scale = d ** -0.5
    rnd = rounder(fmt)
    g = torch.Generator().manual_seed(R._seed_for(f"attn_bounds.{family}.{d}.{N}", seed))
    qkv = torch.randn(B, N, 3, H, d, generator=g)
    dout = torch.randn(B, N, H, d, generator=g)
    if family == "spread":
        for i, (lo, hi) in enumerate(((-2, 2), (-1, 1), (-6, 2))):
            qkv[:, :, i] *= _pow2(g, (B, N, 1, 1), lo, hi)
        dout *= _pow2(g, (B, N, 1, 1), -6, 2)
    elif family == "spike":
        qkv = R.tensor_for("att.spike", (B, N, 3, H, d), seed=seed, scale=1.0)
        w = lambda i: i % N  # noqa: E731
        one = torch.ones(d)
        for b in range(B):
            for h in range(H):
                q4 = qkv[b, :, :, h]
                q4[w(5), 1] = q4[w(17), 0] * 6.0
                q4[w(190), 1] = q4[w(17), 0] * 12.0
                q4[w(130), 1] = q4[w(64), 0] * 10.0
                q4[:, 1] += 3.0 * one
                q4[w(40), 0] = -4.0 * one
                q4[w(41), 0] = -4.0 * one
                q4[w(100), 1] = -2.0 * one
    elif family == "probe":
        assert N <= d, "probe: one V column per key"
        eye = torch.eye(d)[:N]
        for b, pat in enumerate((eye, eye.flip(-1))):
            qkv[b, :, 2] = pat[:, None, :]
            dout[b] = pat[:, None, :]
    else:
        raise ValueError(family)
    qkv = rnd(qkv.reshape(B * N, 3 * H * d))
    dout = rnd(dout.reshape(B * N, H * d))
    if prescaled:
        opnd, q64 = prescaled_pair(qkv, B, N, H, scale, rnd, d=d)
    else:
        opnd, q64 = qkv, qkv.double()
    return Inputs(opnd, q64, dout, scale, B, N, H, d, fmt, prescaled)


# ------------------------------------------------------------------------------------------------------------------ reference
class Ref(dict):
    __getattr__ = dict.__getitem__


def reference(qkv, dout, scale, B, N, H, d, keep=None, p=0.0):
    """exact attention forward and backward in float64.  qkv [B*N, 3*H*d], dout [B*N, H*d] (any float dtype); keep: the oracle's
    dropout keep mask [B,H,N,N] (bool) with probability p.  Everything [B,H,N,*] float64."""
    q, k, v = qkv_heads(qkv, B, N, H, d)
    dO = heads(dout, B, N, H, d)
    S = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    kf = torch.ones_like(P) if keep is None else keep.to(P.device).double() / (1.0 - p)
    Pd = P * kf
    out = Pd @ v
    dPd = (dO @ v.transpose(-1, -2)) * kf       # d loss / d P
    delta = (dO * out).sum(-1)
    dS = P * (dPd - delta[..., None])
    return Ref(q=q, k=k, v=v, dO=dO, S=S, lse=lse, P=P, Pd=Pd, kf=kf, out=out, dPd=dPd, delta=delta, dS=dS,
               dq=scale * (dS @ k), dk=scale * (dS.transpose(-1, -2) @ q), dv=Pd.transpose(-1, -2) @ dO,
               scale=scale, N=N, d=d, drop=keep is not None)


# ------------------------------------------------------------------------------------------------------------------ bounds
def _nz(*ts):
    """1.0 where any of the tensors is non-zero (the store's eta is only charged there)"""
    m = ts[0] != 0
    for t in ts[1:]:
        m = m | (t != 0)
    return m.double()


def fwd_bounds(r, fmt, f32_terms=True):
    """{"out32", "out16", "sum16" (out + out_lo), "lse"}: bounds on |kernel - reference|, shapes of r.out / r.lse.  f32_terms=False: the
    leading 16-bit terms alone (what the emulation, which rounds nowhere else, must already meet)"""
    _, u, eta = FORMATS[fmt]
    f = 1.0 if f32_terms else 0.0
    N, d = r.N, r.d
    aV, aout = r.v.abs(), r.out.abs()
    smax = r.S.amax(-1)
    A = r.q.abs() @ r.k.abs().transpose(-1, -2)
    ef = gam(d + 2) * r.scale * A + 2.0 ** -22 * (r.S.abs() + smax.abs()[..., None]) + ((smax[..., None] - r.S) + 8 * LN2 + 1.0) * 2.0 ** -23
    n2 = N + 2 * ((N + 31) // 32) + 8
    PV = r.Pd @ aV
    colV = aV.sum(-2, keepdim=True)
    Pef = (r.P * ef).sum(-1)
    b32 = (2 * u * PV + eta * colV + eta * N * aout
           + f * ((r.Pd * ef) @ aV + aout * Pef[..., None] + gam(n2) * (PV + aout) + ETA32 * colV))
    b16 = b32 + u * aout + eta * _nz(b32, aout)
    bsum = b32 + u * u * aout + eta * _nz(b32, aout)
    blse = ((0.0 if r.drop else u) + eta * N + f * (Pef + gam(n2) + 2.0 ** -21
                                                    + 2.0 ** -22 * (r.lse.abs() + smax.abs() + 8 * LN2 + math.log(N))))
    return dict(out32=b32, out16=b16, sum16=bsum, lse=blse)


def bwd_bounds(r, fmt, lse, out, out_lo=None, f32_terms=True):
    """{"dq", "dk", "dv"}: bounds on |kernel - reference| for a backward HANDED lse [B,H,N], out and (optionally) out_lo [B,H,N,d]: the
    exact ones, or the forward kernel's own.  f32_terms: as in fwd_bounds"""
    _, u, eta = FORMATS[fmt]
    f = 1.0 if f32_terms else 0.0
    N, d, scale = r.N, r.d, r.scale
    o = out.double() if out_lo is None else out.double() + out_lo.double()
    dDelta = ((r.dO * o).sum(-1) - r.delta).abs() + f * gam(d + 2) * (r.dO * o).abs().sum(-1)
    dl = (lse.double() - r.lse).abs()
    aQ, aK, aV, aO = r.q.abs(), r.k.abs(), r.v.abs(), r.dO.abs()
    A = aQ @ aK.transpose(-1, -2)
    la = r.lse.abs()[..., None]
    eP = dl[..., None] + f * (gam(d + 3) * (scale * A + la) + 2.0 ** -22 * (la + r.S.abs()) + ((r.S - r.lse[..., None]).abs() + 1.0) * 2.0 ** -23)
    G = (aO @ aV.transpose(-1, -2)) * r.kf
    ad = r.delta.abs()[..., None]
    edP = f * gam(d + 4) * (G + ad) + dDelta[..., None]
    adS = r.dS.abs()
    e23 = f * 2.0 ** -23
    edS = adS * (eP + u + e23) + r.P * edP + eta + f * ETA32 * (G + ad)
    n2 = f * (N + 2 * ((N + 31) // 32) + 8)
    e1 = u + 2 * e23
    bq = scale * (edS @ aK) + gam(n2) * scale * (adS @ aK)
    bq = bq + e1 * r.dq.abs() + eta * _nz(bq, r.dq)
    bk = scale * (edS.transpose(-1, -2) @ aQ) + gam(n2) * scale * (adS.transpose(-1, -2) @ aQ)
    bk = bk + e1 * r.dk.abs() + eta * _nz(bk, r.dk)
    PdT = r.Pd.transpose(-1, -2)
    bv = ((r.Pd * (eP + u + e23)).transpose(-1, -2) @ aO + (eta + f * ETA32) * aO.sum(-2, keepdim=True) + gam(n2) * (PdT @ aO))
    bv = bv + e1 * r.dv.abs() + eta * _nz(bv, r.dv)
    return dict(dq=bq, dk=bk, dv=bv)


def worst(got, ref, bound):
    """max over the elements of |got - ref| / bound (0 / 0 = 0, x / 0 = inf), as a 0-d tensor on the inputs' device; a non-finite `got`
    counts as inf"""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(torch.isfinite(got.double()), ratio, torch.full_like(ratio, float("inf")))
    return ratio.max()


def locate(got, ref, bound):
    """(index tuple, ratio) of the worst element: (clip, head, row[, column])"""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(torch.isfinite(got.double()), ratio, torch.full_like(ratio, float("inf")))
    i = int(ratio.argmax())
    idx = []
    for s in reversed(ratio.shape):
        idx.append(i % s)
        i //= s
    return tuple(reversed(idx)), float(ratio.max())


# ------------------------------------------------------------------------------------------------------------------ emulation
def _next_clip_row0(x):
    """[B,H,N,d] -> [B,H,d]: row 0 of the NEXT clip (what lies behind a clip's last row in the packed tensor), zeros behind the last clip"""
    nxt = torch.zeros_like(x[:, :, 0])
    nxt[:-1] = x[1:, :, 0]
    return nxt


def emulate_fwd(r, fmt, defect=None):
    """attn_fwd.hip's dataflow in float64 with its 16-bit roundings: 64-key tiles, the running offset moved for a whole 32-row wave when any
    of its rows exceeds it by more than RESCALE_THR log2 units, P rounded to 16 bits at that offset, the row sum taken of the rounded P
    (of the unrounded one under dropout).  Returns (out32, out16, out_lo, lse).
    defect "masked_key": one key behind the sequence (the next clip's first token) enters numerator and denominator with relative weight 2^-12"""
    rnd = rounder(fmt)
    B, H, N, d = r.q.shape
    S2 = r.S * LOG2E
    m = torch.full((B, H, N), -1e30, dtype=torch.float64)
    l = torch.zeros(B, H, N, dtype=torch.float64)
    o = torch.zeros(B, H, N, d, dtype=torch.float64)
    G = (N + 31) // 32
    for t0 in range(0, N, 64):
        cols = slice(t0, min(N, t0 + 64))
        mt = S2[..., cols].amax(-1)
        trig = torch.zeros(B, H, G * 32, dtype=torch.bool)
        trig[..., :N] = (mt - m) > RESCALE_THR
        trig = trig.reshape(B, H, G, 32).any(-1).repeat_interleave(32, -1)[..., :N]
        m_new = torch.where(trig, torch.maximum(m, mt), m)
        alpha = torch.exp2(m - m_new)
        m, l, o = m_new, l * alpha, o * alpha[..., None]
        pe = torch.exp2(S2[..., cols] - m[..., None])
        if r.drop:
            pd = rnd(pe * r.kf[..., cols])
            l = l + pe.sum(-1)
        else:
            pd = rnd(pe)
            l = l + pd.sum(-1)
        o = o + pd @ r.v[:, :, cols]
    if defect == "masked_key" and N % 64:
        w = LEAK * l
        o = o + w[..., None] * _next_clip_row0(r.v)[:, :, None, :]
        l = l + w
    out32 = o / l[..., None]
    out16 = rnd(out32)
    return out32, out16, rnd(out32 - out16), (m + torch.log2(l)) * LN2


def emulate_bwd(r, fmt, lse, out, out_lo=None, defect=None):
    """attn_bwd.hip's dataflow in float64 with its 16-bit roundings: Delta from the out (+ out_lo) handed in, P = exp(S - lse) from the lse
    handed in, dS rounded to 16 bits unscaled (both kernels), the dropped P rounded for dV, the three outputs rounded.  Returns (dq, dk, dv).
    defects: "dead_query_row": the first row behind the sequence (the next clip's first token) enters dK / dV with P = 2^-12;
    "out_lo_ignored": Delta is taken of `out` alone; "lse_row_off": one row's lse is read 2^-7 too large"""
    rnd = rounder(fmt)
    o = out.double() if (out_lo is None or defect == "out_lo_ignored") else out.double() + out_lo.double()
    delta = (r.dO * o).sum(-1)
    lse = lse.double().clone()
    if defect == "lse_row_off":
        lse[:, :, r.N // 2] += 2.0 ** -7
    P = torch.exp(r.S - lse[..., None])
    dS16 = rnd(P * (r.dPd - delta[..., None]))
    dq = r.scale * (dS16 @ r.k)
    dk = r.scale * (dS16.transpose(-1, -2) @ r.q)
    dv = rnd(P * r.kf).transpose(-1, -2) @ r.dO
    if defect == "dead_query_row" and r.N % 64:
        qx, gx = _next_clip_row0(r.q), _next_clip_row0(r.dO)                     # [B,H,d]
        dsx = LEAK * torch.einsum("bhc,bhjc->bhj", gx, r.v)                      # dS of that row: P (dP - 0)
        dv = dv + LEAK * gx[:, :, None, :]
        dk = dk + r.scale * dsx[..., None] * qx[:, :, None, :]
    return rnd(dq), rnd(dk), rnd(dv)
