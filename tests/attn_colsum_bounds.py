"""Per-element yardstick of tad_attn_colsum (csrc/attn_colsum.hip), next to attn_bounds.py whose inputs, reference and terms it reuses: the
fp64 reference R_j = sum_i w_i exp(S_ij - lse_i) on the SAME stored operands and the lse the kernel is HANDED, an a-priori error bound for
every output element, the weight vectors the tests run on, and an f32 torch emulation of the kernel's data flow with four planted defects.

THE BOUND.  P is recomputed from a handed lse exactly as the attention backward does it, so its relative error is attn_bounds.bwd_bounds' eP
without the row error of the lse (the reference uses the handed lse too):
    eP_ij = gam(d + 3) (scale A_ij + |lse_i|)      f32 accumulation of the d products of a score (A = |q| |k|^T)
          + 2^-22 (|lse_i| + |S_ij|)               the factors scale * log2e and lse * log2e
          + (|S_ij - lse_i| + 1) 2^-23             v_exp_f32 (one ulp) and the half ulp of its argument
    bound_j = sum_i |w_i| P_ij (eP_ij + 2^-23)     (2^-23: the product w_i P_ij)
            + gam(N + 2 ceil(N / 32) + 8) sum_i |w_i| P_ij     the f32 sums (every order of at most that many additions)
            + ETA32 sum_i |w_i|                    a P below 2^-126 flushes to zero
P and the sums stay f32 in the kernel: no term carries the unit roundoff of the 16-bit operand format.  Tests allow SLACK x the bound.
"""
import math

import torch

from attn_bounds import ETA32, FORMATS, SLACK, gam, make_inputs, reference, worst  # noqa: F401  (re-exported for the tests)
from attn_util import LOG2E

WEIGHTS = ("uniform", "onehot_first", "onehot_last", "pow2", "signed")
DEFECTS = ("ragged_row_counted", "lse_of_other_head", "w_of_other_clip", "last_key_block_skipped")


def weights(kind, B, N, seed=0):
    """w [B,N] f32 (host).  uniform 1/N; one-hot at i = 0 / i = N - 1 (the output is one row of P; the last row of a ragged tile is
    pinned); random non-negative powers of two 2^-8 .. 2^2; signed Gaussians.  The random ones differ between the clips."""
    g = torch.Generator().manual_seed(977 * N + 31 * seed + WEIGHTS.index(kind))
    if kind == "uniform":
        return torch.full((B, N), 1.0 / N, dtype=torch.float32)
    if kind in ("onehot_first", "onehot_last"):
        w = torch.zeros(B, N, dtype=torch.float32)
        w[:, 0 if kind == "onehot_first" else N - 1] = 1.0
        return w
    if kind == "pow2":
        return torch.pow(2.0, torch.randint(-8, 3, (B, N), generator=g).float())
    if kind == "signed":
        return torch.randn(B, N, generator=g)
    raise ValueError(kind)


def colsum_reference(r, w, lse):
    """R [B,H,N] float64 from attn_bounds.reference's scores: sum_i w_i exp(S_ij - lse_i) with the lse [B,H,N] as handed to the kernel"""
    P = torch.exp(r.S - lse.double()[..., None])
    return torch.einsum("bi,bhij->bhj", w.double(), P)


def colsum_bound(r, w, lse):
    """bound on |kernel - colsum_reference| per element [B,H,N] (module docstring)"""
    N, d, scale = r.N, r.d, r.scale
    l = lse.double()
    la = l.abs()[..., None]
    P = torch.exp(r.S - l[..., None])
    A = r.q.abs() @ r.k.abs().transpose(-1, -2)
    eP = gam(d + 3) * (scale * A + la) + 2.0 ** -22 * (la + r.S.abs()) + ((r.S - l[..., None]).abs() + 1.0) * 2.0 ** -23
    aw = w.double().abs()
    wP = torch.einsum("bi,bhij->bhj", aw, P)
    n2 = N + 2 * ((N + 31) // 32) + 8
    return torch.einsum("bi,bhij->bhj", aw, P * (eP + 2.0 ** -23)) + gam(n2) * wP + ETA32 * aw.sum(-1)[:, None, None]


def _fma(a, b, c):
    """f32 fused multiply-add (the exact product and sum, rounded once)"""
    return (a.double() * b.double() + c.double()).float()


def emulate(opnd, lse, w, B, N, H, d, scale, prescaled, defect=None):
    """The kernel's data flow in f32 torch: opnd [B*N, 3*H*d] (values exact in the operand format; the q third pre-scaled when
    `prescaled`), lse [B,H,N] and w [B,N] f32 -> out [B,H,N] f32.  Key blocks of 128; 64-row query tiles as two half tiles of 32 rows; f32
    scores; P = exp2 of one f32 argument; rows >= N of the ragged half tile excluded by SELECTION (their P is NaN in here, as it may be in the
    kernel); row rho of a half tile goes to the chain (lane half (rho >> 2) & 1, register group rho >> 3), in ascending order; the four
    chains are added pairwise, then the two lane halves.
    defects: "ragged_row_counted": the rows behind the sequence are clamped to row N - 1 and NOT deselected; "lse_of_other_head": lse[b, h ^ 1];
    "w_of_other_clip": w[b ^ 1]; "last_key_block_skipped": the last block of 128 keys is never computed (its outputs stay 0)"""
    f32 = torch.float32
    x5 = opnd.to(f32).reshape(B, N, 3, H, d)
    q, k = x5[:, :, 0].permute(0, 2, 1, 3), x5[:, :, 1].permute(0, 2, 1, 3)  # [B,H,N,d]
    lse, w = lse.to(f32), w.to(f32)
    if defect == "lse_of_other_head":
        lse = lse.flip(1)
    if defect == "w_of_other_clip":
        w = w.flip(0)
    log2e = torch.tensor(LOG2E, dtype=f32)
    c = torch.tensor(scale, dtype=f32) * log2e
    acc = torch.zeros(B, H, 2, 4, N, dtype=f32)
    for row0 in range(0, N, 32):
        rows = torch.arange(row0, row0 + 32)
        valid = rows < N
        rc = rows.clamp(max=N - 1)
        s = (q[:, :, rc].double() @ k.double().transpose(-1, -2)).float()  # [B,H,32,N]  (f32 accumulation: covered by gam(d + 3))
        lse2 = (lse[:, :, rc] * log2e)[..., None]
        p = torch.exp2(s - lse2) if prescaled else torch.exp2(_fma(s, c, -lse2))
        ww = w[:, rc]
        if defect != "ragged_row_counted":
            p = torch.where(valid[None, None, :, None], p, torch.full_like(p, float("nan")))  # what lies behind the sequence may be anything ...
            p = torch.where(valid[None, None, :, None], p, torch.zeros_like(p))               # ... and is deselected, not multiplied by 0
            ww = torch.where(valid[None, :], ww, torch.zeros_like(ww))
        for rho in range(32):
            h5, r4 = (rho >> 2) & 1, rho >> 3
            acc[:, :, h5, r4] = _fma(ww[:, None, rho, None].expand(B, H, N), p[:, :, rho], acc[:, :, h5, r4])
    mine = (acc[:, :, :, 0] + acc[:, :, :, 1]) + (acc[:, :, :, 2] + acc[:, :, :, 3])
    out = mine[:, :, 0] + mine[:, :, 1]
    if defect == "last_key_block_skipped":
        out[:, :, (N - 1) // 128 * 128:] = 0.0
    return out


def rollout_tolerance(r, lse_kernel, N, d):
    """eps_l of one layer for the rollout's compounded relative error (tests/test_explain_gpu.py):
    max_ij (dl_i + eP_ij + 2^-23) + gam(N + 2 ceil(N / 32) + 8) + 2^-22, dl_i = |lse_kernel - lse_fp64|, eP on the kernel's lse"""
    l = lse_kernel.double()
    la = l.abs()[..., None]
    A = r.q.abs() @ r.k.abs().transpose(-1, -2)
    eP = gam(d + 3) * (r.scale * A + la) + 2.0 ** -22 * (la + r.S.abs()) + ((r.S - l[..., None]).abs() + 1.0) * 2.0 ** -23
    dl = (l - r.lse).abs()[..., None]
    return float((dl + eP + 2.0 ** -23).max()) + gam(N + 2 * math.ceil(N / 32) + 8) + 2.0 ** -22
