"""The attention kernels (csrc/attn_fwd.hip, attn_bwd.hip, attn_f32.hip) against the fp64 reference at EVERY output element, each held to
its own a-priori rounding bound (tests/attn_bounds.py; SLACK = 1.0625 x the first-order bound): every ragged length from 1 to 130 and the
tile-count edges up to 257, peaked and spread softmax rows, exact zeros, dropout with the regenerated mask -- forward (f32 and 16-bit
output, out_lo, lse) and backward (on exact operands and on the forward's own outputs, with and without out_lo); and clip isolation:
nothing non-finite in clip 1 changes one bit of clip 0.  The fp64 reference and the bounds are computed on the device.

Each test prints the worst error / bound it saw per output ("RATIO ..." lines: measurements, recorded in DESIGN.md section 4, never asserted --
the assertion threshold is the derived one)."""
import pytest
import torch

import attn_bounds as AB
import edge_cases as E
from oracle import vit_oracle as O
from test_numeric_edges_gpu import ULP16, check_planted

pytestmark = pytest.mark.gpu

# every length up to one past the 128-row block, then the 64-key tile edges of three, four and five tiles (both ring slots, the last-tile branch)
SWEEP = tuple(range(1, 131)) + (191, 192, 193, 255, 256, 257)


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import _lib, kernels
    _lib.load()
    return kernels


def launches(K, x, p=0.0, seed=0):
    """every launch of one case: [(name, got, ref, bound)] with got / ref / bound [B,H,N,*] (lse: [B,H,N]) on the device"""
    B, N, H, d, fmt = x.B, x.N, x.H, x.d, x.fmt
    keep = O.attention_dropout_keep(B, H, N, p, seed).cuda() if p else None
    r = AB.reference(x.qkv.cuda(), x.dout.cuda(), x.scale, B, N, H, d, keep=keep, p=p)
    fb = AB.fwd_bounds(r, fmt)
    hd = lambda t: AB.heads(t, B, N, H, d)  # noqa: E731
    drop = dict(drop_p=p, seed=seed)
    checks = []

    def grads(tag, dqkv, lse, out, lo=None):
        bb = AB.bwd_bounds(r, fmt, lse, hd(out), None if lo is None else hd(lo))
        for nm, g in zip(("dq", "dk", "dv"), AB.qkv_heads(dqkv, B, N, H, d)):
            checks.append((f"{nm}.{tag}", g, r[nm], bb[nm]))

    if fmt == "f32":
        qd, gd = x.opnd.cuda(), x.dout.cuda()
        out, lse = K.attn_fwd_f32(qd, B, N, H, x.scale, want_lse=True, d=d, **drop)
        checks += [("out32", hd(out), r.out, fb["out32"]), ("lse", lse, r.lse, fb["lse"])]
        out_e, lse_e = AB.out_rows(r.out).float().contiguous(), r.lse.float().contiguous()
        grads("exact", K.attn_bwd_f32(qd, out_e, gd, lse_e, B, N, H, x.scale, d=d, **drop), lse_e, out_e)
        grads("chain", K.attn_bwd_f32(qd, out, gd, lse, B, N, H, x.scale, d=d, **drop), lse, out)
        return checks
    dt = AB.FORMATS[fmt][0]
    qd, gd = x.opnd.cuda().to(dt), x.dout.cuda().to(dt)
    kw = dict(q_prescaled=x.prescaled, d=d, **drop)
    out32, lse32 = K.attn_fwd(qd, B, N, H, x.scale, out_dtype=torch.float32, **kw)
    checks += [("out32", hd(out32), r.out, fb["out32"]), ("lse", lse32, r.lse, fb["lse"])]
    out16, lse, lo = K.attn_fwd(qd, B, N, H, x.scale, want_lo=True, **kw)
    checks += [("out16", hd(out16), r.out, fb["out16"]), ("out16+lo", hd(out16) + hd(lo), r.out, fb["sum16"]), ("lse16", lse, r.lse, fb["lse"])]
    rows = AB.out_rows(r.out)
    out_e = rows.float().to(dt).contiguous()
    lo_e = (rows - out_e.double()).float().to(dt).contiguous()
    lse_e = r.lse.float().contiguous()
    grads("exact", K.attn_bwd(qd, out_e, gd, lse_e, B, N, H, x.scale, out_lo=lo_e, **kw), lse_e, out_e, lo_e)
    grads("chain+lo", K.attn_bwd(qd, out16, gd, lse, B, N, H, x.scale, out_lo=lo, **kw), lse, out16, lo)
    grads("chain", K.attn_bwd(qd, out16, gd, lse, B, N, H, x.scale, **kw), lse, out16)
    return checks


class Tally:
    """worst ratio per output over the cases of a test, and every element-level failure with its place"""

    def __init__(self, label):
        self.label, self.worst, self.failures = label, {}, []

    def add(self, what, checks):
        ratios = torch.stack([AB.worst(g, ref, b) for _, g, ref, b in checks]).tolist()  # one synchronisation per case
        for (nm, g, ref, b), v in zip(checks, ratios):
            self.worst[nm] = max(self.worst.get(nm, 0.0), v)
            if not v <= AB.SLACK:
                idx, _ = AB.locate(g, ref, b)
                place = dict(zip(("clip", "head", "row", "column"), idx))
                self.failures.append(f"{what} {nm}: error / bound {v:.3f} at {place} (got {g[idx].item():.6g}, reference {ref[idx].item():.6g}, bound {b[idx].item():.3g})")

    def finish(self):
        print(f"RATIO {self.label}: " + ", ".join(f"{k} {v:.3f}" for k, v in self.worst.items()))
        assert not self.failures, f"{len(self.failures)} outputs over {AB.SLACK} x their bound:\n" + "\n".join(self.failures[:20])


def contracts(fmt):
    return (False,) if fmt == "f32" else (True, False)


# ------------------------------------------------------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("prescaled", [True, False], ids=["q_prescaled", "plain_q"])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("d", [64, 80])
def test_every_ragged_length_16bit(K, d, fmt, prescaled):
    t = Tally(f"sweep d={d} {fmt} {'q_prescaled' if prescaled else 'plain_q'}")
    for N in SWEEP:
        t.add(f"N={N}", launches(K, AB.make_inputs("spread", fmt, d, N, prescaled=prescaled)))
    t.finish()


@pytest.mark.parametrize("d", [64, 80])
def test_every_ragged_length_f32(K, d):
    t = Tally(f"sweep d={d} f32")
    for N in SWEEP:
        t.add(f"N={N}", launches(K, AB.make_inputs("spread", "f32", d, N)))
    t.finish()


# ------------------------------------------------------------------------------------------------------------------ other inputs
@pytest.mark.parametrize("fmt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("d", [64, 80])
def test_peaked_softmax_forward_and_backward(K, d, fmt):
    """the spike family (late maxima in tiles 0 and 2, rows far below zero, |lse| ~ 100): the backward has a peaked softmax to differentiate"""
    t = Tally(f"spike d={d} {fmt}")
    for prescaled in contracts(fmt):
        t.add(f"N=200 prescaled={prescaled}", launches(K, AB.make_inputs("spike", fmt, d, 200, prescaled=prescaled)))
    t.finish()


@pytest.mark.parametrize("fmt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("d,lengths", [(64, (1, 7, 33, 63, 64)), (80, (80,))])
def test_probe_reads_p_and_keeps_exact_zeros(K, d, lengths, fmt):
    """V = dout = one-hot rows: out and dV are P itself, element by element, and the columns no key writes are exactly 0.0"""
    t = Tally(f"probe d={d} {fmt}")
    for N in lengths:
        for prescaled in contracts(fmt):
            checks = launches(K, AB.make_inputs("probe", fmt, d, N, prescaled=prescaled))
            t.add(f"N={N} prescaled={prescaled}", checks)
            for nm, g, ref, b in checks:
                if nm.startswith(("out", "dv")):
                    zero = b == 0
                    assert int(zero.sum()) == 2 * 2 * N * (d - N), f"{nm} N={N}: the probe's zero columns are gone from the bound"
                    assert (g[zero] == 0).all(), f"{nm} N={N}: {int((g[zero] != 0).sum())} elements that no key writes are not exactly 0.0"
    t.finish()


@pytest.mark.parametrize("fmt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("d", [64, 80])
def test_dropout_with_the_regenerated_mask(K, d, fmt):
    t = Tally(f"dropout d={d} {fmt}")
    for N in (33, 129, 200):
        for prescaled in contracts(fmt):
            t.add(f"N={N} prescaled={prescaled}", launches(K, AB.make_inputs("spread", fmt, d, N, prescaled=prescaled), p=0.25, seed=20240919 + N))
    t.finish()


# ------------------------------------------------------------------------------------------------------------------ isolation
def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


@pytest.mark.parametrize("kind", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("d", [64, 80])
@pytest.mark.parametrize("N", [100, 64])
def test_nonfinite_values_in_clip_1_never_reach_clip_0(K, N, d, kind):
    """inf / NaN planted in clip 1 of qkv (q, k, v in turn; first element of row 0, last element of row N - 1) and likewise in clip 1 of dout:
    clip 0's out, lse and dqkv are bit for bit those of the run with a finite clip 1 (keys and query rows behind a clip's end are never
    read: the staged operands' buffer descriptors end with the clip), and clip 1 has at least the non-finite outputs of the fp64 formula
    and none outside the planted (clip, head) -- the contract of check_planted"""
    for prescaled in contracts(kind):
        _isolation(K, N, d, kind, prescaled)


def _isolation(K, N, d, kind, prescaled):
    B = H = 2
    x = AB.make_inputs("spread", kind, d, N, prescaled=prescaled)
    scale = x.scale
    dt = AB.FORMATS[kind][0]
    tol = 1e-5 if kind == "f32" else (2 if kind == "bf16" else 4) * ULP16[kind]  # (test_planted_nonfinite_attention_bwd's)

    def run(qkv, dout):
        qd, gd = qkv.cuda().to(dt), dout.cuda().to(dt)
        if kind == "f32":
            out, lse = K.attn_fwd_f32(qd, B, N, H, scale, want_lse=True, d=d)
            return out, lse, K.attn_bwd_f32(qd, out, gd, lse, B, N, H, scale, d=d)
        out, lse, lo = K.attn_fwd(qd, B, N, H, scale, want_lo=True, d=d, q_prescaled=prescaled)
        return out, lse, K.attn_bwd(qd, out, gd, lse, B, N, H, scale, out_lo=lo, d=d, q_prescaled=prescaled)

    base = run(x.opnd, x.dout)
    assert all(torch.isfinite(t).all() for t in base)
    places = [(0, 0, 0), (N - 1, H - 1, d - 1)]  # (row, head, element)
    cases = [("qkv", i, pl, v) for i in range(3) for pl in places for v in E.NONFINITE] + [("dout", None, pl, v) for pl in places for v in E.NONFINITE]
    for which, third, (n, h, e), v in cases:
        what = f"{kind} d={d} N={N} prescaled={prescaled}: {v} in clip 1 of {which}{'' if third is None else '.' + 'qkv'[third]} at row {n}"
        qkv, q64, dout = x.opnd, x.qkv, x.dout  # (q64: what the reference sees -- the operand, its q third divided by scale * log2e when pre-scaled)
        if which == "qkv":
            qkv = E.plant(qkv.reshape(B, N, 3, H, d), (1, n, third, h, e), v).reshape(B * N, -1)
            q64 = E.plant(q64.reshape(B, N, 3, H, d), (1, n, third, h, e), v).reshape(B * N, -1)
        else:
            dout = E.plant(dout.reshape(B, N, H, d), (1, n, h, e), v).reshape(B * N, -1)
        got = run(qkv, dout)
        for nm, a, b in zip(("out", "lse", "dqkv"), base, got):
            a0, b0 = (a[0], b[0]) if nm == "lse" else (a[:N], b[:N])
            assert torch.equal(_bits(a0), _bits(b0)), f"{what}: clip 0's {nm} changed in {int((_bits(a0) != _bits(b0)).sum())} elements"
        r = AB.reference(q64.cuda(), dout.cuda(), scale, B, N, H, d)
        radius = torch.zeros(B, H, N, d, dtype=torch.bool)
        radius[1, h] = True
        ref_dqkv = torch.stack([AB.out_rows(r[k]).reshape(B, N, H, d) for k in ("dq", "dk", "dv")], 2).reshape(B * N, -1)
        rad_dqkv = torch.stack([AB.out_rows(radius).reshape(B, N, H, d)] * 3, 2).reshape(B * N, -1)
        if which == "qkv":  # (a planted dout leaves the forward finite)
            check_planted(got[0].float(), AB.out_rows(r.out), AB.out_rows(radius), "out, " + what, tol=tol)
            if third < 2:
                check_planted(got[1], r.lse, radius[..., 0], "lse, " + what, tol=1e-3 if kind == "f32" else 4 * ULP16[kind])
            else:  # v does not enter the scores
                assert torch.equal(_bits(got[1]), _bits(base[1])), f"{what}: lse changed"
        check_planted(got[2].float(), ref_dqkv, rad_dqkv, "dqkv, " + what, tol=tol)
