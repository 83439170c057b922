"""tad_attn_colsum (csrc/attn_colsum.hip) against its fp64 reference at EVERY output element, each held to its own a-priori bound
(tests/attn_colsum_bounds.py; SLACK = 1.0625 x the first-order bound): head dims, operand formats and q contracts, the ragged lengths around
every tile edge, spread and peaked softmax rows, five weight vectors, the lse handed exact and as tad_attn_fwd wrote it; conservation;
clip isolation and reproducibility; guard bands.  The fp64 work stays on the device.

The bound test prints the worst error / bound it saw ("RATIO ..." lines: measurements, recorded in DESIGN.md section 8n, never asserted)."""
import pytest
import torch

import attn_colsum_bounds as CB
import edge_cases as E
from guarded import GuardedArena, same_bits

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 191, 193, 257)
FAMILIES = ("spread", "spike")


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import _lib, kernels
    _lib.load()
    return kernels


def _case(K, family, fmt, d, N, prescaled):
    """(inputs, reference, device operand, {"exact": lse, "fwd": lse}) of one shape"""
    x = CB.make_inputs(family, fmt, d, N, prescaled=prescaled)
    r = CB.reference(x.qkv.cuda(), x.dout.cuda(), x.scale, x.B, N, x.H, d)
    qd = x.opnd.cuda().to(CB.FORMATS[fmt][0])
    lse_fwd = K.attn_fwd(qd, x.B, N, x.H, x.scale, out_dtype=torch.float32, q_prescaled=prescaled, d=d)[1]
    return x, r, qd, {"exact": r.lse.float().contiguous(), "fwd": lse_fwd}


@pytest.mark.parametrize("prescaled", [True, False], ids=["q_prescaled", "plain_q"])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("d", [64, 80])
def test_every_element_within_its_bound_and_the_sum_is_conserved(K, d, fmt, prescaled):
    checks, cons = [], []
    for family in FAMILIES:
        for N in LENGTHS:
            x, r, qd, lses = _case(K, family, fmt, d, N, prescaled)
            for wk in CB.WEIGHTS:
                w = CB.weights(wk, x.B, N).cuda()
                for lk, lse in lses.items():
                    got = K.attn_colsum(qd, lse, w, x.B, N, x.H, x.scale, q_prescaled=prescaled, d=d)
                    ref, bound = CB.colsum_reference(r, w, lse), CB.colsum_bound(r, w, lse)
                    checks.append((f"{family} N={N} w={wk} lse={lk}", CB.worst(got, ref, bound)))
                    if lk == "exact":  # sum_j P_ij = 1: the weights' sum comes back
                        gap = (got.double().sum(-1) - w.double().sum(-1)[:, None]).abs()
                        cons.append((f"{family} N={N} w={wk}", (gap / bound.sum(-1)).max()))
    ratios = torch.stack([v for _, v in checks]).tolist()
    cratios = torch.stack([v for _, v in cons]).tolist()
    print(f"RATIO colsum d={d} {fmt} {'q_prescaled' if prescaled else 'plain_q'}: worst error / bound {max(ratios):.3f}, "
          f"worst conservation gap / sum of bounds {max(cratios):.3f}")
    bad = [f"{what}: error / bound {v:.3f}" for (what, _), v in zip(checks, ratios) if not v <= CB.SLACK]
    assert not bad, f"{len(bad)} launches over {CB.SLACK} x their bound:\n" + "\n".join(bad[:20])
    bad = [f"{what}: gap / sum of bounds {v:.3f}" for (what, _), v in zip(cons, cratios) if not v <= 1.0]
    assert not bad, f"{len(bad)} launches do not conserve the weights' sum:\n" + "\n".join(bad[:20])


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("d", [64, 80])
@pytest.mark.parametrize("N", [100, 64, 129])
def test_clips_are_isolated_and_results_reproducible(K, N, d, fmt):
    """inf / NaN planted in clip 1 of qkv (q and k thirds), lse and w: clip 0's output keeps its bits.  Clip b computed alone equals clip b
    computed in the batch, and two calls give identical bits."""
    prescaled = True
    x, r, qd, lses = _case(K, "spread", fmt, d, N, prescaled)
    B, H = x.B, x.H
    lse = lses["fwd"]
    w = CB.weights("signed", B, N).cuda()
    run = lambda q, l, ww, b=B: K.attn_colsum(q, l, ww, b, N, H, x.scale, q_prescaled=prescaled, d=d)  # noqa: E731
    base = run(qd, lse, w)
    assert torch.isfinite(base).all()
    assert same_bits(base, run(qd, lse, w)), "two calls differ"
    for b in range(B):
        alone = run(qd[b * N:(b + 1) * N].contiguous(), lse[b:b + 1].contiguous(), w[b:b + 1].contiguous(), 1)
        assert same_bits(alone[0], base[b]), f"clip {b} alone differs from clip {b} in the batch"
    for v in E.NONFINITE:
        for n, h, e in ((0, 0, 0), (N - 1, H - 1, d - 1)):
            for third in (0, 1):
                q2 = qd.clone().reshape(B, N, 3, H, d)
                q2[1, n, third, h, e] = v
                got = run(q2.reshape(B * N, -1), lse, w)
                assert same_bits(got[0], base[0]), f"{v} in clip 1's qkv third {third} row {n}: clip 0 changed"
                assert not torch.isfinite(got[1, h]).all(), f"{v} in clip 1's qkv third {third} row {n} left its own head finite"
            l2 = lse.clone()
            l2[1, h, n] = v
            assert same_bits(run(qd, l2, w)[0], base[0]), f"{v} in clip 1's lse row {n}: clip 0 changed"
            w2 = w.clone()
            w2[1, n] = v
            assert same_bits(run(qd, lse, w2)[0], base[0]), f"{v} in clip 1's w row {n}: clip 0 changed"


@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("N", [33, 129])
def test_guard_bands(K, N, fmt, poison):
    """every operand between two poisoned bands: no store lands outside `out`, and the result is, bit for bit, that of the same call on
    ordinary allocations (nothing read from the bands reaches it)"""
    d, prescaled = 80, True
    x, r, qd, lses = _case(K, "spread", fmt, d, N, prescaled)
    w = CB.weights("pow2", x.B, N).cuda()
    plain = K.attn_colsum(qd, lses["fwd"], w, x.B, N, x.H, x.scale, q_prescaled=prescaled, d=d)
    arena = GuardedArena(16 << 20, "cuda", poison=poison)
    qa, la, wa = arena.place(qd, name="qkv"), arena.place(lses["fwd"], name="lse"), arena.place(w, name="w")
    with arena.route(K):
        got = K.attn_colsum(qa, la, wa, x.B, N, x.H, x.scale, q_prescaled=prescaled, d=d)
    arena.verify()
    assert arena.contains(got), "the wrapper's output was not routed into the arena"
    assert same_bits(got, plain), "the result depends on bytes outside the operands"
