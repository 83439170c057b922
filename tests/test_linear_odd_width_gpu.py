"""A Linear whose width is no multiple of 8 -- the MAE decoder head of a 14 x 14 patch, 588 pixels -- on the way back.  The
weight-gradient GEMM and the 16-bit column sums move dy's rows in 16-byte pieces and refuse such a width; kernels.linear_bwd_weight and
kernels.colsum_bf16 pad dy with zero columns to the next multiple of 8 and drop what the extra columns produce.  Held here bit for bit
against the same call on a hand-padded dy (N = 592), whose first 588 rows / entries are the same sums in the same order."""
import pytest
import torch
import torch.nn.functional as F

import guarded
import simple_tad_amd as T
from simple_tad_amd import kernels as K, ops

pytestmark = pytest.mark.gpu

M, N, NP, KD = 70, 588, 592, 64
FORMATS = [torch.bfloat16, torch.float16]


@pytest.fixture(autouse=True)
def _restore():
    yield
    T.set_precision("fast")
    ops.set_skip_frozen(True)
    ops.invalidate_weight_cache()


def operands(dtype):
    g = torch.Generator().manual_seed(588)
    dy = torch.randn(M, N, generator=g).cuda().to(dtype)
    x = torch.randn(M, KD, generator=g).cuda().to(dtype)
    return dy, x, F.pad(dy, (0, NP - N)).contiguous()


@pytest.mark.parametrize("dtype", FORMATS)
def test_weight_gradient_at_588_is_the_padded_call_bit_for_bit(dtype):
    dy, x, dyp = operands(dtype)
    refW, refb = K.linear_bwd_weight(dyp, x, want_bias=True)
    assert refW.shape == (NP, KD) and not refW[N:].any() and not refb[N:].any()  # (what the zero columns produce)
    dW, db = K.linear_bwd_weight(dy, x, want_bias=True)
    assert dW.shape == (N, KD) and db.shape == (N,) and dW.is_contiguous()
    assert guarded.same_bits(dW, refW[:N]) and guarded.same_bits(db, refb[:N])
    dW2, none = K.linear_bwd_weight(dy, x, want_bias=False)
    assert none is None and guarded.same_bits(dW2, refW[:N])
    # against fp64, per element: f32 accumulation of M exact products of 16-bit values
    ref64 = dy.double().t() @ x.double()
    bound = M * 2.0 ** -24 * (dy.double().abs().t() @ x.double().abs()) + 2.0 ** -23 * ref64.abs()
    assert ((dW.double() - ref64).abs() <= bound).all()
    # given outputs (gradient sinks): overwritten, or with accumulate added to -- one more f32 add per element
    g = torch.Generator().manual_seed(1)
    w0, b0 = torch.randn(N, KD, generator=g).cuda(), torch.randn(N, generator=g).cuda()
    w1, b1 = w0.clone(), b0.clone()
    outW, outb = K.linear_bwd_weight(dy, x, want_bias=True, dW=w1, db=b1, accumulate=True)
    assert outW.data_ptr() == w1.data_ptr() and outb.data_ptr() == b1.data_ptr()
    assert guarded.same_bits(w1, w0 + refW[:N]) and guarded.same_bits(b1, b0 + refb[:N])
    K.linear_bwd_weight(dy, x, want_bias=True, dW=w1, db=b1, accumulate=False)
    assert guarded.same_bits(w1, refW[:N]) and guarded.same_bits(b1, refb[:N])


@pytest.mark.parametrize("dtype", FORMATS)
def test_column_sums_at_588_are_the_padded_call_bit_for_bit(dtype):
    dy, _, dyp = operands(dtype)
    ref = K.colsum_bf16(dyp)
    s = K.colsum_bf16(dy)
    assert s.shape == (N,) and guarded.same_bits(s, ref[:N])
    out = torch.full((N,), float("nan"), device="cuda")
    assert K.colsum_bf16(dy, out=out).data_ptr() == out.data_ptr() and guarded.same_bits(out, ref[:N])


@pytest.mark.parametrize("mode", ["fast", "half"])
def test_linear_fn_at_588_all_trainable_bias_only_and_into_sinks(mode):
    """ops.LinearFn, the decoder head's route: weight and bias gradients equal the padded kernel call on the same 16-bit operands; with
    the weight frozen the bias gradient comes from the column sums alone; with gradient sinks both are added in place"""
    T.set_precision(mode)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(M, KD, generator=g).cuda()
    w = torch.nn.Parameter((0.1 * torch.randn(N, KD, generator=g)).cuda())
    b = torch.nn.Parameter(torch.randn(N, generator=g).cuda())
    dy = torch.randn(M, N, generator=g).cuda()
    dyb, xb = K.cast_bf16(dy), K.cast_bf16(x)
    refW, refb = K.linear_bwd_weight(F.pad(dyb, (0, NP - N)).contiguous(), xb, want_bias=True)
    refW, refb = refW[:N], refb[:N]

    xg = x.clone().requires_grad_()
    ops.LinearFn.apply(xg, w, b).backward(dy)
    assert guarded.same_bits(w.grad, refW) and guarded.same_bits(b.grad, refb) and xg.grad.shape == (M, KD)
    dx = xg.grad.clone()

    # the weight frozen, the bias trainable: no weight-gradient launch, the bias gradient from the 16-bit column sums
    w.requires_grad_(False)
    w.grad = b.grad = None
    calls = []
    orig = K.linear_bwd_weight
    K.linear_bwd_weight = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        xg = x.clone().requires_grad_()
        ops.LinearFn.apply(xg, w, b).backward(dy)
    finally:
        K.linear_bwd_weight = orig
    assert not calls and w.grad is None and guarded.same_bits(xg.grad, dx)
    assert guarded.same_bits(b.grad, K.colsum_bf16(F.pad(dyb, (0, NP - N)).contiguous())[:N])

    # gradient sinks on both: added in place, autograd gets None
    w.requires_grad_(True)
    g0w, g0b = torch.randn(N, KD, generator=g).cuda(), torch.randn(N, generator=g).cuda()
    w.grad, b.grad = g0w.clone(), g0b.clone()
    ops.register_grad_sink(w, w.grad.view(-1))
    ops.register_grad_sink(b, b.grad.view(-1))
    sink_w, sink_b = w.grad, b.grad
    ops.LinearFn.apply(x.clone().requires_grad_(), w, b).backward(dy)
    assert w.grad is sink_w and b.grad is sink_b
    assert guarded.same_bits(w.grad, g0w + refW) and guarded.same_bits(b.grad, g0b + refb)
