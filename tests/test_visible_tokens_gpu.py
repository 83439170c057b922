"""csrc/visible_tokens.hip (the pre-training ABI, tadp_visible_tokens_fwd / _bwd) on the GPU, bit for bit against torch:

    forward   out[b, i] = x[b, tok[b, i]] + pos[tok[b, i]]                       one f32 add: the same bits as torch's
    dx        g scattered to [B, N, D], +0 where a token is masked                every row written
    dpos      the clips added in the order b = 0, 1, ... from +0                  a torch loop in that order gives the same bits

at the smallest shapes at which the kernels can go wrong (one element; ragged sizes; the model fixture's; nothing masked; one visible
token with 352 column groups -- more than a block's 256 threads; a sum of 33 terms), on operands between poisoned guard bands
(tests/guarded.py).  Each case is a fraction of a second."""
import pytest
import torch

import guarded
from simple_tad_amd import kernels as K, ops
from simple_tad_amd._lib import TadError

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 4), (3, 5, 2, 132), (2, 16, 4, 128), (5, 7, 7, 384), (4, 9, 1, 1408), (33, 3, 2, 8)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


@pytest.fixture(autouse=True)
def _restore_switches():
    yield
    ops.set_visible_token_kernels(True)
    ops.set_skip_frozen(True)


def visible(B, N, Nv, g):
    """tok [B, Nv] int32, distinct per clip, in no particular order.  Where the shape allows it the sets differ per clip, token 0 is
    visible in every clip and token N - 1 in none."""
    rows = []
    for b in range(B):
        if Nv == N:
            row = torch.randperm(N, generator=g)
        elif Nv == 1:
            row = torch.tensor([b % (N - 1)])                       # (token N - 1 is never seen)
        else:
            hi = N - 1 if N - 2 > Nv - 1 else N                     # keep token N - 1 out where the rest still leaves a choice
            pool = torch.arange(1, hi)
            row = torch.cat([torch.zeros(1, dtype=torch.long), pool[torch.randperm(pool.numel(), generator=g)[:Nv - 1]]])
            row = row[torch.randperm(Nv, generator=g)]
        rows.append(row)
    tok = torch.stack(rows).to(torch.int32)
    assert all(len(set(r.tolist())) == Nv for r in tok)
    return tok


def slot_of(tok, N):
    B, Nv = tok.shape
    slot = torch.full((B, N), -1, dtype=torch.int32)
    slot.scatter_(1, tok.long(), torch.arange(Nv, dtype=torch.int32).expand(B, -1))
    return slot


_CASES = {}


def case(shape):
    """inputs and torch references of one shape on the device: computed once, shared, never changed"""
    if shape not in _CASES:
        B, N, Nv, D = shape
        g = torch.Generator().manual_seed(B * 1000 + N * 100 + Nv * 10 + D)
        c = dict(x=torch.randn(B, N, D, generator=g), pos=torch.randn(N, D, generator=g), tok=visible(B, N, Nv, g),
                 g=torch.randn(B, Nv, D, generator=g), prev=torch.randn(N, D, generator=g))
        c["slot"] = slot_of(c["tok"], N)
        c = {k: v.cuda() for k, v in c.items()}
        bidx = torch.arange(B, device="cuda").unsqueeze(1)
        tl = c["tok"].long()
        c["out"] = c["x"][bidx, tl] + c["pos"][tl]
        c["dx"] = torch.zeros(B, N, D, device="cuda")
        c["dx"][bidx, tl] = c["g"]
        acc = torch.zeros(N, D, device="cuda")
        for b in range(B):                                          # the clips in order, from +0; masked tokens add nothing
            acc[tl[b]] = acc[tl[b]] + c["g"][b]
        c["dpos"] = acc
        c["dpos_acc"] = c["prev"] + acc                             # accumulate: the finished sum, one more add
        if N > 2 and 1 < Nv < N - 1:
            seen = torch.zeros(N, dtype=torch.int32, device="cuda").scatter_add_(0, tl.reshape(-1), torch.ones(B * Nv, dtype=torch.int32, device="cuda"))
            assert int(seen[0]) == B and int(seen[N - 1]) == 0 and (B == 1 or len({tuple(sorted(r.tolist())) for r in c["tok"].cpu()}) > 1)
        _CASES[shape] = c
    return _CASES[shape]


def eq(a, b):
    return guarded.same_bits(a, b)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_and_backward_bit_for_bit(shape):
    c = case(shape)
    B, N, Nv, D = shape
    out = K.visible_tokens_fwd(c["x"], c["pos"], c["tok"])
    assert out.shape == (B, Nv, D) and eq(out, c["out"])
    dx, dpos = K.visible_tokens_bwd(c["g"], c["slot"])
    assert eq(dx, c["dx"]), "dx, zeros included"
    assert eq(dpos, c["dpos"]), "dpos: the clips in order from +0"
    assert not (guarded.bits(dx) == -2 ** 31).any(), "masked rows are +0, not -0"
    # each output alone leaves the other unchanged
    dx1, none = K.visible_tokens_bwd(c["g"], c["slot"], want_dpos=False)
    assert none is None and eq(dx1, dx)
    none, dpos1 = K.visible_tokens_bwd(c["g"], c["slot"], want_dx=False)
    assert none is None and eq(dpos1, dpos)
    # accumulate: what the table's gradient held plus the finished sum
    into = c["prev"].clone()
    dx2, same = K.visible_tokens_bwd(c["g"], c["slot"], into=into.view(-1))
    assert same.data_ptr() == into.data_ptr() and eq(into, c["dpos_acc"]) and eq(dx2, dx)
    # two calls give the same bits
    dx3, dpos3 = K.visible_tokens_bwd(c["g"], c["slot"])
    assert eq(dx3, dx) and eq(dpos3, dpos) and eq(K.visible_tokens_fwd(c["x"], c["pos"], c["tok"]), out)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_nan_goes_exactly_where_it_belongs(shape):
    c = case(shape)
    B, N, Nv, D = shape
    # NaN in every masked row of x reaches nothing: those rows are never read
    x = c["x"].clone()
    masked = c["slot"] < 0
    x[masked] = float("nan")
    assert eq(K.visible_tokens_fwd(x, c["pos"], c["tok"]), c["out"])
    # NaN in one row of g reaches exactly its dx row and its dpos row
    b, i = B - 1, Nv - 1
    n = int(c["tok"][b, i])
    g = c["g"].clone()
    g[b, i] = float("nan")
    dx, dpos = K.visible_tokens_bwd(g, c["slot"])
    assert torch.isnan(dx[b, n]).all() and torch.isnan(dpos[n]).all()
    keep = torch.ones(B, N, dtype=torch.bool, device="cuda")
    keep[b, n] = False
    assert eq(dx[keep], c["dx"][keep])
    rows = torch.arange(N, device="cuda") != n
    assert eq(dpos[rows], c["dpos"][rows])


@pytest.mark.parametrize("poison", guarded.POISON_MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_between_poisoned_guard_bands(shape, poison):
    """every operand between guards (NaN, then the largest finite value; index guards hold in-range indices): the same bits, and no
    byte outside the outputs changes"""
    c = case(shape)
    B, N, Nv, D = shape
    arena = guarded.GuardedArena(48 << 20, "cuda", poison=poison)
    x, pos, g = (arena.place(c[k], role="input", name=k) for k in ("x", "pos", "g"))
    tok = arena.place(c["tok"], role="input", name="tok", index_range=N)
    slot = arena.place(c["slot"], role="input", name="slot", index_range=Nv)
    into = arena.place(c["prev"].reshape(-1), role="inout", name="dpos sink")
    with arena.route(K):
        out = K.visible_tokens_fwd(x, pos, tok)
        dx, dpos = K.visible_tokens_bwd(g, slot)
        dx_only, _ = K.visible_tokens_bwd(g, slot, want_dpos=False)
        _, dpos_only = K.visible_tokens_bwd(g, slot, want_dx=False)
        K.visible_tokens_bwd(g, slot, want_dx=False, into=into)
    arena.verify()
    assert all(arena.contains(t) for t in (out, dx, dpos, dx_only, dpos_only))
    assert eq(out, c["out"]) and eq(dx, c["dx"]) and eq(dpos, c["dpos"]) and eq(dx_only, c["dx"]) and eq(dpos_only, c["dpos"])
    assert eq(into.view(N, D), c["dpos_acc"])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_function_with_kernels_off_equals_kernels_on(shape):
    """ops.VisibleTokensFn: the torch route ((x + pos) then the index; autograd's backward) gives the kernels' bits in the forward and
    in dx.  In dpos it sums the clips in torch's order: the two differ by reordering at most, per element (B - 1) 2^-24 sum_b |g|."""
    c = case(shape)
    B, N, Nv, D = shape
    res = {}
    for on in (True, False):
        ops.set_visible_token_kernels(on)
        x = c["x"].clone().requires_grad_()
        pos = c["pos"].reshape(1, N, D).clone().requires_grad_()
        out = ops.VisibleTokensFn.apply(x, pos, c["tok"])
        out.backward(c["g"])
        assert pos.grad.shape == (1, N, D)
        res[on] = (out.detach(), x.grad, pos.grad[0])
    assert eq(res[True][0], c["out"]) and eq(res[False][0], c["out"])
    assert eq(res[True][1], c["dx"]) and eq(res[False][1], c["dx"])
    assert eq(res[True][2], c["dpos"])
    bound = (B - 1) * 2.0 ** -24 * c["dx"].abs().double().sum(0)
    err = (res[False][2].double() - res[True][2].double()).abs()
    print(f"{shape}: worst dpos reordering difference / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert (err <= bound).all()


def test_function_requests_only_what_is_wanted_and_takes_a_2d_table(monkeypatch):
    c = case((3, 5, 2, 132))
    calls = []
    orig = K.visible_tokens_bwd

    def spy(g, slot, want_dx=True, want_dpos=True, into=None):
        calls.append((want_dx, want_dpos, into is not None))
        return orig(g, slot, want_dx=want_dx, want_dpos=want_dpos, into=into)
    monkeypatch.setattr(K, "visible_tokens_bwd", spy)
    for x_grad, pos_grad in ((True, True), (False, True), (True, False)):
        x = c["x"].clone().requires_grad_(x_grad)
        pos = c["pos"].clone().requires_grad_(pos_grad)         # [N, D]
        ops.VisibleTokensFn.apply(x, pos, c["tok"]).backward(c["g"])
        assert calls[-1] == (x_grad, pos_grad, False)
        assert (x.grad is not None) == x_grad and (pos.grad is not None) == pos_grad
        if x_grad:
            assert eq(x.grad, c["dx"])
        if pos_grad:
            assert pos.grad.shape == (5, 132) and eq(pos.grad, c["dpos"])
    # a gradient sink: the table's gradient is added in place and autograd gets None
    x = c["x"].clone().requires_grad_()
    pos = torch.nn.Parameter(c["pos"].reshape(1, 5, 132).clone())
    pos.grad = c["prev"].reshape(1, 5, 132).clone()
    ops.register_grad_sink(pos, pos.grad.view(-1))
    ops.VisibleTokensFn.apply(x, pos, c["tok"]).backward(c["g"])
    assert calls[-1] == (True, True, True) and eq(pos.grad[0], c["dpos_acc"])
    # no forward without a GPU tensor, and inconsistent shapes are refused before the launch
    with pytest.raises(TadError, match="no CPU fallback"):
        ops.VisibleTokensFn.apply(c["x"].cpu(), c["pos"], c["tok"])
    with pytest.raises(TadError, match="do not belong together"):
        ops.VisibleTokensFn.apply(c["x"], c["pos"][:4], c["tok"])
    with pytest.raises(TadError, match="Nv=6 exceeds N=5"):
        K.visible_tokens_fwd(c["x"], c["pos"], torch.zeros(3, 6, dtype=torch.int32, device="cuda"))
