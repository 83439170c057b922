"""CPU-side checks of the attention column sum and the rollout built on it: tad_attn_colsum's host validation (through ctypes, before any
launch), the f32 emulation of the kernel's data flow against the per-element bound of tests/attn_colsum_bounds.py -- and four planted defects
that must leave it --, the rollout identity in fp64, and capture_attention's refusals."""
import ctypes

import pytest
import torch

import attn_colsum_bounds as CB


@pytest.fixture(scope="module")
def lib():
    from simple_tad_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------------ host validation
def test_host_validation_refuses_before_any_launch(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(qkv=p, op=1, lse=p, w=p, out=p, B=1, N=8, H=1, d=64, scale=0.125, qs=0)

    def call(**kw):
        a = {**ok, **kw}
        return lib.tad_attn_colsum(a["qkv"], a["op"], a["lse"], a["w"], a["out"], a["B"], a["N"], a["H"], a["d"], a["scale"], a["qs"], None)

    for name in ("qkv", "lse", "w", "out"):
        assert call(**{name: None}) == -1, name
        assert b"null" in lib.tad_last_error_string(), name
    for d in (32, 96, 0):
        assert call(d=d) == -1
        assert b"head_dim" in lib.tad_last_error_string()
    for op in (0, 3, -1):
        assert call(op=op) == -1
        assert b"op_dtype" in lib.tad_last_error_string()
    for dim in ("B", "N", "H"):
        for v in (0, -3):
            assert call(**{dim: v}) == -1, (dim, v)
            assert b"bad shape" in lib.tad_last_error_string(), (dim, v)


def test_binding_is_declared_without_a_half_twin():
    from simple_tad_amd import _lib
    assert "tad_attn_colsum" in _lib.SIGNATURES and "tad_attn_colsum_f16" not in _lib.SIGNATURES
    assert "tad_attn_colsum" not in _lib.F16_TWINS


# ------------------------------------------------------------------------------------------------------------------ emulation vs bound
CASES = [("spread", 64, 33), ("spread", 80, 129), ("spread", 64, 130), ("spike", 64, 193), ("spike", 80, 65), ("spread", 64, 1), ("spread", 80, 64)]


def _run(family, fmt, d, N, prescaled, wkind, defect=None):
    x = CB.make_inputs(family, fmt, d, N, prescaled=prescaled)
    r = CB.reference(x.qkv, x.dout, x.scale, x.B, N, x.H, d)
    lse = r.lse.float()
    w = CB.weights(wkind, x.B, N)
    got = CB.emulate(x.opnd, lse, w, x.B, N, x.H, d, x.scale, prescaled, defect=defect)
    return float(CB.worst(got, CB.colsum_reference(r, w, lse), CB.colsum_bound(r, w, lse)))


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("prescaled", [True, False], ids=["q_prescaled", "plain_q"])
def test_emulation_meets_the_bound(fmt, prescaled):
    worst = {}
    for family, d, N in CASES:
        for wkind in CB.WEIGHTS:
            worst[(family, d, N, wkind)] = _run(family, fmt, d, N, prescaled, wkind)
    print("worst emulation error / bound", max(worst.values()))
    over = {k: v for k, v in worst.items() if not v <= CB.SLACK}
    assert not over, over


# (defect, the weights under which it must show, shapes with a ragged half tile / more than one key block)
DEFECT_CASES = {
    "ragged_row_counted": ("uniform", [("spread", 64, 33), ("spread", 80, 129), ("spike", 64, 193)]),
    "lse_of_other_head": ("uniform", [("spread", 64, 33), ("spread", 80, 129), ("spike", 64, 193)]),
    "w_of_other_clip": ("pow2", [("spread", 64, 33), ("spread", 80, 129), ("spike", 64, 193)]),
    "last_key_block_skipped": ("uniform", [("spread", 80, 129), ("spread", 64, 130), ("spike", 64, 193)]),
}
WIDE = 64.0  # "by a wide margin": a defect of this kind is a term of the sum gone wrong, the bound is 1e-6 of the sum


@pytest.mark.parametrize("defect", CB.DEFECTS)
def test_each_planted_defect_leaves_the_bound_by_a_wide_margin(defect):
    wkind, cases = DEFECT_CASES[defect]
    for fmt in ("bf16", "f16"):
        for family, d, N in cases:
            clean = _run(family, fmt, d, N, True, wkind)
            broken = _run(family, fmt, d, N, True, wkind, defect=defect)
            assert clean <= CB.SLACK and broken > WIDE * CB.SLACK, (defect, fmt, family, d, N, clean, broken)


# ------------------------------------------------------------------------------------------------------------------ rollout identity
@pytest.mark.parametrize("start_kind", ["uniform", "onehot"])
def test_vector_recurrence_equals_the_matrix_rollout_fp64(start_kind):
    """v_{l-1} = alpha v_l + (1 - alpha) mean_h(v_l^T P_{l,h}) from the last layer to the first equals u^T prod_l (alpha I + (1 - alpha) Abar_l)
    (the product taken with the LAST layer leftmost), and simple_tad_amd.explain.token_rollout runs exactly that recurrence"""
    from simple_tad_amd import explain
    N, L, H, alpha = 7, 3, 2, 0.5
    g = torch.Generator().manual_seed(5)
    P = torch.softmax(3.0 * torch.randn(L, 1, H, N, N, generator=g, dtype=torch.float64), -1)  # row-stochastic
    u = torch.full((1, N), 1.0 / N, dtype=torch.float64) if start_kind == "uniform" else torch.eye(N, dtype=torch.float64)[:1]
    M = torch.eye(N, dtype=torch.float64)
    for l in range(L):  # rollout = A~_L ... A~_1
        M = (alpha * torch.eye(N, dtype=torch.float64) + (1 - alpha) * P[l, 0].mean(0)) @ M
    want = u @ M
    want = want / want.sum(-1, keepdim=True)
    colsum = lambda rec, v: torch.einsum("bi,bhij->bhj", v, rec)  # noqa: E731
    got = explain.token_rollout([P[l] for l in range(L)], u, residual=alpha, colsum=colsum)
    assert got.dtype == torch.float64 and got.shape == (1, N)
    assert float((got - want).abs().max()) <= 1e-12
    assert float((got.sum(-1) - 1).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------ capture refusals
def _tiny_model():
    from simple_tad_amd.modeling_finetune import VisionTransformer
    return VisionTransformer(img_size=32, patch_size=16, num_classes=2, embed_dim=128, depth=1, num_heads=2, all_frames=4, tubelet_size=2,
                             init_values=0.0)


def test_capture_refuses_precise_training_grad_and_nesting():
    import simple_tad_amd as T
    from simple_tad_amd import ops
    from simple_tad_amd._lib import TadError
    assert not ops.attention_capture_active()
    with pytest.raises(TadError, match="no_grad"):
        with ops.capture_attention():
            pass
    model = _tiny_model()
    with torch.no_grad():
        with ops.capture_attention() as rec:
            assert rec == [] and ops.attention_capture_active()
            with pytest.raises(TadError, match="nest"):
                with ops.capture_attention():
                    pass
            assert ops.attention_capture_active(), "the refused inner capture must not end the outer one"
            # a model in training mode is refused by its attention modules before any device work (CPU tensors never reach a kernel)
            model.train()
            with pytest.raises(TadError, match="training mode"):
                model.blocks[0].attn(torch.zeros(1, 8, 128))
        assert not ops.attention_capture_active()
        with pytest.raises(TadError, match="training mode"):
            with ops.capture_attention(model):
                pass
        model.eval()
        T.set_precision("precise")
        try:
            with pytest.raises(TadError, match="precise"):
                with ops.capture_attention(model):
                    pass
        finally:
            T.set_precision("fast")
        assert not ops.attention_capture_active()
        with pytest.raises(RuntimeError, match="boom"):
            with ops.capture_attention():
                raise RuntimeError("boom")
        assert not ops.attention_capture_active()
