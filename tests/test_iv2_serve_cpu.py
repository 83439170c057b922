"""The InternVideo2 family's entry on the scoring path, as far as a machine without a GPU can see it: the input-stage attributes, the
refusals in their order, and the torch restatements of the two entry kernels (tests/iv2_serve_ref.py) that the GPU tests compare with."""
import pytest
import torch

import iv2_recipe as R
import iv2_serve_ref as S
import simple_tad_amd as T
from simple_tad_amd import internvideo2 as IV2, modeling_finetune as MF, ops
from simple_tad_amd._lib import TadError


@pytest.fixture(autouse=True)
def _restore():
    yield
    T.set_precision("fast")


def tiny(**over):
    torch.manual_seed(0)
    return IV2.InternVideo2(**dict(R.TINY, **R.REF_ROUTE, **over))


def test_patch_embed_carries_the_input_stage():
    m = tiny()
    pe, ref = m.patch_embed, MF.PatchEmbed
    for a in ("input_mean", "input_std", "input_bgr", "t_offset"):
        assert getattr(IV2.PatchEmbed, a) == getattr(ref, a), a
    assert "input_mean" not in vars(pe) and pe.t_offset == 0
    pe.set_input_normalization((0.5, 0.25, 0.125), (1, 2, 4), bgr=True)
    assert pe.input_mean == (0.5, 0.25, 0.125) and pe.input_std == (1.0, 2.0, 4.0) and pe.input_bgr is True
    assert IV2.PatchEmbed.input_bgr is False, "set_input_normalization writes the instance"
    assert (m.num_frames, m.tubelet_size, m.num_classes) == (2, 1, 2)
    from simple_tad_amd.explain import token_grid
    assert token_grid(m) == (2, 2, 2)
    # plain attributes: the state dict and the parameter census are what they were (tests/test_iv2_cpu.py pins their values)
    assert not any(k.startswith(("num_", "tubelet")) for k in m.state_dict())
    big = T.create_model("internvideo2_small_patch14_224", num_classes=2)
    assert (big.num_frames, big.tubelet_size, big.num_classes) == (8, 1, 2)


def test_wrong_frame_size_is_refused_by_the_assertion():
    pe = tiny().patch_embed
    text = r"Input image size \(14\*28\) doesn't match model \(28\*28\)\."
    with pytest.raises(AssertionError, match=text):
        pe(torch.zeros(1, 2, 14, 28, 3, dtype=torch.uint8))
    with pytest.raises(AssertionError, match=text):
        pe(torch.zeros(1, 3, 2, 14, 28))
    with pytest.raises(AssertionError, match=text):
        pe(torch.zeros(1, 3, 2, 14, 28, dtype=torch.bfloat16))
    from simple_tad_amd.frame_store import FrameWindows
    with pytest.raises(AssertionError, match=text):
        pe(FrameWindows(torch.zeros(4, 14, 28, 3, dtype=torch.uint8), torch.zeros(1, 2, dtype=torch.int32)))


def test_uint8_clip_is_refused_under_precise_before_the_family_refusal():
    pe = tiny().patch_embed
    T.set_precision("precise")
    with pytest.raises(TadError, match='"precise" takes the normalised f32 clip'):
        pe(torch.zeros(1, 2, 28, 28, 3, dtype=torch.uint8))
    from simple_tad_amd.frame_store import FrameWindows
    with pytest.raises(TadError, match='"precise" takes the normalised f32 clip'):
        pe(FrameWindows(torch.zeros(4, 28, 28, 3, dtype=torch.uint8), torch.zeros(1, 2, dtype=torch.int32)))
    # the float clip meets the family's own refusal
    with pytest.raises(TadError, match="has no route for the InternVideo2 family"):
        pe(torch.zeros(1, 3, 2, 28, 28))


def test_cpu_model_still_refuses_to_run():
    m = tiny().eval()
    for x in (R.clip(), torch.zeros(1, 2, 28, 28, 3, dtype=torch.uint8)):
        with pytest.raises(TadError, match="no CPU fallback"), torch.no_grad():
            m(x)
    with pytest.raises(TadError, match="no CPU fallback"):
        m(R.clip())
    with pytest.raises(TadError, match="no CPU fallback"):
        ops.ClassTokenEntryFn.apply(torch.zeros(1, 8, 128), m.cls_token, m.pos_embed)


def test_scoring_entry_points_give_their_own_no_cpu_errors():
    from simple_tad_amd.inference import SlidingWindow, score_video
    m = tiny()
    frames = torch.zeros(4, 28, 28, 3, dtype=torch.uint8)
    with pytest.raises(TadError, match=r"score_video keeps its frames in HBM.*no CPU path"):
        score_video(m, frames, orig_fps=10, target_fps=10)
    with pytest.raises(TadError, match=r"SlidingWindow keeps its frames in HBM.*no CPU path"):
        SlidingWindow(m)


def test_the_switch_is_a_plain_flag():
    assert ops.get_iv2_serve_kernels() is True
    ops.set_iv2_serve_kernels(0)
    try:
        assert ops.get_iv2_serve_kernels() is False
    finally:
        ops.set_iv2_serve_kernels(True)


@pytest.mark.parametrize("B,N,D", [(1, 1, 4), (2, 8, 12), (3, 2, 8), (5, 9, 20)])
def test_the_restatements_of_the_entry_kernels(B, N, D):
    """fp64: the restated forward is cat + add; the restated backward is the explicit loop over the clips (and autograd's own sums)"""
    g = torch.Generator().manual_seed(B * 100 + N * 10 + D)
    patch, cls, pos = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((B, N, D), (D,), (N + 1, D)))
    out = S.entry_fwd(patch, cls, pos)
    assert torch.equal(out, torch.cat((cls.reshape(1, 1, D).expand(B, -1, -1), patch), 1) + pos)
    for b in range(B):
        assert torch.equal(out[b, 0], cls + pos[0])
        for n in range(N):
            assert torch.equal(out[b, 1 + n], patch[b, n] + pos[1 + n])
    go = torch.randn(B, N + 1, D, generator=g, dtype=torch.float64)
    dpatch, dpos, dcls = S.entry_bwd(go)
    acc = go[0].clone()
    for b in range(1, B):
        acc = acc + go[b]
    assert torch.equal(dpatch, go[:, 1:]) and torch.equal(dpos, acc) and torch.equal(dcls, acc[0])
    leaves = [t.clone().requires_grad_() for t in (patch, cls, pos)]
    (S.entry_fwd(*leaves) * go).sum().backward()
    assert torch.equal(leaves[0].grad, dpatch)
    assert torch.allclose(leaves[2].grad, dpos, rtol=1e-14, atol=1e-14) and torch.allclose(leaves[1].grad, dcls, rtol=1e-14, atol=1e-14)
    # the f32 loop is what the kernel is held to, bit for bit: it starts from g[0], not from +0 (a -0 survives)
    z = torch.full((1, 2, 4), -0.0)
    assert torch.equal(S.entry_bwd(z)[1].view(torch.int32), z[0].view(torch.int32))
