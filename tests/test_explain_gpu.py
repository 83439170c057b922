"""simple_tad_amd.explain on the GPU, on a tiny model (embed 128, 2 heads of 64, depth 3; 4 frames of 32 x 32 or 48 x 32, patch 16, tubelet 2):
the logits under capture are the plain ones bit for bit on every block route; attention_rollout is, bit for bit, the recurrence written out
here with kernels.attn_colsum; it equals the explicit fp64 N x N rollout within the compounded per-layer bound; the maps are normalised,
non-negative and laid out time-major; score_video's saliency option changes nothing else."""
import pytest
import torch

import attn_bounds as AB
import attn_colsum_bounds as CB
from attn_util import LOG2E
from guarded import same_bits

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
T_FRAMES, TUB, PATCH = 4, 2, 16
MODES = ("fast", "half")


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import _lib, kernels
    _lib.load()
    return kernels


@pytest.fixture()
def mode(request):
    import simple_tad_amd as T
    T.set_precision(request.param)
    yield request.param
    T.set_precision("fast")


def tiny(img=(32, 32), seed=0, **kw):
    import simple_tad_amd as T
    torch.manual_seed(seed)
    cfg = dict(img_size=img, patch_size=PATCH, embed_dim=128, depth=3, num_heads=2, mlp_ratio=4, qkv_bias=True, all_frames=T_FRAMES,
               tubelet_size=TUB, num_classes=2, init_scale=1.0)
    cfg.update(kw)
    m = T.VisionTransformer(**cfg).cuda().eval()
    with torch.no_grad():  # (the default initialisation leaves every softmax row uniform to three digits: give the scores a spread)
        for blk in m.blocks:
            blk.attn.qkv.weight.mul_(12.0)
    return m


def clip(B, img=(32, 32), seed=1):
    return torch.randn(B, 3, T_FRAMES, *img, generator=torch.Generator().manual_seed(seed)).cuda()


class Route:
    """the switches that send the blocks of a tiny model down one of the routes through ops._attn_fwd_core"""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        from simple_tad_amd import ops
        self.saved = (ops.get_pooled_tail(), ops.get_block_variants())
        ops.set_pooled_tail(self.name == "pooled_tail")
        ops.set_block_variants(self.name != "composed")
        layer_scale = self.name in ("composed", "variant")
        return tiny(init_values=0.1 if layer_scale else 0.0)

    def __exit__(self, *a):
        from simple_tad_amd import ops
        ops.set_pooled_tail(self.saved[0])
        ops.set_block_variants(self.saved[1])


def _records(m, x):
    from simple_tad_amd import ops
    with torch.no_grad():
        with ops.capture_attention(m) as recs:
            logits = m(x)
    return logits, recs


# ------------------------------------------------------------------------------------------------------------------ logits
@pytest.mark.parametrize("mode", MODES, indirect=True)
@pytest.mark.parametrize("route", ["fused", "pooled_tail", "composed", "variant"])
def test_logits_under_capture_are_the_plain_logits(route, mode):
    from simple_tad_amd import ops
    with Route(route) as m:
        x = clip(3)
        with torch.no_grad():
            plain = m(x)
        logits, recs = _records(m, x)
        assert not ops.attention_capture_active()
        assert same_bits(logits, plain), f"{route} {mode}: the capture changed the logits"
        assert len(recs) == 3
        op = torch.float16 if mode == "half" else torch.bfloat16
        for qkv, lse, B, N, H, d, scale, qs in recs:
            assert (B, N, H, d) == (3, 8, 2, 64) and qkv.dtype == op and qkv.shape == (B * N, 3 * H * d)
            assert lse.dtype == torch.float32 and lse.shape == (B, H, N) and torch.isfinite(lse).all()
        with torch.no_grad():
            assert same_bits(m(x), plain), "a forward after the capture differs"


# ------------------------------------------------------------------------------------------------------------------ wiring
@pytest.mark.parametrize("mode", MODES, indirect=True)
@pytest.mark.parametrize("reduction,alpha", [("fc_norm", 0.5), ("cls", 0.5), ("fc_norm", 0.25)])
def test_rollout_is_the_written_out_recurrence(K, reduction, alpha, mode):
    from simple_tad_amd import explain
    m = tiny(final_reduction=reduction)
    x = clip(2)
    logits, sal = explain.attention_rollout(m, x, residual=alpha)
    plain, recs = _records(m, x)
    assert same_bits(logits, plain)
    B, N = 2, 8
    v = torch.full((B, N), 1.0 / N, device="cuda") if reduction == "fc_norm" else torch.eye(N, device="cuda")[:1].repeat(B, 1)
    for qkv, lse, b, n, H, d, scale, qs in reversed(recs):
        c = K.attn_colsum(qkv, lse, v.contiguous(), b, n, H, scale, q_prescaled=qs, d=d)
        v = alpha * v + (1 - alpha) * c.mean(1)
    v = v / v.sum(-1, keepdim=True)
    assert sal.shape == (B, 2, 2, 2) and same_bits(sal.reshape(B, N), v)
    assert same_bits(explain.token_rollout(recs, torch.full((B, N), 1.0 / N, device="cuda") if reduction == "fc_norm" else
                                           torch.eye(N, device="cuda")[:1].repeat(B, 1), alpha), v)


def test_reduction_none_needs_a_start_vector():
    from simple_tad_amd import explain
    from simple_tad_amd._lib import TadError
    m = tiny(final_reduction="none")
    x = clip(1)
    with pytest.raises(TadError, match="start"):
        explain.attention_rollout(m, x)
    start = torch.zeros(1, 8, device="cuda")
    start[0, 5] = 1.0
    _, sal = explain.attention_rollout(m, x, start=start)
    assert sal.shape == (1, 2, 2, 2) and abs(float(sal.sum()) - 1.0) < 1e-5
    assert not m.training


# ------------------------------------------------------------------------------------------------------------------ numerics
def _fp64_layer(rec):
    """attn_bounds.reference of a captured layer: the stored operands in fp64 (the q third divided by scale * log2e where it is pre-scaled)"""
    qkv, lse, B, N, H, d, scale, qs = rec
    q5 = qkv.double().reshape(B, N, 3, H, d).clone()
    if qs:
        q5[:, :, 0] /= scale * LOG2E
    return AB.reference(q5.reshape(B * N, -1), torch.zeros(B * N, H * d, dtype=torch.float64, device=qkv.device), scale, B, N, H, d)


@pytest.mark.parametrize("mode", MODES, indirect=True)
@pytest.mark.parametrize("img", [(32, 32), (48, 32)])
@pytest.mark.parametrize("reduction", ["fc_norm", "cls"])
def test_rollout_equals_the_fp64_matrix_rollout(reduction, img, mode):
    """every factor of the chain is non-negative, so the relative errors of the layers compound at most additively to first order:
    |got - ref| <= SLACK (sum_l eps_l + 2^-22) ref per element (2^-22: the blend's and the normalisation's roundings), eps_l from
    attn_colsum_bounds.rollout_tolerance -- the kernel's own lse error dl_i, measured against fp64, is part of it"""
    from simple_tad_amd import explain
    alpha = 0.5
    m = tiny(img=img, final_reduction=reduction)
    x = clip(2, img)
    _, sal = explain.attention_rollout(m, x, residual=alpha)
    _, recs = _records(m, x)
    B, N = recs[0][2], recs[0][3]
    eye = torch.eye(N, dtype=torch.float64, device="cuda")
    v = torch.full((B, 1, N), 1.0 / N, dtype=torch.float64, device="cuda") if reduction == "fc_norm" else eye[:1].repeat(B, 1, 1)
    eps = 0.0
    for rec in reversed(recs):
        r = _fp64_layer(rec)
        v = v @ (alpha * eye + (1 - alpha) * r.P.mean(1))
        eps += CB.rollout_tolerance(r, rec[1], N, rec[5])
    ref = (v / v.sum(-1, keepdim=True)).reshape(B, N)
    got = sal.reshape(B, N).double()
    ratio = ((got - ref).abs() / ((eps + 2.0 ** -22) * ref)).max().item()
    spread = (ref.max() / ref.min()).item()
    print(f"RATIO rollout {reduction} {img} {mode}: error / tolerance {ratio:.3f} (sum of eps_l {eps:.3g}, largest / smallest saliency {spread:.2f})")
    assert ratio <= CB.SLACK
    assert spread > 1.05, "the test's rollout is all but uniform: it would not tell the layers apart"


# ------------------------------------------------------------------------------------------------------------------ shape / layout
@pytest.mark.parametrize("img", [(32, 32), (48, 32)])
def test_maps_are_normalised_and_time_major(K, img):
    from simple_tad_amd import explain
    m = tiny(img=img)
    gh, gw = img[0] // PATCH, img[1] // PATCH
    N = (T_FRAMES // TUB) * gh * gw
    x = clip(3, img)
    logits, sal = explain.attention_rollout(m, x)
    assert logits.shape == (3, 2) and sal.shape == (3, T_FRAMES // TUB, gh, gw) and sal.dtype == torch.float32
    assert (sal >= 0).all() and float((sal.sum((1, 2, 3)) - 1).abs().max()) < 1e-5
    _, recs = _records(m, x)
    rec = explain.attention_received(recs)
    assert rec.shape == (3, 2, N) and (rec >= 0).all() and float((rec.sum(-1) - 1).abs().max()) < 1e-3
    fr = explain.saliency_to_frames(sal, (T_FRAMES, *img))
    assert fr.shape == (3, T_FRAMES, *img)
    assert torch.equal(fr[:, 3, 16:32, 0:16], sal[:, 1, 1, 0][:, None, None].expand(3, 16, 16))
    assert explain.saliency_to_frames(sal, (T_FRAMES, *img), mode="bilinear").shape == (3, T_FRAMES, *img)
    # one bright patch: tubelet 1, patch row gh - 1, patch column 0.  Block 0 is given weights under which every query looks for the bright
    # token: q = q_bias = beta (xn_b - mean_j xn_j) (the q rows of the weight are zero), k_j = xn_j (identity), so the score of key j is
    # beta scale (xn_b - mean) . xn_j per head: largest, by tens of nats, at j = b
    tp, py, px = 1, gh - 1, 0
    xb = torch.zeros(1, 3, T_FRAMES, *img, device="cuda")
    xb[:, :, tp * TUB:(tp + 1) * TUB, py * PATCH:(py + 1) * PATCH, px * PATCH:(px + 1) * PATCH] = 3.0
    blk = m.blocks[0]
    with torch.no_grad():
        tok = m.patch_embed(xb, pos_embed=m._pos_on(xb.device)).float().reshape(1, N, 128)
        xn = torch.nn.functional.layer_norm(tok, (128,), blk.norm1.weight, blk.norm1.bias, blk.norm1.eps)[0]
        b = (tp * gh + py) * gw + px  # time-major
        dirn = xn[b] - xn.mean(0)
        score = 0.125 * (xn.reshape(N, 2, 64) * dirn.reshape(1, 2, 64)).sum(-1)   # [N, heads] at beta = 1
        gap = (score[b] - torch.cat([score[:b], score[b + 1:]]).max(0).values).min().item()
        assert gap > 0, "the crafted direction does not single out the bright token"
        beta = 30.0 / gap
        blk.attn.qkv.weight.zero_()
        blk.attn.qkv.weight[128:256] = torch.eye(128, device="cuda")
        blk.attn.q_bias.copy_(beta * dirn)
    _, recs = _records(m, xb)
    got = explain.attention_received(recs, layer=0).mean(1).reshape(T_FRAMES // TUB, gh, gw)
    win = (got == got.max()).nonzero()[0].tolist()
    assert win == [tp, py, px] and float(got.max()) > 0.9, (win, float(got.max()))


# ------------------------------------------------------------------------------------------------------------------ score_video
def test_score_video_saliency():
    from simple_tad_amd import FrameStore, explain
    from simple_tad_amd.inference import score_video
    m = tiny()
    frames = torch.randint(0, 256, (9, 32, 32, 3), generator=torch.Generator().manual_seed(13), dtype=torch.uint8)
    kw = dict(orig_fps=10, target_fps=10, batch_size=4, mean=MEAN, std=STD)
    plain = score_video(m, frames, **kw)
    none = score_video(m, frames, saliency=None, **kw)
    assert list(plain) == list(none) == ["frame", "logits", "prob", "bytes_uploaded"]
    for k in ("frame", "logits", "prob"):
        assert same_bits(plain[k], none[k]), k
    store = FrameStore(9, 32, 32, "cuda")
    store.append(frames)
    table = torch.tensor([[s, s + 1, s + 2, s + 3] for s in range(6)]).cuda()
    batches = (store.frames[table[:4]], store.frames[table[4:]])  # a ragged last batch of two
    for kind, fn in (("rollout", explain.attention_rollout), ("received", explain.attention_received_map)):
        res = score_video(m, frames, saliency=kind, **kw)
        assert list(res) == ["frame", "logits", "prob", "bytes_uploaded", "saliency"]
        for k in ("frame", "logits", "prob"):
            assert same_bits(plain[k], res[k]), (kind, k)
        want = torch.cat([fn(m, b)[1] for b in batches])
        assert res["saliency"].dtype == torch.float32 and res["saliency"].device.type == "cpu" and res["saliency"].shape == (6, 2, 2, 2)
        assert same_bits(res["saliency"], want.cpu()), kind
        assert float((res["saliency"].sum((1, 2, 3)) - 1).abs().max()) < 1e-4
    assert not m.training
    short = score_video(m, frames[:3], orig_fps=10, target_fps=10, saliency="rollout")
    assert short["saliency"].shape == (0, 2, 2, 2) and short["logits"].shape == (0, 2)
    with pytest.raises(ValueError, match="saliency"):
        score_video(m, frames, saliency="gradcam", **kw)
    m.train()
    score_video(m, frames, saliency="rollout", **kw)
    assert m.training, "score_video must put the model's mode back"
