"""The InternVideo2 family on the scoring path: uint8 clips, frame-store windows, 16-bit operand clips, ``SlidingWindow`` (eager and
HIP-graph replay), ``score_video``, ``engine.final_test`` over ``StoreViews``, training from uint8 buffers -- and the fused evaluation
loop (ops.set_iv2_serve_kernels) against the module route it replaces.

The model is the TINY configuration of tests/iv2_recipe.py: 28 x 28, patch 14, 2 frames -> 8 + 1 tokens, D 128.  The input-stage
comparisons are bit for bit (the criterion of tests/test_input_stage.py: the same patch-matrix bits go into the same functions at the
same batch size).  Accuracy is held to the yardstick of tests/test_iv2_gpu.py: whole-tensor rel-L2 against the fp64 restatement, ours
<= 2 x what the restatement under torch.autocast deviates by.

Measured on an MI355X (evaluation logits, rel-L2 against fp64: switch on / off / the restatement under autocast): TINY fast 2.637e-3 /
2.637e-3 / 1.043e-2, TINY half 3.794e-4 / 3.794e-4 / 1.068e-3, on and off the same bits in all eight variant x mode cases; the real small
size (B 1, N 2049, D 384, fast, perturbed weights) 7.163e-4 / 7.002e-4 / 5.893e-3, on against off 1.607e-5.
"""
import csv
import types
from collections import OrderedDict
from contextlib import contextmanager

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import iv2_recipe as R
import simple_tad_amd as T
from oracle import vit_oracle as O
from simple_tad_amd import internvideo2 as IV2, kernels as K, ops
from simple_tad_amd._lib import TadError

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MODES = {"fast": torch.bfloat16, "half": torch.float16}
FACTOR = 2.0
HW, NF = 28, 2  # TINY's frame size and frames per window


@pytest.fixture(autouse=True)
def _restore_switches():
    yield
    ops.set_iv2_serve_kernels(True)
    ops.set_iv2_kernels(True)
    T.set_precision("fast")
    ops.invalidate_weight_cache()


def rel(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def build(**over):
    torch.manual_seed(0)
    m = IV2.InternVideo2(**dict(R.TINY, **R.REF_ROUTE, **over))
    R.perturb_(m.named_parameters())
    return m.cuda()


def u8(shape, seed):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def float_clips(clips_u8_rgb):
    """[B,T,H,W,3] uint8 RGB -> the loaders' normalised float clips [B,3,T,H,W] (dota.py: tensor_normalize)"""
    return torch.stack([O.tensor_normalize(c, MEAN, STD).permute(3, 0, 1, 2) for c in clips_u8_rgb]).contiguous()


@contextmanager
def counting(names):
    """call recorders around wrappers of simple_tad_amd.kernels (ops and the models look every one up on the module at call time): the
    pattern of tests/test_freeze_gpu.py"""
    calls, orig = [], {}
    for n in names:
        f = getattr(K, n)
        assert isinstance(f, types.FunctionType)
        orig[n] = f

        def rec(*a, _n=n, _f=f, **k):
            calls.append(_n)
            return _f(*a, **k)
        setattr(K, n, rec)
    try:
        yield calls
    finally:
        for n, f in orig.items():
            setattr(K, n, f)


# ------------------------------------------------------------------------------------------------ 1. the entry's input forms
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("bgr", [False, True])
def test_uint8_clip_equals_the_float_clip(mode, bgr):
    T.set_precision(mode)
    m = build().eval()
    m.patch_embed.set_input_normalization(MEAN, STD, bgr=bgr)
    frames = u8((2, NF, HW, HW, 3), 3)
    as_bgr = lambda f: f.numpy() if bgr else f.numpy()[..., ::-1]  # (clip_from_frames takes cv2's BGR frames)
    xf = torch.cat([O.clip_from_frames([as_bgr(frames[b, t]) for t in range(NF)], MEAN, STD) for b in range(2)])
    with torch.no_grad():
        a, b = m(frames.cuda()), m(xf.cuda())
    assert a.shape == (2, 2) and torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("bgr", [False, True])
def test_frame_windows_equal_the_materialised_clips(mode, bgr):
    from simple_tad_amd import FrameStore
    T.set_precision(mode)
    m = build().eval()
    m.patch_embed.set_input_normalization(MEAN, STD, bgr=bgr)
    store = FrameStore(7, HW, HW, "cuda", bgr=bgr)
    store.append(u8((7, HW, HW, 3), 4))
    table = [[0, 1], [5, 6], [0, 0], [6, 3], [1, 2]]
    fw = store.windows(table)
    clips = store.frames[torch.tensor(table).cuda()]
    assert torch.equal(fw.materialize(), clips)
    with torch.no_grad():
        a, b = m(fw), m(clips)
    assert a.shape == (5, 2) and torch.equal(a, b)


@pytest.mark.parametrize("mode", list(MODES))
def test_operand_clip_equals_its_upcast(mode):
    T.set_precision(mode)
    m = build().eval()
    x16 = R.clip().cuda().to(MODES[mode])
    with torch.no_grad():
        a, b = m(x16), m(x16.float())
        other = m(R.clip().cuda().to(torch.float16 if mode == "fast" else torch.bfloat16))  # the other 16-bit format: the upcast route
    assert torch.equal(a, b) and torch.isfinite(other).all()


def test_refusals_on_the_gpu_build():
    m = build().eval()
    with pytest.raises(AssertionError, match="Input image size"), torch.no_grad():
        m(torch.zeros(1, NF, 14, HW, 3, dtype=torch.uint8).cuda())
    with pytest.raises(TadError, match=r"\[B,T,H,W,3\]"), torch.no_grad():
        m(torch.zeros(NF, HW, HW, 3, dtype=torch.uint8).cuda())
    T.set_precision("precise")
    with pytest.raises(TadError, match="precise"), torch.no_grad():
        m(torch.zeros(1, NF, HW, HW, 3, dtype=torch.uint8).cuda())


# ------------------------------------------------------------------------------------------------ 2. SlidingWindow
@pytest.mark.parametrize("mode", list(MODES))
def test_sliding_window_eager_and_graph(mode):
    from simple_tad_amd.inference import SlidingWindow
    T.set_precision(mode)
    m = build().eval()
    frames = [u8((HW, HW, 3), 20 + i).numpy() for i in range(5)]  # two and a half laps of the two-slot ring (cv2-style BGR frames)
    sw = SlidingWindow(m, MEAN, STD, bgr=True)
    with pytest.raises(TadError, match="at least 2 frames"):
        sw.predict()
    eager = []
    for i, f in enumerate(frames):
        sw.push(f)
        if sw.full:
            eager.append(sw.predict())
            win = O.clip_from_frames(frames[i - 1:i + 1], MEAN, STD)
            with torch.no_grad():
                want = m(win.cuda())
            assert torch.equal(eager[-1], want), i
    assert len(eager) == 4 and not torch.equal(eager[0], eager[-1]) and m.patch_embed.t_offset == 0
    swg = SlidingWindow(m, MEAN, STD, bgr=True, use_graph=True)
    got = []
    for f in frames:
        swg.push(f)
        if swg.full:
            got.append(swg.predict())
    assert len(got) == 4 and len(swg._graphs) == 2 and all(torch.equal(a, b) for a, b in zip(got, eager))
    # the graphs follow the weights: an in-place update drops them
    with torch.no_grad():
        m.head.weight.mul_(2.0)
        m.blocks[0].mlp.fc1.weight.mul_(1.5)
        m.pos_embed.add_(0.25)
    a, b = swg.predict(), sw.predict()
    assert torch.equal(a, b) and len(swg._graphs) == 1 and not torch.equal(a, got[-1])


def test_sliding_window_graph_with_a_composed_position_table():
    from simple_tad_amd.inference import SlidingWindow
    m = build(sep_pos_embed=True).eval()
    frames = [u8((HW, HW, 3), 40 + i).numpy() for i in range(4)]
    swe, swg = SlidingWindow(m, MEAN, STD), SlidingWindow(m, MEAN, STD, use_graph=True)
    for f in frames:
        swe.push(f)
        swg.push(f)
        if swe.full:
            assert torch.equal(swg.predict(), swe.predict())
    with torch.no_grad():
        m.pos_embed_temporal.add_(0.5)
    assert torch.equal(swg.predict(), swe.predict()) and len(swg._graphs) == 1


# ------------------------------------------------------------------------------------------------ 3. score_video, final_test
@pytest.mark.parametrize("bgr", [False, True])
def test_score_video(bgr):
    from simple_tad_amd import FrameStore
    from simple_tad_amd.inference import score_video
    m = build().eval()
    frames = u8((7, HW, HW, 3), 13)
    four = score_video(m, frames.numpy(), orig_fps=10, target_fps=10, batch_size=4, mean=MEAN, std=STD, bgr=bgr)
    assert four["frame"].tolist() == [1, 2, 3, 4, 5, 6] and four["logits"].shape == (6, 2) and four["bytes_uploaded"] == 7 * HW * HW * 3
    store = FrameStore(7, HW, HW, "cuda", bgr=bgr)
    store.append(frames)
    table = torch.tensor([[s, s + 1] for s in range(6)]).cuda()
    with torch.no_grad():
        want = torch.cat([m(store.frames[table[:4]]), m(store.frames[table[4:]])])
    assert torch.equal(four["logits"], want.cpu()) and not m.training
    assert torch.equal(four["prob"], torch.softmax(four["logits"].cuda(), dim=1)[:, 1].cpu())
    short = score_video(m, frames[:1], orig_fps=10, target_fps=10)
    assert short["frame"].shape == (0,) and short["logits"].shape == (0, 2) and short["prob"].shape == (0,)
    with pytest.raises(TadError, match="no attention the capture could see"):
        score_video(m, frames, orig_fps=10, target_fps=10, saliency="rollout")


def test_final_test_over_store_views(tmp_path):
    from simple_tad_amd import FrameStore, StoreViews
    from simple_tad_amd import engine as E
    from simple_tad_amd.sequencing import RegularSequencer
    m = build()
    sv = StoreViews(FrameStore(12, HW, HW, "cuda"))
    la, lb = [0, 0, 1, 1, 0, 0, 1], [0, 1, 1, 0, 0]
    sv.add_video("vid_a", u8((7, HW, HW, 3), 21), [f"a/{i:04d}.jpg" for i in range(7)], la, np.arange(7, dtype=np.float32))
    sv.add_video("vid_b", u8((5, HW, HW, 3), 22).numpy(), [f"b/{i:04d}.jpg" for i in range(5)], lb, np.arange(5, dtype=np.float32))
    seq = RegularSequencer(10, NF, 1)
    parsed = {}
    for what, loader in (("store", lambda: sv.batches(seq, 10, batch_size=4)),
                         ("clips", lambda: [(b[0].materialize(), *b[1:]) for b in sv.batches(seq, 10, batch_size=4)])):
        preds = tmp_path / f"{what}.csv"
        E.final_test(loader(), m, torch.device("cuda"), preds, tmp_path / f"{what}.txt")
        rows = list(csv.reader(open(preds, newline="")))[1:]
        assert len(rows) == 6 + 4 and [r[1] for r in rows] == ["vid_a"] * 6 + ["vid_b"] * 4
        parsed[what] = rows
    assert parsed["store"] == parsed["clips"] and not m.training
    with torch.no_grad():
        logits = torch.cat([m(b[0]) for b in sv.batches(seq, 10, batch_size=4)]).float().cpu()
    got = torch.tensor([[float(r[3]), float(r[4])] for r in parsed["store"]], dtype=torch.float64).to(torch.float32)
    assert torch.equal(got, logits)


# ------------------------------------------------------------------------------------------------ 4. training from uint8 buffers
def grads_of(m, x):
    m.zero_grad(set_to_none=True)
    logits = m(x)
    F.cross_entropy(logits, torch.tensor([0, 1, 1][:logits.shape[0]]).cuda()).backward()
    return logits.detach(), OrderedDict((k, p.grad.clone()) for k, p in m.named_parameters())


@pytest.mark.parametrize("mode", list(MODES))
def test_training_from_uint8_clips_and_from_a_store(mode):
    from simple_tad_amd import FrameStore
    T.set_precision(mode)
    m = build().train()
    m.patch_embed.set_input_normalization(MEAN, STD, bgr=False)
    store = FrameStore(6, HW, HW, "cuda")
    store.append(u8((6, HW, HW, 3), 31))
    table = [[0, 1], [4, 5], [2, 2]]
    clips = store.frames[torch.tensor(table).cuda()]
    l_f, g_f = grads_of(m, float_clips(clips.cpu()).cuda())
    for what, x in (("uint8 clips", clips), ("store windows", store.windows(table))):
        l, g = grads_of(m, x)
        assert torch.equal(l, l_f), what
        assert set(g) == set(g_f) and "cls_token" in g and "pos_embed" in g
        for k in g_f:
            assert torch.equal(g[k], g_f[k]), f"{what}: {k}"
    assert all(v.abs().sum() > 0 for k, v in g_f.items() if "norm1_k.bias" not in k and "k_bias" not in k)


def test_gradient_sinks_of_the_entry():
    """the optimizer's flat-buffer sinks: cls_token and pos_embed receive the kernel's sums in place; a composed sep_pos_embed table
    receives its gradient as a tensor and autograd carries it to the three parts"""
    from simple_tad_amd.optim import FusedAdamW
    x = R.clip().cuda()
    for over in ({}, {"sep_pos_embed": True}):
        plain, sunk = build(**over).train(), build(**over).train()
        _, want = grads_of(plain, x)
        opt = FusedAdamW(sunk.parameters(), lr=0.0)
        sunk.zero_grad(set_to_none=False)
        with counting(["class_token_entry_bwd"]) as calls:
            F.cross_entropy(sunk(x), torch.tensor([0, 1]).cuda()).backward()
        assert calls == ["class_token_entry_bwd"]
        entry = [k for k in want if k.startswith(("cls_token", "pos_embed"))]
        assert len(entry) == (4 if over else 2)
        for k, p in sunk.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
            if k in entry:  # (the kernel's sum added onto a zeroed sink, or autograd's += of the returned tensor: the same bits)
                assert torch.equal(p.grad, want[k]) and p.grad.abs().sum() > 0, f"{over}: {k}"
        del opt


# ------------------------------------------------------------------------------------------------ 5. the switch
_REF = {}


def references(over=()):
    """per variant: fp64 logits of the restatement on the device, and per mode the restatement under autocast; computed once"""
    key = tuple(sorted(dict(over).items()))
    if key not in _REF:
        cfg = dict(R.TINY, **dict(over))
        m = build(**dict(over))
        x = R.clip().cuda()
        with torch.no_grad():
            ref = R.model(R.leaves(m.named_parameters(), dtype=torch.float64), x.double(), cfg)
            P = OrderedDict((k, v.detach()) for k, v in m.named_parameters())
            yard = {}
            for mode, dt in MODES.items():
                with torch.autocast(device_type="cuda", dtype=dt):
                    yard[mode] = R.model(P, x, cfg).float()
        _REF[key] = (ref, yard)
    return _REF[key]


@pytest.mark.parametrize("over", [{}, {"sep_pos_embed": True}, {"init_values": 0}, {"qkv_bias": True, "qk_normalization": False, "init_values": 0}],
                         ids=["tiny", "sep_pos", "no_layerscale", "plain_attn"])
@pytest.mark.parametrize("mode", list(MODES))
def test_switch_on_against_switch_off(mode, over):
    T.set_precision(mode)
    m = build(**over)
    x = R.clip().cuda()
    ref, yard = references(over)
    out = {}
    for on in (True, False):
        ops.set_iv2_serve_kernels(on)
        m.train()
        train = m(x).detach()
        m.eval()
        with torch.no_grad():
            out[on] = (train, m(x))
    assert torch.equal(out[True][0], out[False][0]), "training logits are the same bits with the switch on and off"
    ey = rel(yard[mode], ref)
    e_on, e_off = rel(out[True][1], ref), rel(out[False][1], ref)
    diff = rel(out[True][1], out[False][1])
    print(f"{over or 'tiny'} {mode}: evaluation logits rel-L2 against fp64: on {e_on:.3e}  off {e_off:.3e}  autocast {ey:.3e}; on against off {diff:.3e}")
    assert e_on <= FACTOR * ey and e_off <= FACTOR * ey


def test_launch_count_of_the_evaluation_forward():
    m = build().eval()
    x = R.clip().cuda()
    names = ["residual_rmsnorm", "rmsnorm_fwd", "class_token_entry_fwd"]
    with counting(names) as calls, torch.no_grad():
        m(x)
    assert calls.count("residual_rmsnorm") == 4 and calls.count("rmsnorm_fwd") == 1 and calls.count("class_token_entry_fwd") == 1
    assert calls[:2] == ["class_token_entry_fwd", "rmsnorm_fwd"]
    ops.set_iv2_serve_kernels(False)
    with counting(names) as calls, torch.no_grad():
        m(x)
    assert calls == ["rmsnorm_fwd"] * 4, "off: the module route, and the torch cat + add"
    ops.set_iv2_serve_kernels(True)
    with counting(names) as calls:
        m(x)
    assert calls.count("residual_rmsnorm") == 0 and calls.count("rmsnorm_fwd") == 4, "with gradients enabled nothing about the blocks changes"
    m.train()
    m.blocks[1].drop_path1 = IV2.DropPath(0.5)
    with counting(names) as calls, torch.no_grad():
        m(x)
    assert calls.count("residual_rmsnorm") == 0, "a model left in training mode with a DropPath keeps the module route"


def test_real_small_size_evaluation_forward():
    """B = 1, N = 2049, D = 384: the shape the sliding window serves"""
    torch.manual_seed(0)
    m = T.create_model("internvideo2_small_patch14_224", num_classes=2)
    R.perturb_(m.named_parameters())
    m = m.cuda().eval()
    cfg = dict(embed_dim=384, num_heads=6, depth=12, attn_pool_num_heads=16, patch_size=14, tubelet_size=1)
    x = torch.randn(1, 3, 8, 224, 224, generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        ref = R.model(R.leaves(m.named_parameters(), dtype=torch.float64), x.double(), cfg)
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            yard = R.model(OrderedDict((k, v.detach()) for k, v in m.named_parameters()), x, cfg).float()
        with counting(["residual_rmsnorm"]) as calls:
            on = m(x)
        ops.set_iv2_serve_kernels(False)
        off = m(x)
    assert calls == ["residual_rmsnorm"] * 24 and on.shape == (1, 2) and torch.isfinite(on).all()
    e_on, e_off, ey = rel(on, ref), rel(off, ref), rel(yard, ref)
    print(f"small, B 1: rel-L2 against fp64: on {e_on:.3e}  off {e_off:.3e}  autocast {ey:.3e}; on against off {rel(on, off):.3e}")
    assert e_on <= FACTOR * ey and e_off <= FACTOR * ey
