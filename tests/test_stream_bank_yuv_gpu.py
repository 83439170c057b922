"""StreamBank.push_yuv on the GPU, for both model families (the TINY configurations of tests/test_stream_bank_gpu.py): three cameras
that deliver 4:2:0 YUV surfaces -- NV12 pitched, I420, NV21 -- at different phases of their rings, against a second bank fed
``push_raw`` with the frames the recipe (tests/yuv_recipe.py) converted to RGB on the host.  The stores must be equal byte for byte and
the logits bit for bit; a bank may mix ``push_raw`` and ``push_yuv`` cameras under either channel order of the store; a refusal leaves
counts, starts and store as they were."""
import numpy as np
import pytest
import torch

import iv2_recipe as R
import yuv_recipe as Y
import simple_tad_amd as T
from simple_tad_amd import internvideo2 as IV2, ops
from simple_tad_amd._lib import TadError

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
S = 3
CSETS = Y.colour_sets()
# per camera: extents, format, pitch padding, matrix
CAMERAS = [dict(hw=(45, 80), fmt="nv12", pad=16, matrix="bt601"), dict(hw=(21, 23), fmt="i420", pad=0, matrix="bt709"),
           dict(hw=(9, 13), fmt="nv21", pad=3, matrix="bt601-full")]


@pytest.fixture(autouse=True)
def _restore_switches():
    yield
    T.set_precision("fast")
    ops.invalidate_weight_cache()


def vit():
    torch.manual_seed(0)
    return T.VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True, all_frames=4,
                               tubelet_size=2, num_classes=2, init_scale=1.0).cuda().eval()


def iv2():
    torch.manual_seed(0)
    m = IV2.InternVideo2(**dict(R.TINY, **R.REF_ROUTE))
    R.perturb_(m.named_parameters())
    return m.cuda().eval()


FAMILIES = {"vit": vit, "iv2": iv2}


@pytest.fixture(params=list(FAMILIES))
def model(request):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return FAMILIES[request.param]()


def shot(cam, seed):
    """(YuvFrame, the recipe's RGB frame) of one picture of camera ``cam``"""
    c = CAMERAS[cam]
    h, w = c["hw"]
    planes = Y.planes(h, w, 1000 * cam + seed)
    step = 1 if c["fmt"] == "i420" else 2
    yp, cp = w + c["pad"], (w + 1) // 2 * step + c["pad"]
    buf, lay = Y.pack(*planes, c["fmt"], yp, cp, fill=0x3C)
    return T.YuvFrame(buf, h, w, c["fmt"], yp, cp, c["matrix"]), Y.convert(*planes, CSETS[c["matrix"]])


def script(Tn):
    """the ticks: camera 0 ends with exactly T frames, camera 1 delivers 2T + 1 (its ring wraps twice), camera 2 starts late and
    drops every other tick: T - 1 frames, not ready"""
    ticks, n, late = [], 2 * Tn + 1, 0
    for i in range(n):
        tick = []
        if i >= n - Tn:
            tick.append(0)
        tick.append(1)
        if i >= 3 and i % 2 and late < Tn - 1:
            tick.append(2)
            late += 1
        ticks.append(tick[::-1] if i % 3 == 0 else tick)
    return ticks


def feed(yuv, raw, ticks, yuv_cams=(0, 1, 2), seed0=0):
    """tick by tick: ``yuv`` gets the YUV cameras through push_yuv (and the others through push_raw, if it is one bank that mixes
    them), ``raw`` gets every camera's recipe-converted RGB frame through push_raw"""
    for i, tick in enumerate(ticks):
        shots = {s: shot(s, seed0 + i) for s in tick}
        a = [s for s in tick if s in yuv_cams]
        b = [s for s in tick if s not in yuv_cams]
        if a:
            yuv.push_yuv(a, [shots[s][0] for s in a])
        if b:
            yuv.push_raw(b, [shots[s][1] for s in b])
        raw.push_raw(tick, [shots[s][1] for s in tick])


def same(a, b):
    assert a.count == b.count and a.start == b.start and a.ready == b.ready
    assert torch.equal(a.store, b.store)
    if a.ready:
        x, y = a.predict(), b.predict()
        assert x["stream"].tolist() == y["stream"].tolist() and torch.equal(x["logits"], y["logits"]) and torch.equal(x["prob"], y["prob"])


def test_push_yuv_equals_push_raw_of_the_converted_frames(model):
    Tn = int(model.num_frames)
    # the reference bank takes RGB frames: bgr=False.  The YUV bank is told nothing about its cameras' order; its store is RGB too
    yuv, raw = T.StreamBank(model, S, MEAN, STD, bgr=False), T.StreamBank(model, S, MEAN, STD, bgr=False)
    feed(yuv, raw, script(Tn))
    assert yuv.count == [Tn, 2 * Tn + 1, Tn - 1] and yuv.start == [0, 1 % Tn, 0] and yuv.ready == [0, 1], "ring wrap, as push_raw assigns it"
    same(yuv, raw)
    assert torch.equal(yuv.predict([1])["logits"], raw.predict([1])["logits"])
    # camera 2 catches up with a bare uint8 [h * 3 / 2, w] array: a contiguous NV12 frame, BT.601
    h, w = 12, 10
    planes = Y.planes(h, w, 9)
    buf, _ = Y.pack(*planes, "nv12")
    yuv.push_yuv([2], [buf.reshape(h * 3 // 2, w)])
    raw.push_raw([2], [Y.convert(*planes, CSETS["bt601"])])
    assert yuv.ready == [0, 1, 2]
    same(yuv, raw)
    # reset: camera 1 reconnects and fills again
    yuv.reset(1)
    raw.reset(1)
    assert yuv.ready == [0, 2] and yuv.count[1] == 0
    same(yuv, raw)
    for i in range(Tn):
        f, rgb = shot(1, 500 + i)
        yuv.push_yuv([1], [f])
        raw.push_raw([1], [rgb])
    assert yuv.ready == [0, 1, 2]
    same(yuv, raw)


@pytest.mark.parametrize("store_bgr", [False, True])
def test_one_bank_mixes_push_raw_and_push_yuv(model, store_bgr):
    """camera 1 delivers decoded frames through push_raw, cameras 0 and 2 YUV surfaces through push_yuv, into one store of either
    channel order: the YUV rows write B first exactly when the store is BGR.  The reference bank is fed the converted frames in the
    store's order."""
    Tn = int(model.num_frames)
    mixed, raw = T.StreamBank(model, S, MEAN, STD, bgr=store_bgr), T.StreamBank(model, S, MEAN, STD, bgr=store_bgr)
    assert mixed.store_bgr is store_bgr
    for i, tick in enumerate(script(Tn) + [[2]]):
        shots = {s: shot(s, i) for s in tick}
        order = lambda rgb: np.ascontiguousarray(rgb[..., ::-1]) if store_bgr else rgb
        a, b = [s for s in tick if s != 1], [s for s in tick if s == 1]
        if a:
            mixed.push_yuv(a, [shots[s][0] for s in a])
        if b:
            mixed.push_raw(b, [order(shots[s][1]) for s in b])
        raw.push_raw(tick, [order(shots[s][1]) for s in tick])
    assert mixed.ready == [0, 1, 2]
    same(mixed, raw)
    # cameras of both orders in one bank: the store is RGB, the BGR camera is swapped on its way in, the YUV cameras write R first
    both = T.StreamBank(model, S, MEAN, STD, bgr=[True, True, False])
    ref = T.StreamBank(model, S, MEAN, STD, bgr=False)
    assert both.store_bgr is False
    for i in range(Tn):
        (f0, rgb0), (_, rgb1) = shot(0, 700 + i), shot(1, 700 + i)
        both.push_yuv([0], [f0])
        both.push_raw([1], [np.ascontiguousarray(rgb1[..., ::-1])])
        ref.push_raw([0, 1], [rgb0, rgb1])
    same(both, ref)


def test_refusals_leave_the_bank_as_it_was(model):
    bank = T.StreamBank(model, S, MEAN, STD)
    ok, _ = shot(2, 1)
    bank.push_yuv([0, 2], [shot(0, 0)[0], ok])
    state = (list(bank.count), list(bank.start), bank.store.clone())
    for ids, frames, exc, text in (([1, 1], [ok, ok], TadError, "stream id 1 is named twice"),
                                   ([0, 3], [ok, ok], TadError, r"stream id 3 outside \[0, 3\)"),
                                   ([0, 1], [ok], TadError, "2 stream ids and 1 frames"),
                                   ([0, 1], [ok, np.zeros((9, 7), np.uint8)], TypeError, "Input 1 must be a YuvFrame or a uint8 array"),
                                   ([0], [np.zeros((6, 6, 3), np.uint8)], TypeError, "Input 0 must be a YuvFrame or a uint8 array"),
                                   ([0], ["frame.yuv"], TypeError, "but got str")):
        with pytest.raises(exc, match=text):
            bank.push_yuv(ids, frames)
    with pytest.raises(TadError, match="at most 16"):                                       # too many colour sets for one launch
        many = T.StreamBank(model, 17, MEAN, STD)
        many.push_yuv(list(range(17)), [T.YuvFrame(np.zeros(6, np.uint8), 2, 2, matrix=(16, 1 << 20, 1000 + i, 0, 0, 0)) for i in range(17)])
    assert many.count == [0] * 17 and not many.store.any()
    bank.push_yuv([], [])                                                                   # an empty tick is no launch and no change
    assert (bank.count, bank.start) == state[:2] and torch.equal(bank.store, state[2])
    T.set_precision("precise")
    with pytest.raises(TadError, match=r'precision "precise" takes the normalised f32 clip'):
        bank.push_yuv([1], [ok])
    T.set_precision("fast")
    assert (bank.count, bank.start) == state[:2] and torch.equal(bank.store, state[2])
