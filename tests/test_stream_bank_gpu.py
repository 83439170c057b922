"""StreamBank on the GPU, for both model families (the TINY configurations of tests/test_frame_resize_gpu.py and tests/iv2_recipe.py):
three cameras fed different numbers of frames of different sizes, so their rings sit at different phases and one has wrapped.  The
bank's logits must be, bit for bit, those of the model on uint8 clips materialised in temporal order from frames resized one by one
(``resize_frames``) at the same batch size; with one stream, those of a ``SlidingWindow`` fed the same frames; and the same with captured
graphs as without, across a change of the batch size and across a weight change."""
import numpy as np
import pytest
import torch

import iv2_recipe as R
import simple_tad_amd as T
from simple_tad_amd import internvideo2 as IV2, ops
from simple_tad_amd._lib import TadError
from simple_tad_amd.frame_resize import resize_frames
from simple_tad_amd.inference import SlidingWindow

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
S = 3


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


def frame(h, w, seed):
    return np.random.RandomState(1000 * seed + 7 * h + w).randint(0, 256, (h, w, 3)).astype(np.uint8)


def script(Tn, H, W):
    """the ticks of three cameras: [(stream, frame), ...] per tick.  Camera 0 delivers 45 x 80 frames and ends with exactly T of them;
    camera 1 switches between 20 x 23 and 9 x 13 and delivers 2T + 1 (its ring wraps twice and ends one slot in); camera 2 delivers
    frames at the model's own size, starts late and drops every other tick: T - 1 frames, not ready."""
    ticks, n = [], 2 * Tn + 1
    for i in range(n):
        tick = []
        if i >= n - Tn:
            tick.append((0, frame(45, 80, i)))
        tick.append((1, frame(*((20, 23) if i % 2 else (9, 13)), 100 + i)))
        if i >= 3 and i % 2 and sum(1 for t in ticks for s, _ in t if s == 2) < Tn - 1:
            tick.append((2, frame(H, W, 200 + i)))
        ticks.append(tick[::-1] if i % 3 == 0 else tick)                                    # the order of the ids in a call is free
    return ticks


class Windows:
    """the reference: per camera the last T frames, each resized on its own with the one-size kernel"""

    def __init__(self, Tn, H, W, flip=()):
        self.T, self.size, self.flip = Tn, (H, W), set(flip)
        self.win = {s: [] for s in range(S)}

    def push(self, s, f):
        r = resize_frames(torch.from_numpy(f[None]).cuda(), self.size)[0]
        self.win[s] = (self.win[s] + [r.flip(-1) if s in self.flip else r])[-self.T:]

    def reset(self, s):
        self.win[s] = []

    def clips(self, ids):
        return torch.stack([torch.stack(self.win[s]) for s in ids]).contiguous()


def run(bank, ref, ticks):
    for tick in ticks:
        bank.push_raw([s for s, _ in tick], [f if k % 2 else torch.from_numpy(f) for k, (_, f) in enumerate(tick)])
        for s, f in tick:
            ref.push(s, f)


def reference_logits(model, ref, ids, bgr):
    model.patch_embed.set_input_normalization(MEAN, STD, bgr=bgr)
    with torch.no_grad():
        return model(ref.clips(ids)).float()


def test_predict_equals_the_model_on_materialised_clips(model):
    Tn, (H, W) = int(model.num_frames), model.patch_embed.img_size
    bank, ref = T.StreamBank(model, streams=S, mean=MEAN, std=STD, bgr=True), Windows(Tn, H, W)
    assert bank.store.shape == (S * Tn, H, W, 3) and bank.ready == []
    empty = bank.predict()
    assert empty["stream"].shape == (0,) and empty["logits"].shape == (0, 2) and empty["prob"].shape == (0,)
    assert empty["stream"].dtype == torch.int64 and empty["logits"].dtype == empty["prob"].dtype == torch.float32
    run(bank, ref, script(Tn, H, W))
    assert bank.count == [Tn, 2 * Tn + 1, Tn - 1] and bank.start == [0, 1 % Tn, 0] and bank.ready == [0, 1]
    got = bank.predict()
    want = reference_logits(model, ref, [0, 1], True)
    assert got["stream"].tolist() == [0, 1] and torch.equal(got["logits"], want)
    assert torch.equal(got["prob"], torch.softmax(want, dim=1)[:, 1])
    assert not model.training and model.patch_embed.t_offset == 0
    # the store holds what the one-size kernel gives, frame by frame, in the rings' slots
    for s in (0, 1):
        order = [s * Tn + (bank.start[s] + t) % Tn for t in range(Tn)]
        assert torch.equal(bank.store[order], torch.stack(ref.win[s]))
    # an explicit order, and one stream at a time: the same batch size as the reference's
    assert torch.equal(bank.predict([1, 0])["logits"], reference_logits(model, ref, [1, 0], True))
    assert torch.equal(bank.predict([1])["logits"], reference_logits(model, ref, [1], True))
    with pytest.raises(TadError, match=rf"We need at least {Tn} frames! \(stream 2 has {Tn - 1}\)"):
        bank.predict([0, 2])
    # camera 2 catches up through push (frames at the model's size, on the device): all three are ready
    f = frame(H, W, 300)
    bank.push(np.asarray([2]), torch.from_numpy(f[None]).cuda())
    ref.push(2, f)
    assert bank.ready == [0, 1, 2]
    assert torch.equal(bank.store[2 * Tn + Tn - 1].cpu(), torch.from_numpy(f)), "equal extents give the input bytes back"
    assert torch.equal(bank.predict()["logits"], reference_logits(model, ref, [0, 1, 2], True))
    # camera 1 reconnects: it is not ready until it has T new frames, the others are not disturbed
    bank.reset(1)
    ref.reset(1)
    assert bank.ready == [0, 2] and bank.count[1] == 0
    assert torch.equal(bank.predict()["logits"], reference_logits(model, ref, [0, 2], True))
    for i in range(Tn):
        with pytest.raises(TadError, match="We need at least"):
            bank.predict([1])
        g = frame(20, 23, 400 + i)
        bank.push_raw([1], [g])
        ref.push(1, g)
    assert torch.equal(bank.predict()["logits"], reference_logits(model, ref, [0, 1, 2], True))


def test_one_stream_equals_a_sliding_window(model):
    Tn, (H, W) = int(model.num_frames), model.patch_embed.img_size
    bank = T.StreamBank(model, streams=S, mean=MEAN, std=STD, bgr=True)
    wins = [SlidingWindow(model, MEAN, STD, bgr=True) for _ in range(S)]
    checked = 0
    for tick in script(Tn, H, W):
        bank.push_raw([s for s, _ in tick], [f for _, f in tick])
        for s, f in tick:
            wins[s].push_raw(f)
        for s in bank.ready:
            assert (bank.count[s], bank.start[s]) == (wins[s].count, wins[s].start)
            assert torch.equal(bank.predict([s])["logits"], wins[s].predict().float()), (s, bank.count[s])
            checked += 1
    assert checked >= Tn + 2 and not wins[2].full


def test_graphs_give_the_eager_bits_across_batch_sizes_and_a_weight_change(model):
    Tn, (H, W) = int(model.num_frames), model.patch_embed.img_size
    eager, graph = T.StreamBank(model, S, MEAN, STD, bgr=True), T.StreamBank(model, S, MEAN, STD, bgr=True, use_graph=True)
    ticks = script(Tn, H, W)
    sizes = []
    for tick in ticks + [[(2, frame(H, W, 500))], [(0, frame(30, 30, 501)), (1, frame(9, 13, 502))]]:
        for b in (eager, graph):
            b.push_raw([s for s, _ in tick], [f for _, f in tick])
        assert torch.equal(eager.store, graph.store)
        a, g = eager.predict(), graph.predict()
        assert a["stream"].tolist() == g["stream"].tolist() and torch.equal(a["logits"], g["logits"]) and torch.equal(a["prob"], g["prob"])
        sizes.append(len(a["stream"]))
    assert {1, 2, 3} <= set(sizes) and sorted(graph._graphs) == [1, 2, 3], "one graph per batch size, each built once"
    held = dict(graph._graphs)
    g2 = graph.predict([0, 2])
    assert graph._graphs[2] is held[2] and torch.equal(g2["logits"], eager.predict([0, 2])["logits"]), "another pair of streams, the same graph"
    before = eager.predict()["logits"]
    with torch.no_grad():                                                                  # a weight change drops the graphs
        for p in model.parameters():
            p.mul_(1.01)
    a, g = eager.predict(), graph.predict()
    assert sorted(graph._graphs) == [3] and graph._graphs[3] is not held[3]
    assert torch.equal(a["logits"], g["logits"]) and not torch.equal(a["logits"], before)
    assert torch.equal(eager.predict([1])["logits"], graph.predict([1])["logits"])
    assert not model.training and model.patch_embed.t_offset == 0


def test_cameras_of_both_channel_orders_fill_one_store(model):
    Tn, (H, W) = int(model.num_frames), model.patch_embed.img_size
    bank = T.StreamBank(model, S, MEAN, STD, bgr=[True, False, True])
    assert bank.store_bgr is False and bank.swap == [True, False, True]
    ref = Windows(Tn, H, W, flip=(0, 2))
    ticks = script(Tn, H, W) + [[(2, frame(H, W, 600))]]
    run(bank, ref, ticks)
    assert bank.ready == [0, 1, 2]
    assert torch.equal(bank.predict()["logits"], reference_logits(model, ref, [0, 1, 2], False))
    # every camera RGB, every camera BGR: the store keeps the cameras' order and nothing is swapped
    for order in (False, True):
        same = T.StreamBank(model, S, MEAN, STD, bgr=[order] * S)
        assert same.store_bgr is order and same.swap == [False] * S
        ref = Windows(Tn, H, W)
        run(same, ref, ticks)
        assert torch.equal(same.predict()["logits"], reference_logits(model, ref, [0, 1, 2], order))
    with pytest.raises(TadError, match="bgr names 2 streams"):
        T.StreamBank(model, S, MEAN, STD, bgr=[True, False])


def test_refusals_leave_the_bank_as_it_was(model):
    Tn, (H, W) = int(model.num_frames), model.patch_embed.img_size
    bank = T.StreamBank(model, S, MEAN, STD)
    bank.push_raw([0, 2], [frame(5, 7, 1), frame(9, 4, 2)])
    state = (list(bank.count), list(bank.start), bank.store.clone())
    ok = frame(6, 6, 3)
    for ids, frames, exc, text in (([1, 1], [ok, ok], TadError, "stream id 1 is named twice"),
                                   ([0, 3], [ok, ok], TadError, r"stream id 3 outside \[0, 3\)"),
                                   ([-1], [ok], TadError, "stream id -1 outside"),
                                   ([0, 1], [ok], TadError, "2 stream ids and 1 frames"),
                                   ([0, 1], [ok, ok.astype(np.float32)], TypeError, "Input 1 must be a uint8 image"),
                                   ([0], [ok[..., :2]], TypeError, "Input 0 must be a uint8 image"),
                                   ([0], [ok[:0]], TypeError, "Input 0 must be a uint8 image"),
                                   ([0], [ok[None]], TypeError, "Input 0 must be a uint8 image"),
                                   ([0], ["frame.jpg"], TypeError, "but got str")):
        with pytest.raises(exc, match=text):
            bank.push_raw(ids, frames)
    with pytest.raises(TypeError, match="Input must be uint8 frames of shape"):
        bank.push([0], np.zeros((1, H + 1, W, 3), np.uint8))
    with pytest.raises(TadError, match="named twice"):
        bank.predict([0, 0])
    with pytest.raises(TadError, match="outside"):
        bank.reset(S)
    bank.push_raw([], [])                                                                   # an empty tick is no launch and no change
    assert (bank.count, bank.start) == state[:2] and torch.equal(bank.store, state[2])
    T.set_precision("precise")
    for call in (lambda: bank.push_raw([1], [ok]), lambda: bank.predict(), lambda: T.StreamBank(model, S, MEAN, STD)):
        with pytest.raises(TadError, match=r'precision "precise" takes the normalised f32 clip \(the uint8 input stage feeds the bf16 path\)'):
            call()
    T.set_precision("fast")
    assert (bank.count, bank.start) == state[:2] and torch.equal(bank.store, state[2])
    with pytest.raises(TadError, match=r"streams=0 must be in"):
        T.StreamBank(model, 0, MEAN, STD)
