"""The frame ingest on the GPU: tad_frame_resize against the numpy restatement of the contract (tests/frame_resize_recipe.py), bit for
bit over whole tensors -- the resize at the smallest extents at which each branch can go wrong, the five pad modes, writes into a slot
of a larger buffer, guard bands -- and the three public paths (``FrameStore.append_resized``, ``score_video(resize=True)``,
``SlidingWindow.push_raw``) against the same model on recipe-resized frames.  Every table here is valid: the kernel's clamps are never
exercised; refusals are the host's (tests/test_frame_resize_cpu.py)."""
import numpy as np
import pytest
import torch

import frame_resize_recipe as R
from guarded import GuardedArena, POISON_MODES, same_bits

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ALL_SHAPES = R.SHAPES + R.EXTRA_SHAPES
IDS = [f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in ALL_SHAPES]


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import _lib, kernels
    _lib.load()
    return kernels


@pytest.fixture(scope="module")
def FR(K):
    from simple_tad_amd import frame_resize
    return frame_resize


def six(H, W):
    """uint8 [6,H,W,3]: noise, smooth and step images under two seeds"""
    return np.concatenate([R.images(H, W, 0), R.images(H, W, 1)])


# ------------------------------------------------------------------------------------------------ 1. the resize
@pytest.mark.parametrize("src,dst", ALL_SHAPES, ids=IDS)
def test_resize_equals_the_recipe_bit_for_bit(K, FR, src, dst):
    im = six(*src)
    want = R.resize(im, *dst)                                                      # computed once, shared by every layout
    for frames in (im[:1], im[:3], im.reshape(2, 3, *src, 3)):
        x = torch.from_numpy(frames).cuda()
        w = torch.from_numpy(want[:frames.size // (src[0] * src[1] * 3)].reshape(*frames.shape[:-3], *dst, 3))
        got = FR.resize_frames(x, dst)
        assert got.dtype == torch.uint8 and got.shape == w.shape and torch.equal(got.cpu(), w)
        clip = FR.resize_frames(x, dst, MEAN, STD)
        ref = K.frames_to_clip(got if got.dim() == 5 else got.unsqueeze(0), MEAN, STD)
        assert clip.dtype == torch.float32 and same_bits(clip if x.dim() == 5 else clip.unsqueeze(0), ref)
    if src == dst:
        assert np.array_equal(want, im)                                            # the identity


def test_saturation_on_both_sides(FR):
    step = R.images(45, 80)[2:]
    un = R.resize_unclipped(step, 28, 28)
    assert un.min() < 0 and un.max() > 255                                         # the clip is exercised, low and high
    got = FR.resize_frames(torch.from_numpy(step).cuda(), 28).cpu().numpy()
    assert np.array_equal(got, np.clip(un, 0, 255).astype(np.uint8)) and got.min() == 0 and got.max() == 255


# ------------------------------------------------------------------------------------------------ 2. the pad modes
H0, W0, S0 = 45, 80, 28


@pytest.fixture(scope="module")
def clips():
    """uint8 [2,3,45,80,3]"""
    return six(H0, W0).reshape(2, 3, H0, W0, 3)


def pad_of(mode, top, bottom):
    return (mode, top, bottom, 0.37, (3, 200, 77) if mode == "color" else (0, 0, 0))


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("top,bottom", [(0, 17), (11, 0), (H0, H0), (1, 2)], ids=["top0", "bottom0", "max", "small"])
def test_pad_mode_equals_the_recipe(FR, clips, mode, top, bottom):
    plan = [pad_of(mode, top, bottom), pad_of(mode, top, bottom)]
    got = FR.PadWideClips(S0)(torch.from_numpy(clips).cuda(), plan=plan)
    want = np.stack([R.pad_resize(clips[b], plan[b], S0) for b in range(2)])
    assert got.shape == (2, 3, S0, S0, 3) and np.array_equal(got.cpu().numpy(), want)
    if (top, bottom) == (H0, H0):
        assert not np.array_equal(want, R.resize(clips, S0, S0))


def test_two_clips_with_different_modes_and_virtual_heights(K, FR, clips):
    x = torch.from_numpy(clips).cuda()
    for plan in ([pad_of("reflect", 20, 3), pad_of("color", 0, 40)], [pad_of(None, 0, 0), pad_of("replicate", 45, 1)],
                 [pad_of("black", 7, 7), pad_of("reflect", 7, 7)]):
        want = np.stack([R.pad_resize(clips[b], plan[b], S0) for b in range(2)])
        assert np.array_equal(FR.PadWideClips(S0)(x, plan=plan).cpu().numpy(), want)
        f32 = FR.PadWideClips(S0)(x, plan=plan, mean=MEAN, std=STD)
        assert same_bits(f32, K.frames_to_clip(torch.from_numpy(want).cuda(), MEAN, STD))
    # the rows of the table name the clips out of order
    plan = [pad_of("reflect", 20, 3), pad_of("color", 0, 40)]
    want = np.stack([R.pad_resize(clips[b], plan[b], S0) for b in range(2)])
    code = {"reflect": 2, "color": 1}
    rows = [(b, code[plan[b][0]], plan[b][1], plan[b][2], plan[b][3], plan[b][4], v) for b, v in ((1, 0), (0, 1))]
    vsets = [(hv, *FR.cubic_coeffs(hv, S0)) for hv in (H0 + 40, H0 + 23)]
    table = K.frame_resize_table(rows, (W0, *FR.cubic_coeffs(W0, S0)), vsets, 2, H0, W0, S0, S0)
    got = K.frame_resize(x, table.cuda(), 2, S0, S0)
    assert np.array_equal(got.cpu().numpy(), want)


def test_pad_wide_clips_draws_and_carries_out(FR):
    x = np.concatenate([six(18, 32), six(18, 32)[::-1]]).reshape(12, 1, 18, 32, 3)
    torch.manual_seed(5)
    plan = FR.PadWideClips(16).plan(12, 18, 32)
    assert len({p.mode for p in plan}) >= 4
    torch.manual_seed(5)
    got = FR.PadWideClips(16)(torch.from_numpy(x).cuda())
    want = np.stack([R.pad_resize(x[b], tuple(plan[b]), 16) for b in range(12)])
    assert np.array_equal(got.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ 3. writing into a slot of a larger buffer
def test_out_slot_leaves_its_neighbours_untouched(FR):
    src, dst = (70, 90), (33, 35)                                                  # a slot of 3465 bytes: slot 2 starts at an even, slot 1 at an odd address
    im = six(*src)
    for slot in (1, 2):
        buf = torch.full((5, *dst, 3), 0xA5, dtype=torch.uint8, device="cuda")
        out = FR.resize_frames(torch.from_numpy(im[:1]).cuda(), dst, out=buf[slot:slot + 1])
        assert out.data_ptr() == buf[slot].data_ptr()
        got = buf.cpu().numpy()
        assert np.array_equal(got[slot], R.resize(im[:1], *dst)[0])
        assert (np.delete(got, slot, axis=0) == 0xA5).all()


# ------------------------------------------------------------------------------------------------ 4. guard bands
@pytest.fixture(scope="module")
def arena():
    return GuardedArena(16 << 20, "cuda")


@pytest.mark.parametrize("poison", POISON_MODES)
@pytest.mark.parametrize("src,dst", [((70, 90), (33, 35)), ((1, 5), (4, 4))], ids=["70x90-33x35", "1x5-4x4"])
def test_guard_bands(K, FR, arena, src, dst, poison):
    """frames, table and output each between two poisoned bands of one allocation, unpadded and under a reflect pad of the full
    height (the row map at both ends of the virtual source); guard words of the table are zeros (rows of sample 0, mode none)"""
    H, W = src
    frames = six(H, W).reshape(2, 3, H, W, 3)
    zeros = torch.zeros(8, dtype=torch.int32)
    for pads in ([FR.NO_PAD, FR.NO_PAD], [FR.Pad("reflect", H, H, 0.6, (0, 0, 0)), FR.Pad("color", 0, H, 0.0, (9, 8, 7))]):
        table, nv = FR.pad_table(pads, 2, H, W, *dst)
        want = np.stack([R.resize(R.pad_frames(frames[b], *pads[b]), *dst) for b in range(2)])
        for f32 in (False, True):
            arena.reset(poison)
            x = arena.place(torch.from_numpy(frames), name="frames")
            t = arena.place(table, guard_pattern=(zeros, zeros), name="table")
            with arena.route(K):
                out = K.frame_resize(x, t, nv, *dst, *((MEAN, STD) if f32 else (None, None)))
            assert arena.contains(out) and arena.placement_of(out).role == "output"
            arena.verify()
            if f32:                                                                # (every output element was born NaN: an unwritten one differs)
                assert same_bits(out, K.frames_to_clip(torch.from_numpy(want).cuda(), MEAN, STD))
            else:                                                                  # (born 0x7F)
                assert np.array_equal(out.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ 5. the public paths, end to end
def tiny_model():
    import simple_tad_amd as TAD
    torch.manual_seed(0)
    return TAD.VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True, all_frames=4,
                                 tubelet_size=2, num_classes=2, init_scale=1.0).cuda()


def raw_video(n, H=45, W=80):
    rng = np.random.RandomState(77)
    base = six(H, W)
    return np.stack([np.roll(base[i % 6], i, axis=1) ^ rng.randint(0, 8, (H, W, 3)).astype(np.uint8) for i in range(n)])


@pytest.fixture(scope="module")
def video():
    raw = raw_video(70)
    return raw, R.resize(raw, 32, 32)                                              # the recipe's frames, computed once


def test_append_resized_across_a_chunk_boundary(video):
    from simple_tad_amd import FrameStore
    raw, small = video
    m = tiny_model().eval()
    a, b = FrameStore(72, 32, 32, "cuda"), FrameStore(72, 32, 32, "cuda")
    assert FrameStore.RESIZE_CHUNK == 64 < len(raw)
    assert a.append_resized(raw) == range(0, 70) and b.append(small) == range(0, 70)
    assert a.bytes_uploaded == 70 * 45 * 80 * 3 and len(a) == 70
    assert torch.equal(a.frames, b.frames)
    assert a.append_resized(torch.from_numpy(raw[:2]).cuda()) == range(70, 72)     # frames that are on the device already
    assert torch.equal(a.frames[70:72], b.frames[:2]) and a.bytes_uploaded == 72 * 45 * 80 * 3
    table = [[0, 1, 2, 3], [62, 63, 64, 65], [66, 67, 68, 69], [63, 64, 64, 69]]   # windows on both sides of and across the boundary
    m.patch_embed.set_input_normalization(MEAN, STD)
    with torch.no_grad():
        assert torch.equal(m(a.windows(table)), m(b.windows(table)))
    from simple_tad_amd._lib import TadError
    with pytest.raises(TadError, match="full"):
        a.append_resized(raw[:1])
    from simple_tad_amd import StoreViews
    sv = StoreViews(FrameStore(8, 32, 32, "cuda"))
    assert sv.add_video("v", raw[:5], [f"{i}.jpg" for i in range(5)], [0] * 5, np.zeros(5, np.float32), resize=True) == range(0, 5)
    assert torch.equal(sv.store.frames[:5], b.frames[:5])


@pytest.mark.parametrize("bgr", [False, True])
def test_score_video_resize(video, bgr):
    from simple_tad_amd.inference import score_video
    raw, small = video
    m = tiny_model().eval()
    got = score_video(m, raw[:9], orig_fps=10, target_fps=10, batch_size=4, mean=MEAN, std=STD, bgr=bgr, resize=True)
    want = score_video(m, small[:9], orig_fps=10, target_fps=10, batch_size=4, mean=MEAN, std=STD, bgr=bgr)
    assert got["frame"].tolist() == want["frame"].tolist() == [3, 4, 5, 6, 7, 8]
    assert torch.equal(got["logits"], want["logits"]) and torch.equal(got["prob"], want["prob"])
    assert got["bytes_uploaded"] == 9 * 45 * 80 * 3 and want["bytes_uploaded"] == 9 * 32 * 32 * 3


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_push_raw_past_one_wrap_of_the_ring(video, use_graph):
    from simple_tad_amd.inference import SlidingWindow
    raw, small = video
    m = tiny_model().eval()
    a, b = SlidingWindow(m, MEAN, STD, bgr=True, use_graph=use_graph), SlidingWindow(m, MEAN, STD, bgr=True)
    outs = 0
    for i in range(10):                                                            # a ring of 4 slots: two and a half laps
        a.push_raw(raw[i] if i % 2 else torch.from_numpy(raw[i]))
        b.push(small[i])
        assert (a.count, a.start) == (b.count, b.start) and torch.equal(a.ring, b.ring)
        if a.full:
            assert torch.equal(a.predict(), b.predict()), i
            outs += 1
    assert outs == 7
    with pytest.raises(TypeError, match="uint8 image"):
        a.push_raw(raw[:2])
