"""The frame-store route on the GPU: tad_im2col_frame_windows against tad_im2col_tubelets_u8 on the materialised clips, the model on
``store.windows(idx)`` against the model on ``store[idx]``, ``score_video`` against ``SlidingWindow`` and against batched clips, and
``engine.final_test`` over ``StoreViews``.  Every comparison is bit for bit: both sides feed the same patch-matrix bits into the same
functions at the same batch size.  Every index table here is valid: the kernel's clamp is never exercised; refusals are the host's."""
import csv

import numpy as np
import pytest
import torch

from guarded import GuardedArena, POISON_MODES

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FMTS = {"bf16": torch.bfloat16, "f16": torch.float16}
# (patch, H, W): the 8-pixel kernel at two patch sizes, and the pairs kernel (/14: K = 1176 padded to 1216)
SHAPES = [(16, 32, 48), (8, 16, 16), (14, 28, 42)]
F, T, TUB = 9, 4, 2
# identity, the last slots (ending at F-1), one frame repeated (start-of-video padding), descending, and one sharing frames with the first
TABLE = [[0, 1, 2, 3], [5, 6, 7, 8], [0, 0, 0, 1], [8, 6, 4, 2], [2, 3, 4, 5]]


def u8(shape, seed):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def bits(t):
    return t.view(torch.int16)


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from simple_tad_amd import _lib, kernels
    _lib.load()
    return kernels


def tiny_model():
    import simple_tad_amd as TAD
    torch.manual_seed(0)
    return TAD.VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True, all_frames=4,
                                 tubelet_size=2, num_classes=2, init_scale=1.0).cuda()


# ------------------------------------------------------------------------------------------------ 1. the patch matrix
@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("patch,H,W", SHAPES)
def test_patch_matrix_equals_im2col_of_the_materialised_clips(K, patch, H, W, bgr, fmt):
    store = u8((F, H, W, 3), 100 + patch).cuda()
    idx = torch.tensor(TABLE, dtype=torch.int32).cuda()
    got = K.im2col_frame_windows(store, idx, TUB, patch, MEAN, STD, bgr=bgr, dtype=FMTS[fmt])
    want = K.im2col_tubelets_u8(store[idx.long()].contiguous(), TUB, patch, MEAN, STD, bgr=bgr, dtype=FMTS[fmt])
    assert got.dtype == want.dtype == FMTS[fmt] and got.shape == want.shape == (len(TABLE) * (T // TUB) * (H // patch) * (W // patch),
                                                                                 K.patch_embed_ldk(3, TUB, patch))
    assert torch.equal(bits(got), bits(want))
    k = 3 * TUB * patch * patch
    assert not bits(got)[:, k:].any()      # the padding columns (patch 14 only) are zero
    assert bits(got)[:, :k].any()


def test_wrapper_refuses_what_it_can_see(K):
    from simple_tad_amd._lib import TadError
    store, idx = u8((F, 32, 32, 3), 1).cuda(), torch.tensor(TABLE, dtype=torch.int32).cuda()
    for bad in (lambda: K.im2col_frame_windows(store, idx.long(), TUB, 16, MEAN, STD),
                lambda: K.im2col_frame_windows(store, idx.cpu(), TUB, 16, MEAN, STD),
                lambda: K.im2col_frame_windows(store[:, :, :, :2], idx, TUB, 16, MEAN, STD),
                lambda: K.im2col_frame_windows(store, idx, TUB, 16, MEAN, STD, dtype=torch.float32),
                lambda: K.im2col_frame_windows(store, idx, TUB, 16, MEAN, (0.0, 1.0, 1.0)),
                lambda: K.im2col_frame_windows(store, idx, 3, 16, MEAN, STD)):
        with pytest.raises(TadError):
            bad()


# ------------------------------------------------------------------------------------------------ 2. the grid-stride second trip
def test_grid_stride_second_trip(K):
    """33 * 8 * 128 * 16 = 540 672 work items against the cap of 2048 blocks * 256 threads = 524 288: the tail takes a second trip"""
    B, T8, HW, nf = 33, 8, 128, 40
    assert B * T8 * HW * (HW // 8) == 540672 > 2048 * 256
    store = u8((nf, HW, HW, 3), 7).cuda()
    idx = torch.randint(0, nf, (B, T8), generator=torch.Generator().manual_seed(8), dtype=torch.int32).cuda()
    got = K.im2col_frame_windows(store, idx, TUB, 16, MEAN, STD)
    want = K.im2col_tubelets_u8(store[idx.long()].contiguous(), TUB, 16, MEAN, STD)
    assert torch.equal(bits(got), bits(want))


# ------------------------------------------------------------------------------------------------ 3. guard bands
@pytest.fixture(scope="module")
def arena():
    return GuardedArena(32 << 20, "cuda")


@pytest.mark.parametrize("poison", POISON_MODES)
@pytest.mark.parametrize("patch,H,W", SHAPES)
def test_guard_bands(K, arena, patch, H, W, poison):
    """store, index table and patch matrix each between two guard bands of one allocation; the table touches slot 0 and slot F-1"""
    store, idx = u8((F, H, W, 3), 200 + patch), torch.tensor(TABLE, dtype=torch.int32)
    assert idx.min() == 0 and idx.max() == F - 1
    for fmt in FMTS.values():
        for bgr in (False, True):
            plain = K.im2col_frame_windows(store.cuda(), idx.cuda(), TUB, patch, MEAN, STD, bgr=bgr, dtype=fmt).clone()
            arena.reset(poison)
            s = arena.place(store, name="store")
            i = arena.place(idx, index_range=F, name="idx")
            with arena.route(K):
                cols = K.im2col_frame_windows(s, i, TUB, patch, MEAN, STD, bgr=bgr, dtype=fmt)
            assert arena.contains(cols) and arena.placement_of(cols).role == "output"
            arena.verify()
            assert torch.equal(bits(cols), bits(plain))       # (every output byte was born NaN: an unwritten element differs)


# ------------------------------------------------------------------------------------------------ 4. the model
@pytest.mark.parametrize("precision", ["fast", "half"])
@pytest.mark.parametrize("bgr", [False, True])
def test_model_on_windows_equals_model_on_clips(precision, bgr):
    from simple_tad_amd import FrameStore, TuningScope
    m = tiny_model()
    store = FrameStore(F, 32, 32, "cuda", bgr=bgr)
    store.append(u8((F, 32, 32, 3), 11))
    fw = store.windows(TABLE)
    clips = store.frames[torch.tensor(TABLE).cuda()]
    assert torch.equal(fw.materialize(), clips) and fw.shape == tuple(clips.shape)
    m.patch_embed.set_input_normalization(MEAN, STD, bgr=bgr)
    with TuningScope(precision=precision):
        m.eval()
        with torch.no_grad():
            a, b = m(fw), m(clips)
        assert a.shape == (len(TABLE), 2) and torch.equal(a, b)
        m.train()
        la = m(fw)
        la.sum().backward()
        ga = m.patch_embed.proj.weight.grad.clone()
        gh = m.head.weight.grad.clone()
        m.zero_grad()
        lb = m(clips)
        lb.sum().backward()
        assert torch.equal(la, lb) and torch.equal(ga, m.patch_embed.proj.weight.grad) and torch.equal(gh, m.head.weight.grad)
        assert ga.abs().sum() > 0


def test_precise_mode_refuses_windows():
    from simple_tad_amd import FrameStore, TuningScope
    from simple_tad_amd._lib import TadError
    m = tiny_model().eval()
    store = FrameStore(4, 32, 32, "cuda")
    store.append(u8((4, 32, 32, 3), 12))
    with TuningScope(precision="precise"):
        with pytest.raises(TadError, match="precise"), torch.no_grad():
            m(store.windows([[0, 1, 2, 3]]))


# ------------------------------------------------------------------------------------------------ 5. score_video
@pytest.mark.parametrize("bgr", [False, True])
def test_score_video(bgr):
    from simple_tad_amd import FrameStore
    from simple_tad_amd.inference import SlidingWindow, score_video
    m = tiny_model().eval()
    frames = u8((9, 32, 32, 3), 13)
    one = score_video(m, frames.numpy(), orig_fps=10, target_fps=10, batch_size=1, mean=MEAN, std=STD, bgr=bgr)
    assert one["frame"].dtype == torch.int64 and one["frame"].tolist() == [3, 4, 5, 6, 7, 8]
    assert one["logits"].dtype == torch.float32 and one["logits"].shape == (6, 2) and one["prob"].shape == (6,)
    assert one["bytes_uploaded"] == 9 * 32 * 32 * 3
    assert torch.equal(one["prob"], torch.softmax(one["logits"].cuda(), dim=1)[:, 1].cpu())
    sw = SlidingWindow(m, MEAN, STD, bgr=bgr)
    outs = []
    for f in frames:
        sw.push(f.numpy())
        if sw.full:
            outs.append(sw.predict())
    assert torch.equal(one["logits"], torch.cat(outs).cpu())
    # batches of 4 with a ragged last batch of 2: equal to the model on the materialised clips, batch by batch
    four = score_video(m, frames, orig_fps=10, target_fps=10, batch_size=4, mean=MEAN, std=STD, bgr=bgr)
    store = FrameStore(9, 32, 32, "cuda", bgr=bgr)
    store.append(frames)
    assert store.bytes_uploaded == 9 * 32 * 32 * 3 == four["bytes_uploaded"]
    table = torch.tensor([[s, s + 1, s + 2, s + 3] for s in range(6)]).cuda()
    with torch.no_grad():
        want = torch.cat([m(store.frames[table[:4]]), m(store.frames[table[4:]])])
    assert torch.equal(four["logits"], want.cpu()) and four["frame"].tolist() == [3, 4, 5, 6, 7, 8]
    assert not m.training
    # a video shorter than one window, and a sequencer of the caller's (stride 2: windows end on 6 and 8)
    short = score_video(m, frames[:3], orig_fps=10, target_fps=10)
    assert short["frame"].shape == (0,) and short["frame"].dtype == torch.int64 and short["logits"].shape == (0, 2) and short["prob"].shape == (0,)
    from simple_tad_amd.sequencing import RegularSequencer
    two = score_video(m, frames, orig_fps=20, target_fps=10, sequencer=RegularSequencer(10, 4, 2), mean=MEAN, std=STD, bgr=bgr)
    assert two["frame"].tolist() == [6, 8]
    with torch.no_grad():
        assert torch.equal(two["logits"], m(store.frames[torch.tensor([[0, 2, 4, 6], [2, 4, 6, 8]]).cuda()]).cpu())


# ------------------------------------------------------------------------------------------------ 6. host refusals on the GPU build
def test_host_refusals_come_before_any_launch():
    from simple_tad_amd import FrameStore
    from simple_tad_amd._lib import TadError
    store = FrameStore(F + 1, 32, 32, "cuda")
    store.append(u8((F, 32, 32, 3), 14))
    with pytest.raises(TadError, match="slot indices"):
        store.windows([[0, 1, 2, F]])          # slot F exists in the allocation but holds no frame
    with pytest.raises(TadError, match="slot indices"):
        store.windows([[0, 1, -1, 3]])
    with pytest.raises(TadError, match="slot indices"):
        store.windows(torch.tensor([[0, 1, 2, F + 5]]).cuda())
    with pytest.raises(TadError, match="full"):
        store.append(u8((2, 32, 32, 3), 15))
    with pytest.raises(TypeError):
        store.append(u8((1, 16, 32, 3), 16))
    with pytest.raises(TypeError):
        store.append(u8((1, 32, 32, 3), 17).float())
    assert len(store) == F and store.bytes_uploaded == F * 32 * 32 * 3
    fw = store.windows(TABLE)
    assert fw.to("cuda") is fw and fw.to(torch.device("cuda", 0), non_blocking=True) is fw
    with pytest.raises(TadError):
        fw.to("cpu")


# ------------------------------------------------------------------------------------------------ 7. final_test
def test_final_test_over_store_views(tmp_path):
    from simple_tad_amd import FrameStore, StoreViews
    from simple_tad_amd import engine as E, metrics as M
    from simple_tad_amd.sequencing import RegularSequencer
    m = tiny_model()
    sv = StoreViews(FrameStore(16, 32, 32, "cuda"))
    la, lb = [0, 0, 0, 0, 1, 1, 1, 0, 0], [0, 0, 0, 1, 1, 0, 0]
    ta, tb = np.arange(9, dtype=np.float32) * 0.25 - 1.0, np.arange(7, dtype=np.float32) + 0.125
    sv.add_video("vid_a", u8((9, 32, 32, 3), 21), [f"a/{i:04d}.jpg" for i in range(9)], la, ta)
    sv.add_video("vid_b", u8((7, 32, 32, 3), 22).numpy(), [f"b/{i:04d}.jpg" for i in range(7)], lb, tb)
    seq = RegularSequencer(10, 4, 1)
    preds_file, stats_file = tmp_path / "predictions.csv", tmp_path / "stats.txt"
    with pytest.warns(UserWarning, match="plot"):
        res = E.final_test(sv.batches(seq, 10, batch_size=4), m, torch.device("cuda"), preds_file, stats_file, plot_dir=str(tmp_path / "plots"))
    assert not (tmp_path / "plots").exists() and not m.training
    # the model's own logits, batch by batch at the same batch size
    with torch.no_grad():
        logits = torch.cat([m(b[0]) for b in sv.batches(seq, 10, batch_size=4)]).float().cpu()
    n = 6 + 4
    assert logits.shape == (n, 2)
    rows = list(csv.reader(open(preds_file, newline="")))
    assert rows[0] == ["", "clip", "filename", "logits_safe", "logits_risk", "label", "ttc"] and len(rows) == n + 1
    body = rows[1:]
    assert [int(r[0]) for r in body] == list(range(n))
    assert [r[1] for r in body] == ["vid_a"] * 6 + ["vid_b"] * 4
    assert [r[2] for r in body] == [f"a/{i:04d}.jpg" for i in range(3, 9)] + [f"b/{i:04d}.jpg" for i in range(3, 7)]
    parsed = torch.tensor([[float(r[3]), float(r[4])] for r in body], dtype=torch.float64).to(torch.float32)
    assert torch.equal(parsed, logits)
    labels = la[3:] + lb[3:]
    assert [int(r[5]) for r in body] == labels and 0 < sum(labels) < n
    assert [float(r[6]) for r in body] == ta[3:].tolist() + tb[3:].tolist()
    acc, recall, precision, f1, confmat, auroc, ap, _, _, _ = M.calculate_metrics(logits.cuda(), torch.tensor(labels).cuda())
    text = open(stats_file).read().split("\n")
    assert text[0] == "" and text[1].startswith("====") and text[-2].startswith("----") and len(text) == 9
    assert text[2] == f"mAP: {ap}, auroc: {auroc}, acc: {acc}"
    assert text[3] == f"P@0.5: {precision}, R@0.5: {recall}, F1@0.5: {f1}"
    assert [text[5].strip(), text[6].strip()] == [f"{confmat[0][0]} | {confmat[0][1]}", f"{confmat[1][0]} | {confmat[1][1]}"]
    hard = logits.argmax(1)
    assert res["acc1"] == 100.0 * int((hard == torch.tensor(labels)).sum()) / n
    losses = [torch.nn.functional.cross_entropy(logits[lo:lo + 4].cuda(), torch.tensor(labels[lo:lo + 4]).cuda()).item() for lo in (0, 4, 8)]
    assert res["loss"] == (losses[0] + losses[1] + losses[2]) / 3
