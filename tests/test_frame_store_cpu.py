"""Host side of the frame-store route, no GPU: the argument checks of tad_im2col_frame_windows (they run before any launch), the
FrameStore / FrameWindows / StoreViews bookkeeping on a CPU-resident store, and final_test's shard merge and CSV writer."""
import csv
import ctypes

import numpy as np
import pytest
import torch

from simple_tad_amd import _lib
from simple_tad_amd import engine as E
from simple_tad_amd.frame_store import FrameStore, FrameWindows, StoreViews
from simple_tad_amd.sequencing import RegularSequencer, UnsafeOverlapSequencer


@pytest.fixture(scope="module")
def lib():
    from simple_tad_amd import build
    build.build(verbose=False)
    return _lib.load()


def test_entry_point_refuses_bad_arguments(lib):
    """every refusal returns TAD_EINVAL (-1) with a message; nothing is launched (the pointers are host memory)"""
    buf = ctypes.create_string_buffer(256)
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p((base + 15) & ~15)          # 16-byte aligned
    mean = (ctypes.c_float * 3)(0.485, 0.456, 0.406)
    std = (ctypes.c_float * 3)(0.229, 0.224, 0.225)
    fn = lib.tad_im2col_frame_windows

    def refused(*args, msg):
        assert fn(*args) == -1
        assert msg in lib.tad_last_error_string(), lib.tad_last_error_string()

    ok = dict(store=p, F=9, idx=p, cols=p, dt=_lib.TAD_BF16, B=2, T=4, H=32, W=32, tub=2, patch=16, mean=mean, std=std)

    def call(msg, **kw):
        a = dict(ok, **kw)
        refused(a["store"], a["F"], a["idx"], a["cols"], a["dt"], a["B"], a["T"], a["H"], a["W"], a["tub"], a["patch"], a["mean"], a["std"], 0,
                None, msg=msg)

    for name in ("store", "idx", "cols", "mean", "std"):
        call(b"null", **{name: None})
    call(b"F=0", F=0)
    call(b"F=-3", F=-3)
    call(b"cols_dtype=0", dt=_lib.TAD_F32)
    call(b"cols_dtype=3", dt=3)
    call(b"even", patch=7, H=28, W=28)
    call(b"multiples", T=3)                          # T % tubelet
    call(b"multiples", H=40)                         # H % patch
    call(b"multiples", B=0)
    call(b"zero std", std=(ctypes.c_float * 3)(0.229, 0.0, 0.225))
    call(b"misaligned", cols=ctypes.c_void_p(p.value + 8))
    call(b"misaligned", store=ctypes.c_void_p(p.value + 2))
    call(b"misaligned", idx=ctypes.c_void_p(p.value + 1))


def test_one_symbol_no_twin():
    assert "tad_im2col_frame_windows" in _lib.SIGNATURES
    assert not any("frame_windows" in k or "frame_windows" in v for k, v in _lib.F16_TWINS.items())


def frames_of(n, H=8, W=8, seed=0):
    return torch.randint(0, 256, (n, H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def test_frame_store_bookkeeping_and_refusals():
    st = FrameStore(6, 8, 8, "cpu", bgr=True)
    f = frames_of(5)
    assert st.append(f[:2]) == range(0, 2) and st.append(f[2:5].numpy()) == range(2, 5)
    assert len(st) == 5 and st.bytes_uploaded == 5 * 8 * 8 * 3 and torch.equal(st.frames[:5], f)
    with pytest.raises(_lib.TadError, match="full"):
        st.append(f[:2])
    assert len(st) == 5
    for bad in (f[:1].float(), f[0], frames_of(1, 8, 16), np.zeros((1, 8, 8, 3), dtype=np.int16), [[1]]):
        with pytest.raises(TypeError):
            st.append(bad)
    fw = st.windows([[0, 1, 2, 3], [4, 4, 3, 0]])
    assert isinstance(fw, FrameWindows) and fw.shape == (2, 4, 8, 8, 3) and fw.dtype == torch.uint8 and fw.device == st.frames.device
    assert fw.bgr is True and fw.idx.dtype == torch.int32 and len(fw) == 2
    assert fw.to("cpu") is fw and fw.to(torch.device("cpu"), non_blocking=True) is fw
    with pytest.raises(_lib.TadError):
        fw.to("cuda")
    assert torch.equal(fw.materialize(), f[torch.tensor([[0, 1, 2, 3], [4, 4, 3, 0]])])
    assert torch.equal(st.windows(np.array([[1, 2]], dtype=np.int16)).idx, st.windows(torch.tensor([[1, 2]])).idx)
    # the range is that of the frames HELD (slot 5 exists but is empty), checked before anything is uploaded
    for bad in ([[0, 1, 2, 5]], [[0, -1, 2, 3]], torch.tensor([[0, 6]])):
        with pytest.raises(_lib.TadError, match="slot indices"):
            st.windows(bad)
    for bad in ([0, 1, 2], [[0.0, 1.0]], np.zeros((0, 4), dtype=np.int64), [[[0]]]):
        with pytest.raises(TypeError):
            st.windows(bad)
    st.clear()
    assert len(st) == 0 and st.bytes_uploaded == 0
    with pytest.raises(_lib.TadError):
        st.windows([[0]])
    with pytest.raises(ValueError):
        FrameStore(0, 8, 8, "cpu")


def two_videos():
    """video a: 7 frames, anomaly on frames 4..5; video b: 3 frames (shorter than one window of 4); video c: 6 frames"""
    st = FrameStore(16, 8, 8, "cpu")
    sv = StoreViews(st)
    fa, fb, fc = frames_of(7, seed=1), frames_of(3, seed=2), frames_of(6, seed=3)
    la = [0, 0, 0, 0, 1, 1, 0]
    lc = [0, 0, 0, 1, 1, 1]
    sv.add_video("a", fa, [f"a_{i:03d}.jpg" for i in range(7)], la, np.arange(7, dtype=np.float32) * 0.5 - 2.0)
    sv.add_video("b", fb, [f"b_{i:03d}.jpg" for i in range(3)], [0, 0, 0], np.zeros(3, dtype=np.float32))
    sv.add_video("c", fc, [f"c_{i:03d}.jpg" for i in range(6)], lc, np.arange(6, dtype=np.float32) + 10.0,
                 smoothed_labels=np.stack([1 - np.linspace(0, 1, 6), np.linspace(0, 1, 6)], 1).astype(np.float32))
    return sv, (fa, fb, fc), (la, lc)


def test_store_views_batches_are_reference_shaped():
    sv, (fa, fb, fc), (la, lc) = two_videos()
    assert sv.store.bytes_uploaded == 16 * 8 * 8 * 3
    batches = list(sv.batches(RegularSequencer(10, 4, 1), 10, batch_size=3))
    # a: windows ending on 3..6 (4 of them), b: none, c: windows ending on 3..5 (3 of them) -> 7 windows: 3 + 3 + 1
    assert [len(b[0]) for b in batches] == [3, 3, 1]
    clips = sum((b[3]["clip"] for b in batches), [])
    files = sum((b[3]["frame"] for b in batches), [])
    assert clips == ["a"] * 4 + ["c"] * 3
    assert files == ["a_003.jpg", "a_004.jpg", "a_005.jpg", "a_006.jpg", "c_003.jpg", "c_004.jpg", "c_005.jpg"]
    labels = torch.cat([b[1] for b in batches])
    assert labels.dtype == torch.int64 and labels.tolist() == [0, 1, 1, 0, 1, 1, 1]
    assert torch.cat([b[2] for b in batches]).tolist() == list(range(7))
    assert torch.cat([b[3]["ttc"] for b in batches]).tolist() == [-0.5, 0.0, 0.5, 1.0, 13.0, 14.0, 15.0]
    sm = torch.cat([b[3]["smoothed_labels"] for b in batches])
    assert sm.shape == (7, 2) and sm[:4].tolist() == [[1, 0], [0, 1], [0, 1], [1, 0]] and torch.allclose(sm[4:, 1], torch.tensor([0.6, 0.8, 1.0]))
    # the windows themselves: video c starts at slot 10 (7 + 3)
    got = torch.cat([b[0].materialize() for b in batches])
    assert torch.equal(got[0], fa[0:4]) and torch.equal(got[3], fa[3:7]) and torch.equal(got[4], fc[0:4]) and torch.equal(got[6], fc[2:6])
    assert batches[1][0].idx.tolist() == [[3, 4, 5, 6], [10, 11, 12, 13], [11, 12, 13, 14]]
    # a labelled sequencer is given the labels (the 3-frame video is skipped: shorter than one window)
    n = sum(len(b[0]) for b in sv.batches(UnsafeOverlapSequencer(10, 4, 3), 10, batch_size=32))
    ref = sum(len(UnsafeOverlapSequencer(10, 4, 3).get_sequences([bool(x) for x in lab], 10)) for lab in (la, lc))
    assert n == ref
    with pytest.raises(ValueError):
        sv.add_video("d", fb, ["x"], [0, 0, 0], [0.0, 0.0, 0.0])


def test_merge_of_two_ranks_and_csv_round_trip(tmp_path):
    g = torch.Generator().manual_seed(5)
    l0, l1 = torch.randn(3, 2, generator=g), torch.randn(2, 2, generator=g) * 1e-3
    shards = [(["a", "a", "b"], ["a_1.jpg", "a_2.jpg", "b_9.jpg"]), (["c", "c"], ["c_4.jpg", "c,5.jpg"])]
    logits, labels = torch.cat([l0, l1]), torch.tensor([0, 1, 0, 1, 1])
    ttc = torch.tensor([-1.0, 0.5, 2.25, float("inf"), 0.1], dtype=torch.float64)
    t = E.merge_prediction_shards(shards, logits, labels, ttc)
    assert tuple(t) == E.PREDICTION_COLUMNS
    assert t["clip"] == ["a", "a", "b", "c", "c"] and t["filename"][3:] == ["c_4.jpg", "c,5.jpg"]
    assert t["logits_safe"].dtype == np.float32 and np.array_equal(t["logits_risk"], logits[:, 1].numpy()) and t["label"].tolist() == [0, 1, 0, 1, 1]
    path = tmp_path / "predictions.csv"
    E.write_predictions_csv(path, t)
    rows = list(csv.reader(open(path, newline="")))
    assert rows[0] == ["", "clip", "filename", "logits_safe", "logits_risk", "label", "ttc"] and len(rows) == 6
    assert [r[0] for r in rows[1:]] == ["0", "1", "2", "3", "4"] and rows[5][2] == "c,5.jpg"
    back = np.array([[float(r[3]), float(r[4])] for r in rows[1:]]).astype(np.float32)
    assert np.array_equal(back, logits.numpy())                      # the float32 logits come back bit for bit
    assert [float(r[6]) for r in rows[1:]] == ttc.tolist() and [int(r[5]) for r in rows[1:]] == [0, 1, 0, 1, 1]
    with pytest.raises(ValueError):
        E.merge_prediction_shards(shards, logits[:4], labels, ttc)
    with pytest.raises(ValueError):
        E.merge_prediction_shards([(["a"], [])], logits[:1], labels[:1], ttc[:1])


def test_score_video_and_patch_embed_refuse_the_cpu():
    """no CPU path: a model on the CPU is refused before anything is computed"""
    import simple_tad_amd as T
    from simple_tad_amd.inference import score_video
    m = T.VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=1, num_heads=2, all_frames=4, tubelet_size=2, num_classes=2)
    with pytest.raises(_lib.TadError, match="GPU"):
        score_video(m, np.zeros((9, 32, 32, 3), dtype=np.uint8), orig_fps=10, target_fps=10)
    st = FrameStore(4, 32, 32, "cpu")
    st.append(np.zeros((4, 32, 32, 3), dtype=np.uint8))
    with pytest.raises(_lib.TadError):
        m(st.windows([[0, 1, 2, 3]]))
