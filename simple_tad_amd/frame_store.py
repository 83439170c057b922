"""A device-resident frame store and windows into it: a video is uploaded ONCE, its windows are a table of slots.

At test time the reference decodes, resizes and uploads all T frames of every window again (dota.py:274-284 ``load_images``): at
``view_step=1`` every frame travels T times.  Here ``FrameStore`` keeps the uint8 frames ``[capacity,H,W,3]`` in HBM (150 KB per
224 x 224 frame), ``store.windows(idx)`` turns a host table ``[B,T]`` of slots into a ``FrameWindows``, and the model's patch embedding
builds its patch matrix straight from the store (``ops.PatchEmbedWindowsFn`` -> tad_im2col_frame_windows): no ``[B,T,H,W,3]`` clips in
memory, and results bit-identical to running the model on ``store[idx]``.

``store.append_resized`` takes the frames as decoded, of any size, and resizes them on the device (the loader's cv2 INTER_CUBIC resize:
``frame_resize``), so the host never shrinks a frame.

``StoreViews`` stands in for the reference datasets' test mode (``_prepare_views`` + ``__getitem__`` + the default collate): videos with
their per-frame labels go in, reference-shaped batches ``(FrameWindows, labels, ids, extra_info)`` come out -- what
``engine.final_test`` and ``engine.validation_one_epoch`` iterate over.

The index table is validated HERE, on the host, before anything reaches the device: the kernel cannot check it.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ._lib import TadError
from .sequencing import BasicLabeledSequencer_Abs


def _same_device(a: torch.device, b) -> bool:
    b = torch.device(b)
    if a.type != b.type:
        return False
    return a.index == b.index or a.index is None or b.index is None


class FrameWindows:
    """B windows of T frames each over one frame store: ``store`` uint8 [F,H,W,3] and ``idx`` int32 [B,T] on the same device, every
    entry already checked against the frames the store holds.  Quacks like the uint8 clip batch ``store[idx]`` as far as the model and
    the engines ask (``shape``, ``dtype``, ``device``, ``to``); ``materialize()`` builds that batch."""

    __slots__ = ("store", "idx", "bgr")

    def __init__(self, store: torch.Tensor, idx: torch.Tensor, bgr: bool = False):
        if store.dtype != torch.uint8 or store.dim() != 4 or store.shape[-1] != 3 or not store.is_contiguous():
            raise TypeError(f"FrameWindows: store must be a contiguous uint8 [F,H,W,3] tensor, got {store.dtype} {tuple(store.shape)}")
        if idx.dtype != torch.int32 or idx.dim() != 2 or idx.device != store.device or not idx.is_contiguous():
            raise TypeError(f"FrameWindows: idx must be a contiguous int32 [B,T] tensor on {store.device}, got {idx.dtype} {tuple(idx.shape)} "
                            f"on {idx.device}")
        self.store, self.idx, self.bgr = store, idx, bool(bgr)

    @property
    def shape(self):
        return (self.idx.shape[0], self.idx.shape[1]) + tuple(self.store.shape[1:])

    @property
    def dtype(self):
        return torch.uint8

    @property
    def device(self):
        return self.store.device

    def __len__(self):
        return self.idx.shape[0]

    def materialize(self) -> torch.Tensor:
        """the clip batch [B,T,H,W,3] uint8 the windows stand for (a copy: every frame once per window that holds it)"""
        return self.store[self.idx.long()]

    def to(self, device=None, *args, **kwargs):
        """the identity on its own device (what the engines' ``batch[0].to(device, non_blocking=True)`` asks); a store does not move"""
        if device is None or _same_device(self.store.device, device):
            return self
        raise TadError(f"FrameWindows lives on {self.store.device} with its frame store and cannot move to {device}")

    def __repr__(self):
        return f"FrameWindows(shape={self.shape}, device={self.device}, bgr={self.bgr})"


class FrameStore:
    """uint8 frames [capacity,H,W,3] on ``device``, filled front to back.  ``bgr``: the frames are cv2's (BGR), as for SlidingWindow."""

    def __init__(self, capacity: int, H: int, W: int, device, bgr: bool = False):
        if int(capacity) <= 0 or int(H) <= 0 or int(W) <= 0:
            raise ValueError(f"FrameStore: capacity, H and W must be positive, got {capacity}, {H}, {W}")
        self.capacity, self.H, self.W = int(capacity), int(H), int(W)
        self.device = torch.device(device)
        self.bgr = bool(bgr)
        self.frames = torch.zeros((self.capacity, self.H, self.W, 3), dtype=torch.uint8, device=self.device)
        self.count = 0            # frames held: slots [0, count) are valid window entries
        self.bytes_uploaded = 0   # bytes that went in through append() / append_resized() since construction / clear()
        self._staging = None      # append_resized's device buffer for raw frames [RESIZE_CHUNK,h,w,3], kept between calls

    def __len__(self):
        return self.count

    def clear(self) -> None:
        self.count = 0
        self.bytes_uploaded = 0

    def append(self, frames) -> range:
        """frames: uint8 [n,H,W,3] (numpy or tensor, host or device), already at the model's input size; ONE copy into the next n
        slots.  Returns the slot range."""
        f = torch.from_numpy(np.ascontiguousarray(frames)) if isinstance(frames, np.ndarray) else frames
        if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or f.dim() != 4 or tuple(f.shape[1:]) != (self.H, self.W, 3):
            got = f"{f.dtype} {tuple(f.shape)}" if isinstance(f, torch.Tensor) else type(frames).__name__
            raise TypeError(f"Input must be uint8 frames of shape {('n', self.H, self.W, 3)}, but got {got}")
        n = int(f.shape[0])
        if self.count + n > self.capacity:
            raise TadError(f"FrameStore is full: {self.count} of {self.capacity} slots used, cannot append {n} frames")
        lo = self.count
        self.frames[lo:lo + n].copy_(f, non_blocking=True)
        self.count += n
        self.bytes_uploaded += n * self.H * self.W * 3
        return range(lo, lo + n)

    RESIZE_CHUNK = 64  # raw frames per staging copy and resize launch of append_resized (64 frames of 1280 x 720 are 177 MB)

    def append_resized(self, frames) -> range:
        """frames: uint8 [n,h,w,3] (numpy or tensor, host or device) of ANY size h x w, as decoded.  They travel to the device once, in
        chunks of at most ``RESIZE_CHUNK`` frames through a staging buffer that is kept between calls, and each chunk is resized
        (``frame_resize.resize_frames``: the loader's cv2 INTER_CUBIC resize, one launch) straight into the next slots.
        ``bytes_uploaded`` counts the raw bytes.  Never waits for the device.  Returns the slot range."""
        from .frame_resize import resize_frames
        f = torch.from_numpy(np.ascontiguousarray(frames)) if isinstance(frames, np.ndarray) else frames
        if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or f.dim() != 4 or f.shape[-1] != 3 or f.shape[1] < 1 or f.shape[2] < 1:
            got = f"{f.dtype} {tuple(f.shape)}" if isinstance(f, torch.Tensor) else type(frames).__name__
            raise TypeError(f"Input must be uint8 frames of shape {('n', 'h', 'w', 3)}, but got {got}")
        if self.device.type != "cuda":
            raise TadError("append_resized resizes on the GPU: the store must live on one (no CPU path)")
        n, h, w = int(f.shape[0]), int(f.shape[1]), int(f.shape[2])
        if self.count + n > self.capacity:
            raise TadError(f"FrameStore is full: {self.count} of {self.capacity} slots used, cannot append {n} frames")
        lo = self.count
        on_device = f.is_cuda and _same_device(self.device, f.device) and f.is_contiguous()
        if not on_device and n and (self._staging is None or tuple(self._staging.shape[1:3]) != (h, w)):
            self._staging = torch.empty((self.RESIZE_CHUNK, h, w, 3), dtype=torch.uint8, device=self.device)
        for at in range(0, n, self.RESIZE_CHUNK):
            m = min(self.RESIZE_CHUNK, n - at)
            if on_device:
                raw = f[at:at + m]
            else:
                raw = self._staging[:m]
                raw.copy_(f[at:at + m], non_blocking=True)
            resize_frames(raw, (self.H, self.W), out=self.frames[lo + at:lo + at + m])
        self.count += n
        self.bytes_uploaded += n * h * w * 3
        return range(lo, lo + n)

    def windows(self, idx) -> FrameWindows:
        """idx: [B,T] integers (list, numpy or tensor), each a slot in [0, len(store)).  The range is checked on the HOST, before the
        table is uploaded (a device tensor is read back for it): the kernel cannot refuse a bad index."""
        host = idx.detach().cpu().numpy() if isinstance(idx, torch.Tensor) else np.asarray(idx)
        if host.ndim != 2 or host.shape[0] == 0 or host.shape[1] == 0:
            raise TypeError(f"windows: idx must be a non-empty [B,T] table, got shape {tuple(host.shape)}")
        if host.dtype.kind not in "iu":
            raise TypeError(f"windows: idx must hold integers, got {host.dtype}")
        lo, hi = int(host.min()), int(host.max())
        if lo < 0 or hi >= self.count:
            raise TadError(f"windows: slot indices must lie in [0, {self.count}) (the frames this store holds), got {lo} .. {hi}")
        table = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).to(self.device)
        return FrameWindows(self.frames, table, self.bgr)


class StoreViews:
    """The reference datasets' test mode over a FrameStore: ``add_video`` uploads a video once with its per-frame annotations;
    ``batches`` cuts every video into windows with a sequencer (dota.py:204-223 ``_prepare_views``) and yields reference-shaped batches
    ``(FrameWindows, labels [B] int64, ids [B] int64, {"ttc": [B], "clip": [B names], "frame": [B names], "smoothed_labels": [B,2]})`` in
    dataset order.  Label, ttc, smoothed label and file name of a window are those of its LAST frame (``seq[-1]``; ``load_images``
    returns the last frame's name).  A video shorter than one window contributes nothing, as in the reference."""

    def __init__(self, store: FrameStore):
        self.store = store
        self.videos = []

    def add_video(self, name: str, frames, frame_names, labels, ttc, smoothed_labels=None, resize: bool = False) -> range:
        """``resize=True``: the frames are as decoded, of any size, and are resized on the device (``FrameStore.append_resized``)"""
        n = len(frame_names)
        labels = np.asarray(labels)
        ttc = np.asarray(ttc)
        if labels.shape != (n,) or ttc.shape != (n,) or len(frames) != n:
            raise ValueError(f"add_video: {n} frame names but {len(frames)} frames, labels {labels.shape}, ttc {ttc.shape}")
        if smoothed_labels is None:  # hard labels as one-hot rows, so that every batch carries the key the reference's batches carry
            smoothed = np.eye(2, dtype=np.float32)[labels.astype(np.int64)]
        else:
            smoothed = np.asarray(smoothed_labels)
            if smoothed.shape[0] != n:
                raise ValueError(f"add_video: {n} frames but smoothed_labels {smoothed.shape}")
        slots = self.store.append_resized(frames) if resize else self.store.append(frames)
        self.videos.append(dict(name=str(name), offset=slots.start, frame_names=[str(f) for f in frame_names],
                                labels=labels.astype(np.int64), ttc=ttc, smoothed=smoothed))
        return slots

    def views(self, sequencer, input_frequency: int):
        """[(video, window of frame indices inside the video)] in dataset order"""
        out = []
        labelled = isinstance(sequencer, BasicLabeledSequencer_Abs)
        for v in self.videos:
            if labelled and input_frequency % sequencer.seq_frequency == 0 and \
                    len(v["frame_names"]) < (sequencer.seq_length - 1) * (input_frequency // sequencer.seq_frequency) + 1:
                continue  # shorter than one window: the regular sequencers return None; the reference's labelled one fails on its last assertion
            arg = [bool(x) for x in v["labels"]] if labelled else len(v["frame_names"])
            seqs = sequencer.get_sequences(arg, input_frequency)
            if seqs is None:
                continue
            out.extend((v, seq) for seq in seqs)
        return out

    def batches(self, sequencer, input_frequency: int, batch_size: int = 32):
        views = self.views(sequencer, input_frequency)
        for lo in range(0, len(views), int(batch_size)):
            part = views[lo:lo + int(batch_size)]
            idx = np.asarray([[v["offset"] + i for i in seq] for v, seq in part], dtype=np.int64)
            last = [(v, seq[-1]) for v, seq in part]
            extra = {"ttc": torch.from_numpy(np.stack([v["ttc"][i] for v, i in last])),
                     "clip": [v["name"] for v, _ in last],
                     "frame": [v["frame_names"][i] for v, i in last],
                     "smoothed_labels": torch.from_numpy(np.stack([v["smoothed"][i] for v, i in last]))}
            labels = torch.from_numpy(np.asarray([v["labels"][i] for v, i in last], dtype=np.int64))
            yield self.store.windows(idx), labels, torch.arange(lo, lo + len(part)), extra
