"""Many live cameras scored together: S sliding windows in one frame store, fed by one ragged ingest launch per tick.

``inference.SlidingWindow`` serves one camera: one upload, one resize launch and one batch-1 forward per frame, and T captured graphs.
A deployment watches many cameras, and they differ: they start at different times, run at different rates, drop frames, and deliver
different frame sizes.  ``StreamBank`` keeps S rings in ONE uint8 store ``[S*T, H, W, 3]`` -- stream s owns slots ``s*T .. s*T + T - 1``
-- with the per-stream ``count`` and ``start`` on the host (deterministic in the pushes: nothing is read back).  A tick is

  push_raw(ids, frames)   the K newest frames, of ANY mix of sizes, packed into one pinned buffer at 4-byte aligned offsets; ONE copy of
                          the bytes, one of the table, ONE launch (``kernels.ingest_frames``, include/tad_mi355x_bank.h) that resizes each
                          frame (the loader's cv2 INTER_CUBIC resize, ``frame_resize``'s contract bit for bit) into its stream's ring slot
  push_yuv(ids, frames)   the same for cameras that deliver 4:2:0 YUV surfaces (``YuvFrame``: NV12, NV21, I420, pitched or not): the planes
                          are packed as they come -- half the bytes of RGB, no conversion on the host -- and converted inside the
                          resize launch (``kernels.ingest_yuv``, include/tad_mi355x_yuv.h) by a colour set the host states
  predict()               the ready streams as one batch: an ``[A, T]`` table of slots in temporal order, ``model(FrameWindows(store,
                          table))`` -- the route ``score_video`` takes, so both model families are served with no family branch

where the pieces before this module needed one resize launch and one table upload per distinct size plus K scatter copies, and a
batch-1 forward per camera.  The logits of a stream are those of the model on that stream's window as a uint8 clip at the same batch
size, bit for bit.

Channel order: the store has ONE.  ``bgr`` is one bool (every camera delivers that order; the store keeps it) or one bool per stream: if
they differ the store is RGB and the frames of the BGR cameras are swapped on their way in (the row flag of the ingest table).

There is no CPU path.  The host side (``StreamRings``, ``plan_ingest``) runs without a GPU.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import TadError
from .inference import IMAGENET_MEAN, IMAGENET_STD

__all__ = ["StreamBank", "StreamRings", "plan_ingest", "YuvFrame", "plan_ingest_yuv", "colour_set", "COLOUR_SETS"]

_HEAD = 64  # slack in front of the first frame and behind the last one in the staging buffers (bytes, a multiple of 4)
_PRECISE = 'precision "precise" takes the normalised f32 clip (the uint8 input stage feeds the bf16 path)'


class StreamRings:
    """The host bookkeeping of S rings of T slots in one store: stream s owns slots s*T .. s*T + T - 1.  ``count[s]`` frames were pushed
    since the stream (re)started, ``start[s]`` is the ring slot of its oldest frame."""

    def __init__(self, streams: int, T: int):
        if int(streams) < 1 or int(T) < 1:
            raise TadError(f"StreamRings: streams={streams} and T={T} must be positive")
        self.S, self.T = int(streams), int(T)
        self.count = [0] * self.S
        self.start = [0] * self.S

    def check_ids(self, ids, who: str):
        """the ids as a list of ints: each inside [0, S), none twice"""
        out = [int(i) for i in (ids.tolist() if isinstance(ids, (np.ndarray, torch.Tensor)) else ids)]
        for s in out:
            if not 0 <= s < self.S:
                raise TadError(f"{who}: stream id {s} outside [0, {self.S})")
        if len(set(out)) != len(out):
            dup = sorted(s for s in set(out) if out.count(s) > 1)
            raise TadError(f"{who}: stream id {dup[0]} is named twice in one call")
        return out

    def assign(self, ids):
        """the store slot the next frame of each stream goes to (ids: checked), and the state after it: a ring that is not full yet fills
        front to back, a full one overwrites its oldest frame and starts one slot later"""
        slots = []
        for s in ids:
            if self.count[s] < self.T:
                ring = self.count[s]
            else:
                ring = self.start[s]
                self.start[s] = (ring + 1) % self.T
            self.count[s] += 1
            slots.append(s * self.T + ring)
        return slots

    @property
    def ready(self):
        return [s for s in range(self.S) if self.count[s] >= self.T]

    def window_table(self, ids) -> np.ndarray:
        """int32 [A, T]: the slots of each stream's window, oldest frame first"""
        T = self.T
        return np.asarray([[s * T + (self.start[s] + t) % T for t in range(T)] for s in ids], dtype=np.int32).reshape(len(ids), T)

    def reset(self, s: int) -> None:
        self.count[s] = 0
        self.start[s] = 0


def _pack(sizes):
    """frames of ``sizes`` bytes back to back at 4-byte aligned offsets behind ``_HEAD`` bytes of slack: (offsets, src_bytes)"""
    offsets, at = [], _HEAD
    for n in sizes:
        offsets.append(at)
        at += (n + 3) // 4 * 4
    return offsets, at


def _cached_plan(cache: Optional[dict], key, slots, row_words: int, slot_word: int, recheck, build):
    """What the two planners share around a table: ``build()`` makes ``(table, offsets, src_bytes, *set counts)``, the table checked.
    ``cache`` keeps the last 16 of them by ``key``; on a hit the table is the kept one with word ``slot_word`` of its rows of
    ``row_words`` words rewritten to ``slots``, and ``recheck(table, K, src_bytes, counts)`` checks it again all the same."""
    hit = cache.get(key) if cache is not None else None
    if hit is not None:
        proto, offsets, at, *counts = hit
        table = proto.clone()
        k = len(offsets)
        table[:k * row_words].view(k, row_words)[:, slot_word] = torch.as_tensor([int(v) for v in slots], dtype=torch.int32)
        recheck(table, k, at, counts)
        return (table, offsets, at, *counts)
    plan = build()
    if cache is not None:
        if len(cache) >= 16:
            cache.clear()
        cache[key] = (plan[0].clone(), *plan[1:])
    return plan


def plan_ingest(extents, slots, swaps, S_h: int, S_w: int, F: int, cache: Optional[dict] = None):
    """The table of one ingest launch: frame k is ``extents[k]`` = (h, w), goes to store slot ``slots[k]`` and has its channels 0 and 2
    swapped on the way if ``swaps[k]``.  The frames are laid out back to back at 4-byte aligned offsets behind ``_HEAD`` bytes of slack;
    there is one horizontal set per distinct w and one vertical set per distinct h.  Returns ``(table int32 CPU tensor, offsets,
    src_bytes, n_hsets, n_vsets)``; the table has passed tadb_ingest_plan_check.  ``cache``: a dict the caller keeps between ticks -- a
    fleet sends the same mix of sizes tick after tick, and then only the slot column of the table changes (it is checked again all the
    same).  Host only."""
    from . import kernels as K
    from .frame_resize import cubic_coeffs
    extents = [(int(h), int(w)) for h, w in extents]

    def recheck(table, k, at, counts):
        _lib.check_bank(_lib.load_bank().tadb_ingest_plan_check(table.data_ptr(), table.numel(), k, *counts, at, int(F), int(S_h), int(S_w)),
                        "tadb_ingest_plan_check")

    def build():
        offsets, at = _pack(h * w * 3 for h, w in extents)
        hsets, vsets = {}, {}
        rows = [(off, h, w, int(slot), hsets.setdefault(w, len(hsets)), vsets.setdefault(h, len(vsets)), _lib.BANK_SWAP_RB if swap else 0)
                for off, (h, w), slot, swap in zip(offsets, extents, slots, swaps)]
        if len(hsets) > _lib.BANK_MAX_SETS or len(vsets) > _lib.BANK_MAX_SETS:
            raise TadError(f"plan_ingest: {len(hsets)} distinct widths and {len(vsets)} distinct heights in one call, at most {_lib.BANK_MAX_SETS} each")
        table = K.ingest_table(rows, [(w, *cubic_coeffs(w, S_w)) for w in hsets], [(h, *cubic_coeffs(h, S_h)) for h in vsets], at, F, S_h, S_w)
        return table, offsets, at, len(hsets), len(vsets)

    key = (tuple(extents), tuple(bool(b) for b in swaps), int(S_h), int(S_w))
    return _cached_plan(cache, key, slots, _lib.BANK_ROW_WORDS, 3, recheck, build)


# ---------------------------------------------------------------------------------------------------------------- 4:2:0 YUV frames
# The colour sets {y_off, cy, cvr, cug, cvg, cub} of include/tad_mi355x_yuv.h, 20-bit fixed point.  The kernel knows no colour standard:
# these integers are what the host states.  "bt601" is the set OpenCV's 8-bit YUV420 -> RGB conversion documents, taken literally (it is
# rounded from the three-digit matrix 1.164, 1.596, 0.391, 0.813, 2.018, so it is NOT what the derivation below gives for BT.601's luma
# weights: (16, 1220945, 1673555, -410793, -852458, 2115221)); the other three come from the derivation.
_KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
_OPENCV_BT601 = (16, 1220542, 1673527, -409993, -852492, 2116026)


def derive_colour_set(kr: float, kb: float, full_range: bool):
    """The usual Y'CbCr -> R'G'B' matrix of the luma weights (kr, kb) in fp64, times 2^20, rounded to nearest: R = Y + 2 (1 - kr) V',
    B = Y + 2 (1 - kb) U', G = Y - (2 kb (1 - kb) / kg) U' - (2 kr (1 - kr) / kg) V' with kg = 1 - kr - kb.  Limited range scales luma
    by 255 / 219 behind an offset of 16 and chroma by 255 / 224; full range by 1 behind no offset."""
    kg = 1.0 - kr - kb
    ys, cs = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    q = lambda v: int(np.rint(np.float64(v) * (1 << 20)))
    return (0 if full_range else 16, q(ys), q(2.0 * (1.0 - kr) * cs), q(-2.0 * kb * (1.0 - kb) / kg * cs), q(-2.0 * kr * (1.0 - kr) / kg * cs),
            q(2.0 * (1.0 - kb) * cs))


COLOUR_SETS = {"bt601": _OPENCV_BT601,
               "bt709": derive_colour_set(*_KR_KB["bt709"], False),
               "bt601-full": derive_colour_set(*_KR_KB["bt601"], True),
               "bt709-full": derive_colour_set(*_KR_KB["bt709"], True)}


def colour_set_bound(cset) -> int:
    """the largest magnitude an int32 sum of the conversion can reach under this set: it must stay below 2^31"""
    _, cy, cvr, cug, cvg, cub = (int(v) for v in cset)
    return 255 * cy + 128 * max(abs(cvr), abs(cub), abs(cug) + abs(cvg)) + (1 << 19)


def colour_set(matrix):
    """the six integers of a colour set: a name of COLOUR_SETS, or six integers of the caller's own (checked against the int32 bound)"""
    if isinstance(matrix, str):
        if matrix not in COLOUR_SETS:
            raise TadError(f"colour_set: unknown matrix {matrix!r}: one of {sorted(COLOUR_SETS)} or six integers")
        return COLOUR_SETS[matrix]
    c = tuple(int(v) for v in matrix)
    if len(c) != 6:
        raise TadError(f"colour_set: a set is six integers (y_off, cy, cvr, cug, cvg, cub), got {len(c)}")
    if not 0 <= c[0] <= 255 or c[1] < 0 or colour_set_bound(c) >= 1 << 31:
        raise TadError(f"colour_set: {c}: y_off must be in [0, 255], cy non-negative and 255 * cy + 128 * max|c| + 2^19 = {colour_set_bound(c)} below 2^31")
    return c


_FORMATS = ("nv12", "nv21", "i420")


class YuvFrame:
    """One 4:2:0 YUV frame as a camera or a decoder hands it over: ``data`` a uint8 array (numpy or a CPU tensor) of any shape whose
    bytes, in order, are the surface -- ``h`` luma rows of ``y_pitch`` bytes (default ``w``), then the chroma: for "nv12" / "nv21"
    ``(h + 1) // 2`` rows of ``c_pitch`` bytes (default ``2 * ((w + 1) // 2)``) of interleaved U V / V U pairs, for "i420" the U plane
    and then the V plane, each ``(h + 1) // 2`` rows of ``c_pitch`` bytes (default ``(w + 1) // 2``).  The last row of the last plane may
    stop at its last live byte.  ``matrix``: a name of ``COLOUR_SETS`` or six integers.  Nothing is copied or converted here."""

    def __init__(self, data, h: int, w: int, format: str = "nv12", y_pitch: Optional[int] = None, c_pitch: Optional[int] = None, matrix="bt601"):
        t = torch.from_numpy(np.ascontiguousarray(data)) if isinstance(data, np.ndarray) else data
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.is_cuda:
            got = f"{t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(data).__name__
            raise TypeError(f"YuvFrame: data must be a uint8 numpy array or CPU tensor, but got {got}")
        if format not in _FORMATS:
            raise TadError(f"YuvFrame: format {format!r} must be one of {_FORMATS}")
        h, w = int(h), int(w)
        if not (1 <= h <= _lib.YUV_MAX_EXTENT and 1 <= w <= _lib.YUV_MAX_EXTENT):
            raise TadError(f"YuvFrame: a frame of {h} x {w} pixels must have 1 .. {_lib.YUV_MAX_EXTENT} per side")
        ch, cw = (h + 1) // 2, (w + 1) // 2
        step = 1 if format == "i420" else 2
        y_pitch = w if y_pitch is None else int(y_pitch)
        c_pitch = cw * step if c_pitch is None else int(c_pitch)
        if y_pitch < w:
            raise TadError(f"YuvFrame: y_pitch={y_pitch} is below the {w} bytes of a luma row")
        if c_pitch < cw * step:
            raise TadError(f"YuvFrame: c_pitch={c_pitch} is below the {cw * step} bytes of a {format} chroma row")
        self.data = t.contiguous().reshape(-1)
        self.h, self.w, self.format, self.y_pitch, self.c_pitch, self.c_step = h, w, format, y_pitch, c_pitch, step
        self.cset = colour_set(matrix)
        c_at = h * y_pitch
        if format == "i420":
            self.u_at, self.v_at = c_at, c_at + ch * c_pitch
            self.nbytes = self.v_at + (ch - 1) * c_pitch + cw
        else:
            self.u_at, self.v_at = (c_at, c_at + 1) if format == "nv12" else (c_at + 1, c_at)
            self.nbytes = c_at + (ch - 1) * c_pitch + 2 * cw
        if self.data.numel() < self.nbytes:
            raise TadError(f"YuvFrame: {self.data.numel()} bytes do not hold a {format} frame of {h} x {w} with y_pitch={y_pitch}, c_pitch={c_pitch} "
                           f"({self.nbytes} bytes)")

    @property
    def layout(self):
        """what a table is planned from (the bytes themselves are not part of it)"""
        return (self.h, self.w, self.y_pitch, self.u_at, self.v_at, self.c_pitch, self.c_step, self.nbytes, self.cset)

    @classmethod
    def of(cls, f, k: int = 0):
        """a YuvFrame as it is; a bare uint8 [h * 3 / 2, w] array (even h and w) as a contiguous NV12 frame, BT.601 limited range"""
        if isinstance(f, cls):
            return f
        t = torch.from_numpy(np.ascontiguousarray(f)) if isinstance(f, np.ndarray) else f
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 2 or t.shape[0] < 3 or t.shape[0] % 3 or t.shape[1] % 2 or t.shape[1] < 2:
            got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(f).__name__
            raise TypeError(f"Input {k} must be a YuvFrame or a uint8 array of shape {('h * 3 / 2', 'w')} with even h and w, but got {got}")
        return cls(t, t.shape[0] // 3 * 2, t.shape[1])


def plan_ingest_yuv(layouts, slots, bgrs, S_h: int, S_w: int, F: int, cache: Optional[dict] = None):
    """The table of one YUV ingest launch: frame k is ``layouts[k]`` (``YuvFrame.layout``), goes to store slot ``slots[k]`` and is
    written B first if ``bgrs[k]``.  The surfaces are laid out back to back, as they come, at 4-byte aligned offsets behind ``_HEAD``
    bytes of slack; there is one horizontal set per distinct w, one vertical set per distinct h and one colour set per distinct set of
    integers.  Returns ``(table int32 CPU tensor, offsets, src_bytes, n_hsets, n_vsets, n_csets)``; the table has passed
    tady_ingest_plan_check.  ``cache``: as for ``plan_ingest`` -- between ticks of one fleet only the slot column changes.  Host only."""
    from . import kernels as K
    from .frame_resize import cubic_coeffs
    layouts = [tuple(l) for l in layouts]

    def recheck(table, k, at, counts):
        _lib.check_yuv(_lib.load_yuv().tady_ingest_plan_check(table.data_ptr(), table.numel(), k, *counts, at, int(F), int(S_h), int(S_w)),
                       "tady_ingest_plan_check")

    def build():
        offsets, at = _pack(l[7] for l in layouts)
        hsets, vsets, csets = {}, {}, {}
        rows = [(off, y_pitch, off + u_at, off + v_at, c_pitch, c_step, h, w, int(slot), hsets.setdefault(w, len(hsets)),
                 vsets.setdefault(h, len(vsets)), csets.setdefault(tuple(cset), len(csets)), _lib.YUV_BGR if bgr else 0)
                for off, (h, w, y_pitch, u_at, v_at, c_pitch, c_step, _, cset), slot, bgr in zip(offsets, layouts, slots, bgrs)]
        if len(hsets) > _lib.YUV_MAX_SETS or len(vsets) > _lib.YUV_MAX_SETS or len(csets) > _lib.YUV_MAX_CSETS:
            raise TadError(f"plan_ingest_yuv: {len(hsets)} distinct widths and {len(vsets)} distinct heights in one call, at most {_lib.YUV_MAX_SETS} each, "
                           f"and {len(csets)} colour sets, at most {_lib.YUV_MAX_CSETS}")
        table = K.ingest_yuv_table(rows, [(w, *cubic_coeffs(w, S_w)) for w in hsets], [(h, *cubic_coeffs(h, S_h)) for h in vsets], list(csets), at,
                                   F, S_h, S_w)
        return table, offsets, at, len(hsets), len(vsets), len(csets)

    key = ("yuv", tuple(layouts), tuple(bool(b) for b in bgrs), int(S_h), int(S_w))
    return _cached_plan(cache, key, slots, _lib.YUV_ROW_WORDS, 8, recheck, build)


class _Staging:
    """one pinned host buffer and its device twin, grown geometrically and kept between ticks; ``free`` is recorded behind the copy that
    reads the host side, and waited for before the host side is written again"""

    def __init__(self, dtype):
        self.dtype, self.host, self.dev, self.free = dtype, None, None, None

    def reserve(self, n, device):
        if self.host is None or self.host.numel() < n:
            cap = max(int(n), 2 * (self.host.numel() if self.host is not None else 0))
            self.host = torch.empty(cap, dtype=self.dtype, pin_memory=True)
            self.dev = torch.empty(cap, dtype=self.dtype, device=device)
            self.free = None
        if self.free is not None:
            self.free.synchronize()  # (the copy of two ticks ago: long done)

    def upload(self, n):
        self.dev[:n].copy_(self.host[:n], non_blocking=True)
        self.free = torch.cuda.Event()
        self.free.record()


class StreamBank:
    def __init__(self, model: torch.nn.Module, streams: int, mean=IMAGENET_MEAN, std=IMAGENET_STD, bgr=True,
                 device: Optional[torch.device] = None, use_graph: bool = False):
        from . import ops
        pe = model.patch_embed
        self.model = model
        self.T = int(model.num_frames)
        self.H, self.W = int(pe.img_size[0]), int(pe.img_size[1])
        self.device = device or next(model.parameters()).device
        if self.device.type != "cuda":
            raise TadError("StreamBank keeps its frames in HBM: the model must be on a GPU (no CPU path)")
        if ops.get_precision() == "precise":
            raise TadError(_PRECISE)
        if not 1 <= int(streams) <= _lib.BANK_MAX_FRAMES:
            raise TadError(f"StreamBank: streams={streams} must be in [1, {_lib.BANK_MAX_FRAMES}] (one ingest launch takes a frame of every stream)")
        self.rings = StreamRings(int(streams), self.T)
        self.S = self.rings.S
        per_stream = [bool(b) for b in bgr] if isinstance(bgr, (list, tuple)) else [bool(bgr)] * self.S
        if len(per_stream) != self.S:
            raise TadError(f"StreamBank: bgr names {len(per_stream)} streams, the bank has {self.S}")
        # one channel order for the store: the cameras' own when they agree, RGB (the BGR cameras swapped on their way in) when not
        self.store_bgr = all(per_stream)
        self.swap = [b != self.store_bgr for b in per_stream]
        pe.set_input_normalization(mean, std, bgr=self.store_bgr)
        self.store = torch.zeros((self.S * self.T, self.H, self.W, 3), dtype=torch.uint8, device=self.device)
        # two staging pairs, used in turn: the tick being packed never waits for the copy of the tick before it
        self._bytes = [_Staging(torch.uint8), _Staging(torch.uint8)]
        self._tables = [_Staging(torch.int32), _Staging(torch.int32)]
        self._tick = 0
        self._plans = {}  # plan_ingest's cache: the tables of the last mixes of sizes
        self._yuv_plans = {}  # plan_ingest_yuv's
        # use_graph: one captured graph per batch size A (the store and a static slot table are its inputs; the table is refilled by a
        # copy outside the graph), built lazily on a stream of this object's own and sharing one pool -- SlidingWindow's scheme, with A
        # in the place of the ring offset
        self.use_graph = bool(use_graph)
        self._graphs = {}
        self._pool = None
        self._params = list(model.parameters())
        self._sig = None
        self._cap_stream = None

    # ------------------------------------------------------------------ state
    @property
    def ready(self):
        """the stream ids that hold T frames, ascending (host side)"""
        return self.rings.ready

    @property
    def count(self):
        return self.rings.count

    @property
    def start(self):
        return self.rings.start

    def reset(self, stream: int) -> None:
        """camera reconnect: the stream starts filling again (its slots keep their bytes until they are overwritten; none is read before)"""
        (s,) = self.rings.check_ids([stream], "StreamBank.reset")
        self.rings.reset(s)

    def _drop_graphs(self) -> None:
        """forget every captured graph together with what only they needed: their memory pool, their slot tables and the scratch
        buffers of the capture stream"""
        self._graphs.clear()
        self._pool = None
        if self._cap_stream is not None:
            from . import kernels as K
            K.release_workspace(self.device, self._cap_stream)

    def __del__(self):
        try:
            self._drop_graphs()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass

    # ------------------------------------------------------------------ frames in
    @staticmethod
    def _frame(f, k):
        t = torch.from_numpy(np.ascontiguousarray(f)) if isinstance(f, np.ndarray) else f
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[-1] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
            got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(f).__name__
            raise TypeError(f"Input {k} must be a uint8 image of shape {('h', 'w', 3)}, but got {got}")
        if t.shape[0] > _lib.BANK_MAX_EXTENT or t.shape[1] > _lib.BANK_MAX_EXTENT:
            raise TadError(f"Input {k}: a frame of {t.shape[0]} x {t.shape[1]} pixels is above {_lib.BANK_MAX_EXTENT} per side")
        return t

    def _push(self, who: str, ids, frames: Sequence, of, plan, launch, stage, after=None) -> None:
        """What push_raw and push_yuv share.  ``of(f, k)`` validates frame k; ``plan(fs, ids, slots)`` is the planner's tuple ``(table,
        offsets, src_bytes, *set counts)``; ``stage(host, f, at)`` copies a frame into the pinned bytes, ``after(dev, f, at)`` into their
        device twin behind the upload; ``launch`` is the kernel's binding.  Everything is checked before the state moves or anything is
        launched."""
        if ops_precise():
            raise TadError(_PRECISE)
        ids = self.rings.check_ids(ids, who)
        if len(frames) != len(ids):
            raise TadError(f"{who}: {len(ids)} stream ids and {len(frames)} frames")
        fs = [of(f, k) for k, f in enumerate(frames)]
        if not ids:
            return
        # the slots these frames will take, worked out on a copy: the rings move only once the table has passed its check
        trial = StreamRings(self.S, self.T)
        trial.count, trial.start = list(self.rings.count), list(self.rings.start)
        table, offsets, nbytes, *counts = plan(fs, ids, trial.assign(ids))
        with torch.cuda.device(self.device):
            sb, st = self._bytes[self._tick & 1], self._tables[self._tick & 1]
            self._tick += 1
            total = nbytes + _HEAD  # (slack behind the last frame as in front of the first)
            sb.reserve(total, self.device)
            st.reserve(table.numel(), self.device)
            host = sb.host.numpy()
            for f, at in zip(fs, offsets):
                stage(host, f, at)
            st.host[:table.numel()].copy_(table)
            sb.upload(total)
            st.upload(table.numel())
            if after is not None:
                for f, at in zip(fs, offsets):
                    after(sb.dev, f, at)
            launch(sb.dev, nbytes, self.store, st.dev[:table.numel()], len(ids), *counts)
        self.rings.count, self.rings.start = trial.count, trial.start

    def push_raw(self, ids, frames: Sequence) -> None:
        """K frames uint8 [h_k, w_k, 3] of ANY sizes, as decoded (numpy arrays or tensors; device tensors are copied in), one for each of
        the K distinct streams ``ids``: resized on the device into the ring slots ``SlidingWindow.push_raw`` would have written, ONE
        launch.  Everything is checked before the state moves or anything is launched."""
        from . import kernels as K

        def plan(fs, ids, slots):
            return plan_ingest([tuple(f.shape[:2]) for f in fs], slots, [self.swap[s] for s in ids], self.H, self.W, self.S * self.T, self._plans)

        def stage(host, f, at):
            if not f.is_cuda:
                host[at:at + f.numel()] = f.contiguous().numpy().reshape(-1)

        def after(dev, f, at):
            if f.is_cuda:
                dev[at:at + f.numel()].copy_(f.reshape(-1), non_blocking=True)

        self._push("StreamBank.push_raw", ids, frames, self._frame, plan, K.ingest_frames, stage, after)

    def push_yuv(self, ids, frames: Sequence) -> None:
        """K 4:2:0 YUV frames of ANY sizes and layouts, as the cameras or decoders deliver them (``YuvFrame``: NV12, NV21 or I420,
        pitched or not; a bare uint8 [h * 3 / 2, w] array is a contiguous NV12 frame), one for each of the K distinct streams ``ids``:
        the planes are packed as they come (one copy, no conversion on the host), converted to RGB and resized on the device into the
        ring slots ``push_raw`` would have written, ONE launch (``kernels.ingest_yuv``, include/tad_mi355x_yuv.h).  The channel order is
        the store's own, so a bank can take ``push_raw`` from some cameras and ``push_yuv`` from others.  Everything is checked before
        the state moves or anything is launched."""
        from . import kernels as K

        def plan(fs, ids, slots):
            return plan_ingest_yuv([f.layout for f in fs], slots, [self.store_bgr] * len(fs), self.H, self.W, self.S * self.T, self._yuv_plans)

        def stage(host, f, at):
            host[at:at + f.nbytes] = f.data.numpy()[:f.nbytes]

        self._push("StreamBank.push_yuv", ids, frames, YuvFrame.of, plan, K.ingest_yuv, stage)

    def push(self, ids, frames) -> None:
        """frames: uint8 [K,H,W,3] (numpy or tensor, host or device), already at the model's input size, frame k for stream ``ids[k]``:
        the same launch as ``push_raw`` with equal extents, which gives the input bytes back"""
        f = torch.from_numpy(np.ascontiguousarray(frames)) if isinstance(frames, np.ndarray) else frames
        if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or f.dim() != 4 or tuple(f.shape[1:]) != (self.H, self.W, 3):
            got = f"{f.dtype} {tuple(f.shape)}" if isinstance(f, torch.Tensor) else type(frames).__name__
            raise TypeError(f"Input must be uint8 frames of shape {('K', self.H, self.W, 3)}, but got {got}")
        self.push_raw(ids, list(f.unbind(0)))

    # ------------------------------------------------------------------ scores out
    @torch.no_grad()
    def predict(self, ids=None) -> dict:
        """The streams ``ids`` (default: every ready stream, ascending) as ONE batch: ``{"stream": int64 [A] (host), "logits": f32 [A,
        num_classes], "prob": f32 [A]}`` -- the raw logits and softmax(logits)[:, 1] as ``score_video`` gives them, on the model's
        device.  With no ready stream the shapes are (0,), (0, C), (0,).  A stream that is asked for and not ready raises."""
        if ops_precise():
            raise TadError(_PRECISE)
        if ids is None:
            ids = self.rings.ready
        else:
            ids = self.rings.check_ids(ids, "StreamBank.predict")
            for s in ids:
                if self.rings.count[s] < self.T:
                    raise TadError(f"We need at least {self.T} frames! (stream {s} has {self.rings.count[s]})")
        nc = int(self.model.num_classes)
        if not ids:
            return {"stream": torch.zeros(0, dtype=torch.int64), "logits": torch.zeros((0, nc), dtype=torch.float32, device=self.device),
                    "prob": torch.zeros(0, dtype=torch.float32, device=self.device)}
        from .frame_store import FrameWindows
        host = torch.from_numpy(self.rings.window_table(ids))
        self.model.eval()
        with torch.cuda.device(self.device):
            if not self.use_graph:
                out = self.model(FrameWindows(self.store, host.to(self.device), self.store_bgr))
            else:
                out = self._replay(host)
        logits = out.float()
        return {"stream": torch.tensor(ids, dtype=torch.int64), "logits": logits, "prob": torch.softmax(logits, dim=1)[:, 1]}

    def _replay(self, host):
        # A captured graph reads the 16-bit weight copies (ops._wcache) and scratch buffers by raw pointer: the graphs are dropped whenever
        # the weights may have changed, and each entry keeps the copies and the scratch buffers it was captured with alive.
        from . import kernels as K
        from . import ops
        from .frame_store import FrameWindows
        sig = (ops.weight_epoch(), tuple(p._version for p in self._params), tuple(p.data_ptr() for p in self._params[:4]))
        if sig != self._sig:
            self._drop_graphs()
            self._sig = sig
        A = int(host.shape[0])
        ent = self._graphs.get(A)
        if ent is None:
            # warm-up AND capture on one stream of this object's own (kernels.workspace is keyed by (device, stream): the warm-up
            # allocates exactly the scratch buffer the capture then bakes in); the slot table is the graph's static input
            idx = host.to(self.device)
            fw = FrameWindows(self.store, idx, self.store_bgr)
            if self._cap_stream is None:
                self._cap_stream = torch.cuda.Stream(self.device)
            side = self._cap_stream
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self.model(fw)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            if self._pool is None:
                self._pool = torch.cuda.graph_pool_handle()
            with torch.cuda.graph(g, pool=self._pool, stream=side):
                out = self.model(fw)
            ent = self._graphs[A] = (g, out, idx, ops.cached_weight_tensors(), K.workspace_refs(self.device, side))
        ent[2].copy_(host)  # outside the graph, on the current stream, in front of the replay
        ent[0].replay()
        return ent[1].clone()


def ops_precise() -> bool:
    from . import ops
    return ops.get_precision() == "precise"
