"""Host-fed clips: ``ClipPrefetcher`` wraps any iterable loader and hands the engines batches that already are on the device.

The reference moves a fresh batch every step with ``pin_memory`` and ``prefetch_factor`` (engine_for_finetuning.py:56-57,
run_class_finetuning.py:266-274).  The engines here do a bare ``samples.to(device, non_blocking=True)``: from pageable memory that copy
runs on the compute stream, serialised with the step.  Wrapped, the copy of batch i+1 runs on a private side stream from a pinned slot
while step i computes, and ``.to(device)`` on what the engine receives is a no-op -- no engine signature changes:

    train_one_epoch(model, criterion, ClipPrefetcher(loader, device), optimizer, device, ...)

Contract
  * one producer thread per ``__iter__``; batches in the loader's order and nesting (tuple / list / dict); every tensor leaf on
    ``device``, every other leaf (names, ints) untouched; ``len`` and unknown attributes (``sampler``, ``dataset``) are the loader's.
  * producer, per batch: take the next host batch; stage every tensor leaf that is not already pinned into a pinned slot of a
    ``depth``-deep ring (slots per leaf path, allocated lazily, regrown when a larger shape arrives, a shorter last batch uses a view);
    copy to a FRESHLY allocated device tensor on the side stream; record an event.  A pinned contiguous leaf is copied from directly.
    A slot is written again only after the event of its last copy has completed: a host-side wait in the producer thread, never on
    the compute stream.
  * consumer: ``__next__`` makes the current stream wait on the batch's event and calls ``record_stream`` on each tensor.  No host
    synchronisation, no stream drain.
  * the producer has taken at most ``depth`` batches more from the loader than ``__next__`` has returned; at most ``depth + 1``
    batches are alive on the device (``depth`` in flight and the one the step holds), plus ``depth`` pinned slot sets.
  * an exception of the loader or of staging is re-raised by ``__next__`` at the position where it happened, after every earlier batch.
  * ``close()``, an early ``break``, a second ``__iter__`` and garbage collection stop and join the producer (daemon thread, join
    timeout).  No thread pool.
  * ``device.type == "cpu"``: the same rotation with plain copies and no pinning (hosts without a GPU, tests).

``wire``
  "same"     every dtype as the loader yields it.
  "operand"  ``batch[clip_index]``, when it is a 5-D f32 clip, travels in the current 16-bit operand format (bfloat16 under "fast", IEEE
             half under "half"; read at ``__iter__``; "precise" raises ValueError).  The rounding happens in the staging pass itself
             (``pinned16.copy_(src32)``: the one host pass that has to happen anyway), so the wire and the HBM copy are half the bytes,
             and PatchEmbed moves the 16-bit words straight into its patch matrix (ops.PatchEmbed16Fn) -- the same bits as from the f32
             clip, which the im2col rounds the same way.  ONLY for loaders that yield the reference's CPU-augmented, normalised f32
             clips with no f32 device stage behind them (no ``augment_fn`` / ``erase_fn`` / ``mixup_fn``: those compute in f32 on what
             they are given).  The MAE engine computes its target from the f32 clip: ``wire="same"`` only.
"""
from __future__ import annotations

import queue
import threading

import torch

JOIN_TIMEOUT_S = 5.0
_ITEM, _END, _ERR = range(3)


def _map_leaves(node, fn, path=()):
    """rebuild the nesting of ``node`` (tuple / list / dict) with fn(leaf, path) in place of every leaf"""
    if isinstance(node, dict):
        out = {k: _map_leaves(v, fn, path + (k,)) for k, v in node.items()}
        return out if type(node) is dict else type(node)(out)
    if isinstance(node, tuple) and hasattr(node, "_fields"):  # namedtuple
        return type(node)(*[_map_leaves(v, fn, path + (i,)) for i, v in enumerate(node)])
    if isinstance(node, (tuple, list)):
        return type(node)(_map_leaves(v, fn, path + (i,)) for i, v in enumerate(node))
    return fn(node, path)


class _Epoch:
    """what one producer thread and its consumer share; holds no reference to the iterator object, so that dropping the iterator (an
    early ``break``) can stop the thread"""

    def __init__(self, device, depth, wire_dtype, clip_index, slots):
        self.device, self.depth, self.wire_dtype, self.clip_path, self.slots = device, depth, wire_dtype, (clip_index,), slots
        self.cuda = device.type == "cuda"
        self.side = torch.cuda.Stream(device) if self.cuda else None
        self.slot_events = [None] * depth  # event of the last copy out of each ring position
        self.q = queue.Queue()             # (kind, payload); never more than depth + 1 entries: bounded by the permits
        self.cv = threading.Condition()
        self.permits = depth
        self.stopped = False
        self.thread = None

    # ------------------------------------------------------------------ producer side
    def _take_permit(self) -> bool:
        with self.cv:
            while self.permits == 0 and not self.stopped:
                self.cv.wait()
            if self.stopped:
                return False
            self.permits -= 1
            return True

    def _slot(self, path, ring, numel, dtype):
        """the staging buffer of leaf ``path`` at ring position ``ring``, at least ``numel`` elements of ``dtype``"""
        ring_slots = self.slots.setdefault(path, [None] * self.depth)
        buf = ring_slots[ring]
        if buf is None or buf.dtype != dtype or buf.numel() < numel:
            buf = ring_slots[ring] = torch.empty(max(numel, 1), dtype=dtype, pin_memory=self.cuda)
        return buf

    def _stage(self, i, host):
        """host batch i -> (batch on the device, its device tensors, the event behind which they are complete)"""
        ring = i % self.depth
        if self.slot_events[ring] is not None:
            self.slot_events[ring].synchronize()  # the slot's last copy has left it (host wait, this thread only)
            self.slot_events[ring] = None
        moved = []

        def leaf(t, path):
            if not torch.is_tensor(t) or (self.cuda and t.device == self.device):
                return t
            if t.device.type != "cpu":
                return t.to(self.device)
            dtype = t.dtype
            if self.wire_dtype is not None and path == self.clip_path and t.dim() == 5 and t.dtype == torch.float32:
                dtype = self.wire_dtype
            if self.cuda and dtype == t.dtype and t.is_contiguous() and t.is_pinned():
                src = t
            else:
                src = self._slot(path, ring, t.numel(), dtype)[:t.numel()].view(t.shape)
                src.copy_(t)  # the one host pass: pageable -> pinned, and the rounding of wire="operand"
            dev = torch.empty(t.shape, dtype=dtype, device=self.device)
            dev.copy_(src, non_blocking=True)
            moved.append((dev, t if src is t else None))
            return dev

        if not self.cuda:
            return _map_leaves(host, leaf), (), None
        with torch.cuda.stream(self.side):
            out = _map_leaves(host, leaf)
            ev = torch.cuda.Event()
            ev.record(self.side)
        self.slot_events[ring] = ev
        # (a pinned source that was copied from directly stays referenced until its batch has been handed over)
        return out, moved, ev

    def produce(self, it):
        try:
            i = 0
            while self._take_permit():
                try:
                    host = next(it)
                except StopIteration:
                    self.q.put((_END, None))
                    return
                self.q.put((_ITEM, self._stage(i, host)))
                i += 1
        except BaseException as e:  # noqa: BLE001 -- handed to the consumer, which re-raises it in its place
            self.q.put((_ERR, e))

    # ------------------------------------------------------------------ consumer side
    def release_permit(self):
        with self.cv:
            self.permits += 1
            self.cv.notify()

    def stop(self) -> bool:
        """stop and join the producer; False if it did not end within the timeout (stuck inside the loader)"""
        with self.cv:
            self.stopped = True
            self.cv.notify_all()
        th = self.thread
        if th is not None and th is not threading.current_thread():
            th.join(JOIN_TIMEOUT_S)
        try:
            while True:
                self.q.get_nowait()  # let go of the batches nobody will take
        except queue.Empty:
            pass
        return th is None or not th.is_alive()


class _EpochIterator:
    def __init__(self, epoch, owner):
        self._epoch, self._owner = epoch, owner  # (the wrapper lives as long as an iterator of it does)

    def __iter__(self):
        return self

    def __next__(self):
        ep = self._epoch
        while True:
            if ep.stopped:
                raise StopIteration
            try:
                kind, payload = ep.q.get(timeout=1.0)
                break
            except queue.Empty:
                if not ep.thread.is_alive() and ep.q.empty():
                    ep.stop()
                    raise RuntimeError("ClipPrefetcher: the producer thread ended without a result")
        if kind == _END:
            ep.stop()
            raise StopIteration
        if kind == _ERR:
            ep.stop()
            raise payload
        batch, moved, ev = payload
        if ev is not None:
            cur = torch.cuda.current_stream(ep.device)
            cur.wait_event(ev)
            for dev, _src in moved:
                dev.record_stream(cur)
        ep.release_permit()
        return batch

    def close(self):
        self._epoch.stop()

    def __del__(self):
        try:
            self._epoch.stop()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass


class ClipPrefetcher:
    """see the module docstring.  ``ClipPrefetcher(loader, device, depth=2, wire="same", clip_index=0)``"""

    def __init__(self, loader, device, depth: int = 2, wire: str = "same", clip_index: int = 0):
        if int(depth) < 1:
            raise ValueError(f"ClipPrefetcher: depth must be >= 1, got {depth}")
        if wire not in ("same", "operand"):
            raise ValueError(f'ClipPrefetcher: wire must be "same" or "operand", got {wire!r}')
        self.loader = loader
        self.device = torch.device(device)
        self.depth, self.wire, self.clip_index = int(depth), wire, clip_index
        self._slots = {}
        self._epoch = None

    def __len__(self):
        return len(self.loader)

    def __getattr__(self, name):  # (only reached for names this object does not have)
        if name.startswith("__") or name in ("loader", "_epoch", "_slots"):
            raise AttributeError(name)
        return getattr(self.loader, name)

    def _wire_dtype(self):
        if self.wire == "same":
            return None
        from . import ops
        if ops.get_precision() == "precise":
            raise ValueError('ClipPrefetcher: wire="operand" needs a 16-bit operand format; precision "precise" computes on the f32 clip '
                             '(use wire="same")')
        return ops.K.operand_dtype()

    def __iter__(self):
        self.close()
        wire_dtype = self._wire_dtype()
        device = self.device
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        it = iter(self.loader)  # (in the caller's thread: what iter() raises is raised here)
        ep = _Epoch(device, self.depth, wire_dtype, self.clip_index, self._slots)
        ep.thread = threading.Thread(target=ep.produce, args=(it,), name="ClipPrefetcher", daemon=True)
        self._epoch = ep
        ep.thread.start()
        return _EpochIterator(ep, self)

    def close(self):
        """stop and join the producer of the current epoch, if any; the pinned slots are kept for the next one"""
        ep, self._epoch = self._epoch, None
        if ep is not None and not ep.stop():
            self._slots = {}  # a producer stuck inside its loader may still write its slots: the next epoch gets its own

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass
