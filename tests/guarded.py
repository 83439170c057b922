"""Guard-band arena: run a kernel on operands that sit in ONE ordinary allocation, each between two poisoned guard bands, and
check afterwards that no byte outside the operands it may write has changed and that no result depends on a byte outside them.

    arena = GuardedArena(256 << 20, "cuda", poison="nan")
    x = arena.place(x_host, role="input")            # 256-byte aligned view, guard right before its first / after its last byte
    with arena.route(kernels):                       # the wrappers' own torch.empty / empty_like / zeros (outputs, workspaces,
        y = kernels.some_op(x)                       # _pad_reduction's copies) land in the arena too, NaN-filled
    arena.verify()                                   # every byte that is not the body of an output / inout / workspace is unchanged

What this establishes: no store lands on, and (together with the caller's value comparison) no result depends on, bytes outside
the operands.  What it cannot: an over-read whose value is discarded (loaded, then masked) changes nothing and is not seen, and
inside the arena it cannot fault either -- "no address outside the operands is ever issued" is NOT shown.

Poison modes (guards around floating-point tensors): "nan" = quiet NaN of the neighbour's format, "huge" = its largest finite
positive value.  Both are needed: a hardware max returns the non-NaN operand, so NaN does not show in a softmax maximum; and a huge
value is hidden where a product with 0 follows.  Guards around index tensors hold in-range indices (never a wild address), around
uint8 frames 0xFF.  Everything lives inside one allocation: nothing here can provoke a fault.
"""
from __future__ import annotations

import contextlib

import torch

ALIGN = 256
TILE_ROWS = 256  # the tallest tile any launcher uses
MIN_GUARD = 64 << 10
POISON_MODES = ("nan", "huge")

# bit patterns per floating-point format: (integer view dtype, quiet NaN, largest finite positive)
_BITS = {
    torch.bfloat16: (torch.int16, 0x7FC0, 0x7F7F),
    torch.float16: (torch.int16, 0x7E00, 0x7BFF),
    torch.float32: (torch.int32, 0x7FC00000, 0x7F7FFFFF),
}
MUTABLE = ("output", "inout", "workspace")
ROLES = ("input",) + MUTABLE


class GuardViolation(AssertionError):
    pass


def poison_bits(dtype, mode):
    """(integer view dtype, bit pattern) of the poison of a floating-point ``dtype`` under ``mode``"""
    view, nan, huge = _BITS[dtype]
    return view, (nan if mode == "nan" else huge)


def bits(t):
    """the tensor's bit patterns as an integer tensor (bit-for-bit comparisons that do not trip over NaN != NaN)"""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a).cpu(), bits(b).cpu())


def _up(n, a=ALIGN):
    return (n + a - 1) // a * a


def _itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


class Placement:
    __slots__ = ("name", "role", "dtype", "shape", "lo", "start", "end", "hi", "view")

    def __repr__(self):
        return f"{self.name} ({self.role} {str(self.dtype).replace('torch.', '')}{list(self.shape)})"


class GuardedArena:
    def __init__(self, nbytes, device, poison="nan"):
        assert poison in POISON_MODES and nbytes <= (1 << 30), "poison mode nan|huge; the arena is at most 1 GiB"
        self.device = torch.device(device)
        self.poison = poison
        self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        self.snap = torch.empty_like(self.buf)
        assert self.buf.data_ptr() % ALIGN == 0 or self.device.type == "cpu"
        self.base = (-self.buf.data_ptr()) % ALIGN  # (a CPU allocation is 64-byte aligned only)
        self.reset()

    def reset(self, poison=None):
        """forget every placement (the bytes stay; each new placement fills its own guards and body)"""
        if poison is not None:
            assert poison in POISON_MODES
            self.poison = poison
        self.cursor = self.base
        self.placements = []

    # ------------------------------------------------------------------ layout
    @staticmethod
    def guard_bytes(shape, dtype, pitch=None):
        """at least 64 KiB and 256 rows of the tensor's row pitch (a tensor without rows: one element), a multiple of 256"""
        if pitch is None:
            pitch = (shape[-1] if len(shape) >= 2 else 1) * _itemsize(dtype)
        return _up(max(MIN_GUARD, TILE_ROWS * int(pitch)))

    def _fill(self, lo, hi, dtype, role, index_range, pattern, anchor):
        """fill arena bytes [lo, hi) with guard content; ``anchor`` is a byte on the element grid (the body's first / one past its last)"""
        if hi <= lo:
            return
        item = _itemsize(dtype)
        assert (lo - anchor) % item == 0 and (hi - lo) % item == 0
        n = (hi - lo) // item
        region = self.buf[lo:hi]
        if pattern is not None:  # caller-supplied elements, tiled so that a whole pattern starts at ``anchor``
            pat = pattern.to(dtype).reshape(-1)
            k = pat.numel()
            phase = ((lo - anchor) // item) % k
            region.view(dtype).copy_(pat.repeat((n + phase + k - 1) // k)[phase:phase + n])
        elif index_range is not None:  # in-range indices, a fixed pseudo-random sequence
            g = torch.Generator().manual_seed(lo & 0x7fffffff)
            region.view(dtype).copy_(torch.randint(0, int(index_range), (n,), generator=g).to(dtype))
        elif dtype in _BITS:
            view, val = poison_bits(dtype, self.poison)
            region.view(view).fill_(val)
        elif dtype == torch.uint8 and role == "workspace":  # scratch is read as f32 partial sums
            view, val = poison_bits(torch.float32, self.poison)
            a, b = lo + (-lo) % 4, hi - hi % 4  # (whole 4-byte words; the bytes an offset= placement leaves around them: 0xFF)
            self.buf[a:b].view(view).fill_(val)
            self.buf[lo:a].fill_(0xFF)
            self.buf[b:hi].fill_(0xFF)
        elif dtype == torch.uint8:
            region.fill_(0xFF)
        else:
            raise ValueError(f"guards around a {dtype} tensor need index_range= or guard_pattern= (no wild indices / addresses)")

    def place(self, tensor_or_shape, dtype=None, role="input", name=None, index_range=None, guard_pattern=None, pitch=None, fill=None, offset=0):
        """A view of the arena: 256-byte aligned start, a guard band immediately before the first and immediately after the last byte.
        offset=k (bytes, a multiple of the element size, default 0): the view starts k bytes behind the 256-byte boundary instead -- the
        guard before it grows by k bytes and still ends immediately before the first byte (tests/test_alignment_gpu.py).
        tensor_or_shape: a tensor (its values become the body) or a shape (then ``dtype`` is required).
        role: input | output | inout | workspace.  output / workspace bodies without data are filled with NaN of their dtype
        (``fill`` overrides: torch.zeros); integer ones with 0x7F bytes.
        index_range=n: guards of an integer tensor hold indices in [0, n).  guard_pattern=(before, after): element sequences tiled
        into the two guards (tables of offsets or addresses: rows that stay valid)."""
        assert role in ROLES, role
        data = tensor_or_shape if isinstance(tensor_or_shape, torch.Tensor) else None
        shape = tuple(data.shape) if data is not None else tuple(int(s) for s in tensor_or_shape)
        dtype = data.dtype if data is not None else dtype
        assert dtype is not None, "place(shape) needs a dtype"
        item = _itemsize(dtype)
        offset = int(offset)
        assert offset >= 0 and offset % item == 0, "offset= is in bytes and must keep the elements on their own grid"
        numel = 1
        for s in shape:
            numel *= s
        g = self.guard_bytes(shape, dtype, pitch)
        p = Placement()
        p.name, p.role, p.dtype, p.shape = name or f"#{len(self.placements)}", role, dtype, shape
        p.lo = self.cursor                      # (on the 256-byte grid)
        p.start = p.lo + g + offset
        p.end = p.start + numel * item          # no rounding: the first guard byte is the byte after the last element
        p.hi = p.end + g + (-(p.end + g - self.base)) % ALIGN  # (back on the grid: a whole number of guard elements of any type)
        if p.hi > self.buf.numel():
            raise MemoryError(f"guarded arena of {self.buf.numel()} bytes is full placing {p}")
        pre, post = guard_pattern if guard_pattern is not None else (None, None)
        self._fill(p.lo, p.start, dtype, role, index_range, pre, p.start)
        self._fill(p.end, p.hi, dtype, role, index_range, post, p.end)
        body = self.buf[p.start:p.end].view(dtype).view(shape)
        if data is not None:
            body.copy_(data)
        elif fill is not None:
            body.fill_(fill)
        elif role in ("output", "workspace"):
            if dtype in _BITS:
                body.fill_(float("nan"))
            elif dtype == torch.uint8 and role == "workspace":
                first = p.start + (-p.start) % 4  # (whole 4-byte words; an offset= placement leaves up to 3 bytes in front of them)
                whole = max(first, p.end - p.end % 4)
                self.buf[first:whole].view(torch.float32).fill_(float("nan"))
                self.buf[p.start:first].fill_(0xFF)
                self.buf[whole:p.end].fill_(0xFF)
            else:
                self.buf[p.start:p.end].fill_(0x7F)
        p.view = body
        self.snap[p.lo:p.hi].copy_(self.buf[p.lo:p.hi])  # stream-ordered before whatever is launched next
        self.cursor = p.hi
        self.placements.append(p)
        return body

    def contains(self, t):
        """is the tensor's storage inside the arena (a placement or a view of one)?"""
        off = t.data_ptr() - self.buf.data_ptr()
        return t.device == self.buf.device and 0 <= off and off + t.numel() * t.element_size() <= self.buf.numel()

    def placement_of(self, t):
        off = t.data_ptr() - self.buf.data_ptr()
        for p in self.placements:
            if p.start == off:
                return p
        raise KeyError("not the start of a placement")

    # ------------------------------------------------------------------ snapshot / verify
    def snapshot(self):
        """take the reference image again (after the test has written input bodies by hand)"""
        self.snap[:self.cursor].copy_(self.buf[:self.cursor])

    def verify(self):
        """every byte that is not the body of an output / inout / workspace placement must equal the snapshot"""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        diff = self.buf[:self.cursor] != self.snap[:self.cursor]
        diff[:self.base] = False
        for p in self.placements:
            if p.role in MUTABLE:
                diff[p.start:p.end] = False
        if not bool(diff.any()):
            return
        bad = diff.nonzero().reshape(-1).cpu()
        msgs = []
        for p in self.placements:
            for what, a, b, origin in (("guard before", p.lo, p.start, p.start), ("body of input", p.start, p.end, p.start),
                                       ("guard after", p.end, p.hi, p.end)):
                sel = bad[(bad >= a) & (bad < b)]
                if sel.numel():
                    rel = "its first byte" if origin == p.start else "the byte after its last"
                    msgs.append(f"{what} {p}: {sel.numel()} byte(s) changed, offsets {int(sel[0]) - origin:+d} .. {int(sel[-1]) - origin:+d} "
                                f"relative to {rel}")
        raise GuardViolation("bytes outside the writable operands changed:\n  " + "\n  ".join(msgs))

    # ------------------------------------------------------------------ routing the wrappers' own allocations
    @contextlib.contextmanager
    def route(self, kernels_module):
        """Inside the block the module's ``torch.empty`` / ``empty_like`` / ``zeros`` for this arena's device, and the copies
        ``torch.nn.functional.pad`` makes of device tensors, are placements of this arena (outputs NaN-filled, padded copies
        inputs): the production wrapper -- plan selection, padding, workspace sizing -- runs unchanged on guarded memory.
        The module's cached workspaces are dropped on entry and on exit."""
        saved = kernels_module.torch
        kernels_module._workspaces.clear()
        kernels_module.torch = _TorchProxy(self)
        try:
            yield self
        finally:
            kernels_module.torch = saved
            kernels_module._workspaces.clear()


class _Forward:
    def __init__(self, target, **overrides):
        self.__dict__["_target"] = target
        self.__dict__.update(overrides)

    def __getattr__(self, name):
        return getattr(self._target, name)


class _TorchProxy(_Forward):
    """forwards everything to torch except empty / empty_like / zeros / nn.functional.pad for tensors on the arena's device"""

    def __init__(self, arena):
        super().__init__(torch)
        self.__dict__["_arena"] = arena
        self.__dict__["nn"] = _Forward(torch.nn, functional=_Forward(torch.nn.functional, pad=self._pad))

    def _mine(self, device):
        return device is not None and torch.device(device).type == self._arena.device.type

    @staticmethod
    def _shape(size):
        if len(size) == 1 and not isinstance(size[0], int):
            return tuple(size[0])
        return tuple(size)

    def empty(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        shape = self._shape(size)
        role = "workspace" if (dtype == torch.uint8 and len(shape) == 1) else "output"
        return self._arena.place(shape, dtype or torch.float32, role, name=f"wrapper {role} #{len(self._arena.placements)}")

    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.zeros(*size, dtype=dtype, device=device, **kw)
        return self._arena.place(self._shape(size), dtype or torch.float32, "output", fill=0, name=f"wrapper zeros #{len(self._arena.placements)}")

    def empty_like(self, t, dtype=None, device=None, **kw):
        if not self._mine(device if device is not None else t.device):
            return torch.empty_like(t, dtype=dtype, device=device, **kw)
        return self._arena.place(tuple(t.shape), dtype or t.dtype, "output", name=f"wrapper output #{len(self._arena.placements)}")

    def _pad(self, t, *a, **kw):
        r = torch.nn.functional.pad(t, *a, **kw)
        if not self._mine(t.device):
            return r
        return self._arena.place(r, role="input", name=f"wrapper padded copy #{len(self._arena.placements)}")
