"""Guard bands around kernel outputs and poisoned padding around kernel inputs (tests only).

guarded_out(shape, dtype, ld) places an output inside a larger allocation: a front guard, row-pitch padding when ld exceeds the last
dimension, and a back guard.  Every element of the allocation starts as a sentinel bit pattern (a NaN with a payload for float types, 0xA5 bytes
for integer types); check() compares everything outside the view bitwise with it, so a store past a row, a tile or the end of the output is
reported even where it wrote a NaN.  poisoned_in(data, ld) is the same layout for inputs: the padding holds NaN / +-Inf / 65504 for float types
and all-ones for integer ones (255 / 65535), so a read outside the view reaches the result.

Guards are whole tiles of the kernel under test (guard_rows rows of ld elements on each side, at least MIN_GUARD_BYTES), so a plausible overrun
stays inside the test's own allocation.  The view starts 16-byte aligned."""
import torch

MIN_GUARD_BYTES = 4096
# the sentinel of each element type: the bits a stray store would have to reproduce exactly to go unseen
SENTINEL = {torch.float32: 0x7FA5A5A5, torch.float16: 0x7DA5, torch.bfloat16: 0x7FA5, torch.float64: 0x7FF4A5A5A5A5A5A5,
            torch.uint8: 0xA5, torch.int16: 0xA5A5, torch.int32: 0xA5A5A5A5, torch.int64: 0xA5A5A5A5A5A5A5A5}
ALT_SENTINEL = {torch.uint8: 0x5A, torch.int16: 0x5A5A, torch.int32: 0x5A5A5A5A}  # the second run of an integer output
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_POISON_F = (float("nan"), float("inf"), -float("inf"), 65504.0)


def _signed(v, nbytes):
    """a bit pattern as the integer of the view type of its width (uint8 unsigned, wider ones signed)"""
    v &= (1 << (8 * nbytes)) - 1
    if nbytes == 1:
        return v
    return v - (1 << (8 * nbytes)) if v >= 1 << (8 * nbytes - 1) else v


class Guarded:
    """`view` (`shape`, rows ld elements apart) inside `base`, a flat allocation of `total` elements whose first `front` lie before the view."""

    def __init__(self, shape, dtype, ld=None, guard_rows=256, device="cuda"):
        shape = tuple(int(s) for s in shape)
        self.shape, self.dtype = shape, dtype
        self.width = shape[-1]
        self.rows = 1
        for s in shape[:-1]:
            self.rows *= s
        self.ld = int(ld) if ld is not None else self.width
        assert self.ld >= self.width, (self.ld, self.width)
        es = torch.empty((), dtype=dtype).element_size()
        self.nbytes = es
        align = max(1, 16 // es)
        guard = max(guard_rows * self.ld, MIN_GUARD_BYTES // es)
        self.front = (guard + align - 1) // align * align
        self.span = (self.rows - 1) * self.ld + self.width if self.rows > 0 else 0
        self.total = self.front + self.span + guard
        self.base = torch.empty((self.total,), dtype=dtype, device=device)
        self.ibase = self.base.view(_BITS[es])
        strides, acc = [], 1
        for i, s in enumerate(reversed(shape)):
            strides.append(acc)
            acc *= self.ld if i == 0 else s
        self.view = self.base.as_strided(shape, tuple(reversed(strides)), self.front)
        idx = torch.arange(self.total, device=device).as_strided(shape, self.view.stride(), self.front)
        self.outside = torch.ones((self.total,), dtype=torch.bool, device=device)
        self.outside[idx.reshape(-1)] = False

    def locate(self, flat):
        """flat index into base -> (row, column) relative to the view's first element"""
        off = int(flat) - self.front
        return off // self.ld, off % self.ld


class GuardedOut(Guarded):
    def __init__(self, shape, dtype, ld=None, guard_rows=256, device="cuda", sentinel=None, init=None):
        super().__init__(shape, dtype, ld, guard_rows, device)
        self.sentinel = _signed(SENTINEL[dtype] if sentinel is None else sentinel, self.nbytes)
        self.ibase.fill_(self.sentinel)
        if init is not None:
            self.view.copy_(init)

    def check(self, what="output"):
        """every element outside the view still holds the sentinel's bits; else name the first one that does not"""
        if self.base.is_cuda:
            torch.cuda.synchronize(self.base.device)
        bad = (self.ibase != self.sentinel) & self.outside
        n = int(bad.sum())
        if n:
            first = int(torch.nonzero(bad)[0, 0])
            row, col = self.locate(first)
            where = ("before the view" if first < self.front else
                     "behind the view" if first >= self.front + self.span else "in the row padding")
            bits = int(self.ibase[first]) & ((1 << 8 * self.nbytes) - 1)
            raise AssertionError(f"{what} {self.shape} (ld {self.ld}): {n} element(s) outside the view changed; the first at (row {row}, column {col}) "
                                 f"relative to the view, {where}: bits {bits:#x}")


def guarded(shape, dtype, ld=None, guard_rows=256, device="cuda", sentinel=None, init=None):
    """the GuardedOut object (view, check, base, front, ...) for tests that need the layout"""
    return GuardedOut(shape, dtype, ld, guard_rows, device, sentinel, init)


def guarded_out(shape, dtype, ld=None, guard_rows=256, device="cuda", sentinel=None, init=None):
    """-> (view, check): an output of `shape` inside guard bands of sentinel bits.  init = the view's starting content (in-place operations);
    without it the view holds the sentinel too, so an element the kernel should write and does not stays a NaN."""
    g = GuardedOut(shape, dtype, ld, guard_rows, device, sentinel, init)
    return g.view, g.check


def poison_bits(dtype, n, device="cuda"):
    """n elements cycling through the poison values of dtype, as the integer view type of its width"""
    es = torch.empty((), dtype=dtype).element_size()
    if dtype.is_floating_point:
        vals = torch.tensor(_POISON_F, dtype=torch.float32).to(dtype).view(_BITS[es])
    else:
        vals = torch.tensor([_signed(-1, es)], dtype=_BITS[es])
    return vals.to(device)[torch.arange(n, device=device) % vals.numel()]


def poisoned_in(data, ld=None, guard_rows=256):
    """data (rows = its last dimension) copied into a view whose row padding and guard bands hold poison: NaN / +Inf / -Inf / 65504 for float
    types, all ones (255 / 65535) for uint8 / 16-bit integer images and maps"""
    g = Guarded(data.shape, data.dtype, ld, guard_rows, data.device)
    g.ibase.copy_(poison_bits(data.dtype, g.total, data.device))
    g.view.copy_(data)
    return g.view
