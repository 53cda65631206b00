"""One caller arena for all the planes of a stage call: what a real host of the reference does (it sub-allocates its planes), and what
makes a stray access of a kernel visible.

Every other GPU test hands the library planes that are separate torch allocations: 512-byte aligned, followed by the caching allocator's
slack, which is usually zero — and an all-zero texel is "sky with a zero normal, weight exactly 0", the CORRECT value of a tap outside the
frame.  A buffer resource a row too long, a `row_ok` off by one on a strip, a gather without its in-frame test: all pass
there.  An `Arena` is ONE uint8 allocation that holds the named planes of a call with margins of known content around them:

    layout   spaced: every plane has a margin of its own before and after it, at least `margin_rows` rows of THAT plane and never below
             4 KiB (margin_rows = the call's reach + 8: the a-trous reach is 2 * step rows, the moments reach 3, the temporal reach the
             case's motion) — a row-indexed overrun in either direction lands in a margin;
             tight: the planes back to back (largest texel first, so that each stays aligned to its texel), margins at the two ends only —
             an overrun of one plane lands in its live neighbour.
    offset   a plane starts k texels (k in {0, 1, 3}) behind a 512-byte boundary: bases at 16-, 8-, 4-byte and odd addresses where the
             texel allows it, never below the texel's own alignment (include/svgf.h, Conventions).
    fill     "nan": the quiet-NaN sentinel of the plane's element type (0xA5 for bytes); "zero"; "live": the plane's own first / last rows
             mirrored outwards, so that a stray tap lands on a plausible surface texel and gets full weight (history: bytes drawn from
             both sides of the "young" limit of 4).  The exact second pass of the streaming kernels drops a NaN tap (fmax) and a zero tap
             is a sky tap: only a live texel cannot hide a stray read.

Checks: `assert_margins_intact()` (every byte outside the planes against the host copy of what was put there), `snapshot_inputs()` /
`assert_inputs_intact()` (named planes as raw bytes).  A failure names the plane, the side, and the byte as a row / column of that plane.

The module works on a CUDA device (torch) or, with device=None, on a numpy buffer (tests/test_plane_arena.py, no GPU)."""
from __future__ import annotations

import numpy as np

SENTINEL = {"f32": (np.uint32, 0x7FCADA55), "f16": (np.uint16, 0x7E55)}   # a quiet NaN no kernel and no input makes
BYTE_SENTINEL = 0xA5
ALIGN = 512                 # what a torch allocation is aligned to
MIN_MARGIN = 4096
OFFSETS = (0, 1, 3)
FILLS = ("nan", "zero", "live")


def _sentinel_plane(shape, storage):
    import torch
    u, v = SENTINEL[storage]
    it, ft = (torch.int32, torch.float32) if storage == "f32" else (torch.int16, torch.float16)
    return torch.full(shape, v, dtype=it, device="cuda").view(ft)


def _is_sentinel(a, storage):
    u, v = SENTINEL[storage]
    return a.view(u) == v


def sentinel_array(shape, dtype):
    """A host plane full of the sentinel of its element type (4-byte elements: the fp32 NaN, 2-byte: the fp16 NaN, bytes: 0xA5)."""
    dtype = np.dtype(dtype)
    if dtype.itemsize == 4:
        return np.full(shape, SENTINEL["f32"][1], np.uint32).view(dtype)
    if dtype.itemsize == 2:
        return np.full(shape, SENTINEL["f16"][1], np.uint16).view(dtype)
    return np.full(shape, BYTE_SENTINEL, np.uint8).view(dtype)


def is_sentinel_array(a):
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize == 4:
        return a.view(np.uint32) == SENTINEL["f32"][1]
    if a.dtype.itemsize == 2:
        return a.view(np.uint16) == SENTINEL["f16"][1]
    return a.view(np.uint8) == BYTE_SENTINEL


def margin_bytes(row_bytes, margin_rows):
    """The derived margin of a plane: `margin_rows` of its rows, never below 4 KiB."""
    return max(MIN_MARGIN, int(margin_rows) * int(row_bytes))


def mirror_rows(rows, n, side):
    """Indices of the n plane rows that continue a plane of `rows` rows outwards, nearest first: before the plane row -1 shows row 0, row -2
    row 1 ...; after it row `rows` shows row rows-1 ...; a margin taller than the plane keeps reflecting."""
    j = np.arange(n) % (2 * rows)
    j = np.where(j < rows, j, 2 * rows - 1 - j)
    return j if side == "before" else rows - 1 - j


class Plane:
    def __init__(self, name, shape, dtype, offset_k):
        self.name, self.shape, self.dtype, self.k = name, tuple(int(s) for s in shape), np.dtype(dtype), int(offset_k)
        self.rows, self.W = self.shape[0], self.shape[1]
        self.texel = int(np.prod(self.shape[2:], dtype=np.int64)) * self.dtype.itemsize
        self.row_bytes = self.W * self.texel
        self.nbytes = self.rows * self.row_bytes
        self.start = self.end = 0
        self.before = self.after = (0, 0)           # [lo, hi) of the margins that belong to this plane


class Arena:
    """specs: list of (name, shape, dtype) with shape (rows, W[, channels]); contents: name -> host array the plane starts out with (an input,
    or an output's pre-fill; a plane without one starts as the sentinel of its type); like: name -> name of the plane whose rows a "live"
    margin of an OUTPUT plane mirrors (default: its own contents); offsets: one k for all planes, or name -> k."""

    def __init__(self, specs, contents=None, *, fill="nan", tight=False, margin_rows=8, offsets=0, like=None, device="cuda", seed=0):
        assert fill in FILLS, fill
        contents, like = dict(contents or {}), dict(like or {})
        self.fill, self.tight, self.margin_rows, self.device = fill, bool(tight), int(margin_rows), device
        self.planes = {}
        order = []
        for i, (name, shape, dtype) in enumerate(specs):
            k = offsets.get(name, 0) if isinstance(offsets, dict) else int(offsets)
            assert k in OFFSETS, k
            p = Plane(name, shape, dtype, k)
            assert name not in self.planes, name
            self.planes[name] = p
            order.append(p)
        if tight:                                   # largest texel first: every plane then starts on a multiple of its own texel
            order.sort(key=lambda p: -p.texel)
        self.order = order
        # ---- layout
        cur = 0
        for i, p in enumerate(order):
            m = margin_bytes(p.row_bytes, self.margin_rows)
            if tight and i > 0:
                p.start = cur
                p.before = (cur, cur)
            else:
                p.start = (cur + m + ALIGN - 1) // ALIGN * ALIGN + p.k * p.texel
                p.before = (cur, p.start)
            p.end = p.start + p.nbytes
            assert p.start % p.texel == 0, (p.name, p.start, p.texel)
            if tight and i < len(order) - 1:
                p.after = (p.end, p.end)
            else:
                p.after = (p.end, p.end + m)
            cur = p.after[1]
        self.nbytes = cur
        # ---- host image: the planes' contents, then the margins
        rng = np.random.default_rng(seed)
        host = np.zeros(self.nbytes, np.uint8)
        init = {}
        for p in order:
            c = contents.get(p.name)
            c = sentinel_array(p.shape, p.dtype) if c is None else np.ascontiguousarray(c)
            assert c.shape == p.shape and c.dtype.itemsize == p.dtype.itemsize, (p.name, c.shape, c.dtype, p.shape, p.dtype)
            init[p.name] = c.view(p.dtype) if c.dtype != p.dtype else c
            host[p.start:p.end] = init[p.name].reshape(-1).view(np.uint8)
        for p in order:
            src = init[like[p.name]] if p.name in like else init[p.name]
            if p.name not in contents and p.name not in like and fill == "live":
                src = self._plausible(rng, p)       # an output nobody gave an image for: finite values of its type
            assert src.shape == p.shape, (p.name, src.shape)
            for side in ("before", "after"):
                lo, hi = getattr(p, side)
                if hi > lo:
                    host[lo:hi] = self._margin(rng, p, src, side, hi - lo)
        self.expected = host
        self.buf = self._upload(host)
        self._snap = {}

    # ---- fills
    @staticmethod
    def _plausible(rng, p):
        if p.dtype.itemsize == 1:
            return rng.choice(np.array([0, 1, 2, 3, 4, 7, 24, 255], np.uint8), p.shape)
        if p.dtype.kind == "f":
            return rng.uniform(0.05, 1.0, p.shape).astype(p.dtype)
        return np.frombuffer(rng.uniform(0.05, 1.0, p.shape).astype(np.float16 if p.dtype.itemsize == 2 else np.float32).tobytes(), p.dtype).reshape(p.shape)

    def _margin(self, rng, p, src, side, n):
        """n bytes that continue plane p on `side`, laid out so that the byte next to the plane is the nearest one."""
        nrows = -(-n // p.row_bytes)
        if self.fill == "zero":
            return np.zeros(n, np.uint8)
        if self.fill == "nan":
            ext = sentinel_array((nrows,) + p.shape[1:], p.dtype)
        elif p.dtype.itemsize == 1:                 # history: both sides of the "young" limit
            ext = rng.choice(np.array([0, 1, 2, 3, 4, 5, 24, 255], np.uint8), (nrows,) + p.shape[1:]).view(p.dtype)
        else:
            ext = src[mirror_rows(p.rows, nrows, side)]
        ext = np.ascontiguousarray(ext)
        if side == "before":                        # farthest row first; the plane's row -1 ends where the plane starts
            return np.ascontiguousarray(ext[::-1]).reshape(-1).view(np.uint8)[nrows * p.row_bytes - n:]
        return ext.reshape(-1).view(np.uint8)[:n]

    # ---- back ends
    def _upload(self, host):
        if self.device is None:
            return host.copy()
        import torch
        return torch.from_numpy(host.copy()).to(self.device)             # (a copy: on a CPU device .to() would share the host image's memory)

    def _download(self):
        if self.device is None:
            return self.buf
        return self.buf.detach().cpu().numpy()

    def view(self, name):
        """The plane as a view of the arena (torch tensor on the device, numpy array with device=None)."""
        p = self.planes[name]
        raw = self.buf[p.start:p.end]
        if self.device is None:
            return raw.view(p.dtype).reshape(p.shape)
        import torch
        tdt = {"float32": torch.float32, "float16": torch.float16, "uint8": torch.uint8, "int16": torch.int16, "uint16": torch.int16,
               "int32": torch.int32, "uint32": torch.int32}[p.dtype.name]
        return raw.view(tdt).view(p.shape)

    def views(self, *names):
        return [self.view(n) for n in names]

    def host(self, name):
        """A host copy of the plane as it is now."""
        p = self.planes[name]
        return self._download()[p.start:p.end].copy().view(p.dtype).reshape(p.shape)

    def address_offset(self, name):
        """The plane's byte offset behind the last 512-byte boundary."""
        return self.planes[name].start % ALIGN

    # ---- checks
    @staticmethod
    def _where(p, byte):
        """Arena byte -> (row, column, byte inside the texel) of plane p; rows before the plane are negative, rows after it >= p.rows."""
        d = byte - p.start
        row = d // p.row_bytes
        col, b = divmod(d - row * p.row_bytes, p.texel)
        return int(row), int(col), int(b)

    def first_stray(self):
        """The first margin byte that is no longer what was put there: (plane, side, arena byte, (row, column, byte)) or None."""
        now = self._download()
        for p in self.order:
            for side in ("before", "after"):
                lo, hi = getattr(p, side)
                bad = np.nonzero(now[lo:hi] != self.expected[lo:hi])[0]
                if len(bad):
                    at = lo + int(bad[0])
                    return p.name, side, at, self._where(p, at), len(bad)
        return None

    def assert_margins_intact(self, what=""):
        s = self.first_stray()
        if s is not None:
            name, side, at, (row, col, b), n = s
            now = int(self._download()[at])
            raise AssertionError(f"{what}: the margin {side} plane '{name}' was written: {n} byte(s), the first at arena byte {at} = row {row}, column {col}, "
                                 f"byte {b} of that plane's grid (0x{int(self.expected[at]):02x} -> 0x{now:02x}; fill {self.fill}, {'tight' if self.tight else 'spaced'})")

    def snapshot_inputs(self, *names):
        now = self._download()
        for n in names:
            p = self.planes[n]
            self._snap[n] = now[p.start:p.end].copy()

    def first_changed_input(self):
        now = self._download()
        for n, was in self._snap.items():
            p = self.planes[n]
            bad = np.nonzero(now[p.start:p.end] != was)[0]
            if len(bad):
                at = p.start + int(bad[0])
                return n, at, self._where(p, at), len(bad)
        return None

    def assert_inputs_intact(self, what=""):
        s = self.first_changed_input()
        if s is not None:
            name, at, (row, col, b), n = s
            raise AssertionError(f"{what}: input plane '{name}' was written: {n} byte(s), the first at row {row}, column {col}, byte {b} of the texel "
                                 f"(arena byte {at}; fill {self.fill}, {'tight' if self.tight else 'spaced'})")

    def check(self, what=""):
        self.assert_margins_intact(what)
        self.assert_inputs_intact(what)
