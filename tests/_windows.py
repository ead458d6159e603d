"""Windows into larger device allocations, for tests of the C ABI's leading dimensions (test infrastructure, NumPy only).

A window is `rows x cols` elements inside an allocation of `rows_before + rows + rows_after` rows of `ld` elements; the
library is handed the pointer to element `(rows_before, col_off)` and the leading dimension `ld`.  Everything outside the
`rows x cols` block is the guard:

  output window   the whole allocation holds a reproducible pattern of finite values in which no two neighbouring elements
                  are equal; after the call every BYTE of the guard must be what it was (compared as unsigned integers, so a
                  NaN payload or the sign of a zero counts).  `rows_after` is at least 129, so the whole overhanging 128 x 128
                  tile of a wrong kernel lands inside the allocation and fails the test instead of touching foreign memory.
  input window    the guard is NaN: an over-read that reaches arithmetic poisons the result.

Layouts
  "aligned"    base pointer and col_off multiples of 16 bytes, ld a multiple of 16 / itemsize: every vector path and the
               in-place factorisation stay eligible.
  "unaligned"  col_off = 1 and ld = cols + 3 (odd when cols is even) or cols + 4: only for entries without an alignment rule.
  "block"      ld = cols, col_off = 0: operands that have no leading dimension (images, [nprob, t, c] blocks); the guard is the
               rows before and after.
"""
import ctypes as C

import numpy as np

ROWS_AFTER = 129      # a whole 128-row tile past the last row, and one more
ROWS_BEFORE = 2


def pattern(nrows, ld, dtype, seed=0):
    """Finite values, exact in fp32, no two horizontal or vertical neighbours equal: (flat index mod 1021) steps by one
    along a row, and the row's own offset (row mod 7) separates a row from the next even where ld is a multiple of 1021."""
    idx = np.arange(nrows * ld, dtype=np.int64).reshape(nrows, ld)
    row = np.arange(nrows, dtype=np.int64)[:, None]
    v = (idx + 17 * seed) % 1021 + 1021 * (row % 7)
    return (v.astype(np.float64) / 128.0 - 20.0).astype(dtype)


class Window:
    def __init__(self, rows, cols, dtype, layout="aligned", kind="out", data=None, ld=None, col_off=None,
                 rows_before=ROWS_BEFORE, rows_after=ROWS_AFTER, seed=0):
        self.dtype = np.dtype(dtype)
        self.rows, self.cols, self.kind, self.layout = int(rows), int(cols), kind, layout
        al = 16 // self.dtype.itemsize
        if layout == "aligned":
            off = al if col_off is None else col_off
            if ld is None:
                ld = (off + self.cols + al) // al * al + al
            assert off % al == 0 and ld % al == 0
        elif layout == "unaligned":
            off = 1 if col_off is None else col_off
            if ld is None:
                ld = self.cols + (3 if self.cols % 2 == 0 else 4)
        elif layout == "block":
            off, ld = 0, (self.cols if ld is None else ld)
        else:
            raise ValueError(layout)
        self.col_off, self.ld = int(off), int(ld)
        assert self.col_off + self.cols <= self.ld
        if kind == "out":
            assert rows_after >= ROWS_AFTER, "an overhanging 128-row tile must land inside the allocation"
        self.rows_before, self.rows_after = int(rows_before), int(rows_after)
        self.nrows = self.rows_before + self.rows + self.rows_after
        if kind == "out":
            self.host0 = pattern(self.nrows, self.ld, self.dtype, seed)
        elif kind == "in":
            self.host0 = np.full((self.nrows, self.ld), np.nan, dtype=self.dtype)
        else:
            raise ValueError(kind)
        if data is not None:
            data = np.asarray(data, dtype=self.dtype).reshape(self.rows, self.cols)
            self.inside(self.host0)[...] = data
        self.dev = None

    # ---- host side
    def inside(self, full=None):
        """The rows x cols block of a whole-allocation array (a view)."""
        full = self.host0 if full is None else full
        return full[self.rows_before:self.rows_before + self.rows, self.col_off:self.col_off + self.cols]

    def initial(self):
        """What the window holds before the call, as an exactly sized contiguous array: the twin buffer of the contiguous call."""
        return np.ascontiguousarray(self.inside())

    def first_damage(self, after):
        """None, or (row, col) of the first changed guard element, relative to the window's element (0, 0)."""
        after = np.ascontiguousarray(after)
        assert after.shape == self.host0.shape and after.dtype == self.dtype
        isz = self.dtype.itemsize
        b0 = self.host0.view(np.uint8).reshape(self.nrows, self.ld, isz)
        b1 = after.view(np.uint8).reshape(self.nrows, self.ld, isz)
        bad = (b0 != b1).any(axis=2)
        self.inside(bad)[...] = False
        hit = np.flatnonzero(bad)
        if hit.size == 0:
            return None
        r, c = divmod(int(hit[0]), self.ld)
        return (r - self.rows_before, c - self.col_off)

    def assert_guard_untouched(self, after=None, what="window"):
        after = self.download() if after is None else after
        hit = self.first_damage(after)
        assert hit is None, "%s: guard damaged, first at (row %d, col %d) relative to the %d x %d window (ld %d, col_off %d)" % (
            what, hit[0], hit[1], self.rows, self.cols, self.ld, self.col_off)
        return after

    # ---- device side
    def upload(self, ctx):
        self.ctx = ctx
        self.dev = ctx.to_device(self.host0)
        return self

    @property
    def ptr(self):
        return C.c_void_p(self.dev.ptr.value + (self.rows_before * self.ld + self.col_off) * self.dtype.itemsize)

    def download(self):
        return self.dev.raw_numpy()

    def result(self, what="window"):
        """Download, check the guard, return the rows x cols block."""
        after = self.assert_guard_untouched(what=what)
        return np.ascontiguousarray(self.inside(after))


def out_window(ctx, rows, cols, dtype, layout="aligned", **kw):
    return Window(rows, cols, dtype, layout, "out", **kw).upload(ctx)


def in_window(ctx, data, layout="aligned", **kw):
    data = np.asarray(data)
    if data.ndim == 1:
        data = data[None, :]
    kw.setdefault("rows_after", ROWS_BEFORE)
    return Window(data.shape[0], data.shape[1], data.dtype, layout, "in", data=data, **kw).upload(ctx)
