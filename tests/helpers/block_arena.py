"""Guard-band harness for the block storage contract (include/hfmi.h, "Conventions"):

  1. rows [N, ld) of every column of a block are +0.0, always (the contractions read them unmasked);
  2. an operation writes nothing outside rows [0, N) of the columns of the blocks it is given as outputs.

An ``Arena`` is one device allocation of ``ncols`` columns of ``ld`` doubles; ``window(first, count)`` hands a run of its columns
to the library as an ``hfmi_block``.  Two kinds:

  * ``Arena.wrapped``: a ``torch.float64`` tensor filled with a quiet NaN of fixed payload, windows made by ``hfmi_block_wrap``
    (as TorchCollective._tensor_of does).  ``ld`` is free (any multiple of 32 >= N), so ``ld != round_up(N, 32)`` is reachable.  A stray
    store changes the sentinel's bits; a stray load that matters poisons the result.
  * ``Arena.in_parent``: a library-allocated block whose columns hold recognisable finite values, windows made by
    ``MultiVector.view``.  The whole allocation, padding rows included, is read back through an alias of the parent's storage.

``snapshot()`` records the bits of the whole allocation; ``check(written=[...])`` reads them again after a context synchronise and
asserts, bit for bit, that every column outside the ``written`` windows is unchanged (guards, neighbours, read-only operands) and that the
padding rows of the written windows are +0.0 (bit pattern 0: -0.0 and denormals fail).  The comparison is plain numpy
(``find_defects``) and has its own CPU test.
"""
import ctypes as C

import numpy as np

SENTINEL_BITS = np.uint64(0x7FF8DEADBEEF5A5A)      # quiet NaN, fixed payload
GUARD, PADDING, READ_ONLY = "guard", "padding", "read-only"


def round_up(n, m):
    return (int(n) + m - 1) // m * m


class Defect:
    """One violated rule: ``kind`` (GUARD: a column outside every window changed; PADDING: a row >= N of a written window is not +0.0;
    READ_ONLY: a window not declared written changed), the first offending (row, column) in column-major order (columns of the whole
    arena) and how many elements are wrong."""

    def __init__(self, kind, row, column, count, was, now):
        self.kind, self.row, self.column, self.count, self.was, self.now = kind, int(row), int(column), int(count), int(was), int(now)

    def __repr__(self):
        return "%s: %d element(s) differ, first at (row %d, column %d): bits 0x%016x -> 0x%016x" % (
            self.kind, self.count, self.row, self.column, self.was, self.now)


def _first(mask):
    c, r = np.argwhere(mask)[0]
    return int(r), int(c), int(mask.sum())


def find_defects(before, after, N, windows, written):
    """``before`` / ``after``: uint64 bit patterns of the arena, shape (ncols, ld) (one row of the array per block column).
    ``windows``: (first, count) column ranges handed to the library; ``written``: those of them the operation may store into.
    Returns the list of ``Defect``s (empty: the contract holds)."""
    before, after = np.asarray(before), np.asarray(after)
    assert before.dtype == np.uint64 and after.dtype == np.uint64 and before.shape == after.shape and before.ndim == 2
    ncols, ld = before.shape
    assert 0 < N <= ld
    windows, written = [tuple(w) for w in windows], [tuple(w) for w in written]
    assert all(w in windows for w in written), "a written window that was never handed out"
    owner = np.full(ncols, -1)
    for i, (first, count) in enumerate(windows):
        assert 0 <= first and count > 0 and first + count <= ncols, "window outside the arena"
        assert np.all(owner[first:first + count] == -1), "windows overlap"
        owner[first:first + count] = i
    changed = before != after
    out = []
    guard = changed & (owner == -1)[:, None]
    if guard.any():
        r, c, n = _first(guard)
        out.append(Defect(GUARD, r, c, n, before[c, r], after[c, r]))
    for i, (first, count) in enumerate(windows):
        sl = slice(first, first + count)
        if (first, count) in written:
            bad = after[sl, N:] != 0
            if bad.any():
                r, c, n = _first(bad)
                out.append(Defect(PADDING, r + N, c + first, n, before[c + first, r + N], after[c + first, r + N]))
        elif changed[sl].any():
            r, c, n = _first(changed[sl])
            out.append(Defect(READ_ONLY, r, c + first, n, before[c + first, r], after[c + first, r]))
    return out


def assert_contract(before, after, N, windows, written, what=""):
    defects = find_defects(before, after, N, windows, written)
    assert not defects, "block storage contract broken%s: %s" % (" by " + what if what else "", "; ".join(map(repr, defects)))


def parent_fill(N, ncols):
    """Recognisable finite values for the columns of a library-allocated parent: column c, row r holds (c + 1) * 2^20 + r + 0.5."""
    return (np.arange(1, ncols + 1, dtype=np.float64)[None, :] * 2.0 ** 20 + np.arange(N, dtype=np.float64)[:, None] + 0.5)


class Window:
    def __init__(self, arena, first, count, mv):
        self.arena, self.first, self.count, self.mv = arena, first, count, mv

    @property
    def key(self):
        return (self.first, self.count)

    def bits(self, raw=None):
        """uint64 (count, ld) rows of this window in a raw image (default: a fresh read)."""
        raw = self.arena.read() if raw is None else raw
        return raw[self.first:self.first + self.count]

    def check(self, window_changed=True, what=""):
        self.arena.check(written=[self] if window_changed else [], what=what)


class Arena:
    def __init__(self, ctx, N, ld, ncols):
        self.ctx, self.N, self.ld, self.ncols = ctx, int(N), int(ld), int(ncols)
        self.windows = []
        self._before = None

    # ---- constructors
    @classmethod
    def wrapped(cls, ctx, N, ncols, ld=None):
        """torch allocation filled with the NaN sentinel; windows through hfmi_block_wrap."""
        import torch
        ld = round_up(N, 32) if ld is None else int(ld)
        assert ld % 32 == 0 and ld >= N, "hfmi_block_wrap needs ld %% 32 == 0 and ld >= N (got ld=%d, N=%d)" % (ld, N)
        self = cls(ctx, N, ld, ncols)
        self.kind = "wrapped"
        self._t = torch.empty(self.ld * self.ncols, dtype=torch.float64, device=torch.device("cuda", ctx.device))
        self._t.view(torch.int64).fill_(int(np.uint64(SENTINEL_BITS).astype(np.int64)))
        torch.cuda.synchronize(self._t.device)
        assert self._t.data_ptr() % 128 == 0, "torch allocation is not 128-byte aligned"
        return self

    @classmethod
    def in_parent(cls, ctx, N, ncols):
        """library-allocated parent (ld = round_up(N, 32)) holding ``parent_fill``; windows through ``view``."""
        import hippyflow_amd as hf
        from hippyflow_amd import _lib as L
        parent = hf.MultiVector.from_dense(parent_fill(N, ncols), ctx=ctx)
        self = cls(ctx, N, parent.leading_dimension(), ncols)
        self.kind = "parent"
        self.parent = parent
        assert self.ld == round_up(N, 32) and parent.device_ptr() % 128 == 0
        # alias of the whole allocation as an ld x ncols block: N == ld, so the wrap zeroes nothing and a download sees the padding rows
        h = C.c_void_p()
        L.call("hfmi_block_wrap", ctx.handle, C.c_void_p(parent.device_ptr()), self.ld, self.ncols, self.ld, C.byref(h))
        self._alias = hf.MultiVector(ctx=ctx, _handle=h, _parent=parent)
        return self

    # ---- windows
    def window(self, first, count):
        import hippyflow_amd as hf
        from hippyflow_amd import _lib as L
        first, count = int(first), int(count)
        assert 0 <= first and count > 0 and first + count <= self.ncols
        assert all(first + count <= w.first or w.first + w.count <= first for w in self.windows), "windows overlap"
        if self.kind == "parent":
            mv = self.parent.view(first, count)
        else:
            p = self._t.data_ptr() + first * self.ld * 8
            assert p % 128 == 0, "window pointer is not 128-byte aligned"
            h = C.c_void_p()
            L.call("hfmi_block_wrap", self.ctx.handle, C.c_void_p(p), self.N, count, self.ld, C.byref(h))
            mv = hf.MultiVector(ctx=self.ctx, _handle=h, _parent=self._t)
            assert (mv.size(), mv.nvec(), mv.leading_dimension(), mv.device_ptr()) == (self.N, count, self.ld, p)
        w = Window(self, first, count, mv)
        self.windows.append(w)
        if self.kind == "wrapped":          # once, before any operation: the wrap zeroed the padding rows and nothing else
            raw = self.read()
            expect = np.full((self.ncols, self.ld), SENTINEL_BITS, dtype=np.uint64)
            for v in self.windows:
                expect[v.first:v.first + v.count, self.N:] = 0
            for v in self.windows[:-1]:     # earlier windows may hold data already
                expect[v.first:v.first + v.count, :self.N] = raw[v.first:v.first + v.count, :self.N]
            bad = raw != expect
            assert not bad.any(), "hfmi_block_wrap: %d element(s) wrong after the wrap, first at (row %d, column %d)" % (
                _first(bad)[2], _first(bad)[0], _first(bad)[1])
        return w

    # ---- raw image
    def read(self):
        """Bits of the whole allocation after a context synchronise: uint64 (ncols, ld)."""
        self.ctx.synchronize()
        if self.kind == "wrapped":
            import torch
            torch.cuda.synchronize(self._t.device)
            host = self._t.cpu().numpy()
        else:
            host = self._alias.to_vectors()
        return np.ascontiguousarray(host).view(np.uint64).reshape(self.ncols, self.ld)

    def snapshot(self):
        self._before = self.read()
        return self._before

    def check(self, written=(), what=""):
        assert self._before is not None, "check() without snapshot()"
        after = self.read()
        assert_contract(self._before, after, self.N, [w.key for w in self.windows], [w.key for w in written], what)
        return after
