"""GPU suite: the block storage contract (include/hfmi.h, "Conventions") under every public operation that stores into a block.

  1. rows [N, ld) of every column stay +0.0;   2. nothing outside rows [0, N) of the output's own columns is written.

Every entry of ``WRITERS`` runs on guard-banded operands (tests/helpers/block_arena.py): windows wrapped over a torch allocation full
of NaN sentinels with ld = round_up(N, 32), + 32 and + 96; a ``view`` in the middle of a library-allocated parent; and all block
operands as different views of ONE parent.  Besides the guard check each entry checks its result: element-wise operations, transfers
and the Philox draw bit for bit against the same call on a fresh block; contractions and operator applications on small integers
(uniform in [-8, 8], so every partial sum is an integer below 2^53 and any summation order is exact) against the int64 numpy product,
exactly; solves, QR and eigensolvers against the same call on standalone blocks at the tolerance of the operation's existing test.

tests/test_block_contract_table_cpu.py checks on the CPU that every prototype of hfmi.h with a mutable block is named here.
Building the table touches no GPU: it holds callables.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import block_arena as ba  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ["wrap_ld0", "wrap_ld32", "wrap_ld96", "view", "shared"]
GUARD_COLS = 2

# N % 32 in {0, 1, 2, 3, 31}, N < 32, 4225 (the project's mesh), N > 65536; nvec in {1, 5, 16, 17, 74, 138}: every N and every nvec
# appears, the pairs cycle
N_LIST = [1, 3, 31, 32, 33, 34, 35, 63, 4225, 65539, 131072]
K_LIST = [1, 5, 16, 17, 74, 138]
SHAPES = [(N, K_LIST[i % len(K_LIST)]) for i, N in enumerate(N_LIST)] + [(33, 138), (4225, 16), (35, 1), (34, 17)]
SMALL_SHAPES = [s for s in SHAPES if s[0] <= 4225]


def _hf():
    import hippyflow_amd as hf
    return hf


def _L():
    from hippyflow_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def ctx():
    hf = _hf()
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


class Env:
    """Hands out arena-backed operands in one of MODES and checks all arenas at once."""

    def __init__(self, ctx, mode):
        self.ctx, self.mode, self.arenas = ctx, mode, []

    def blocks(self, N, *nvecs):
        """One window of N rows per entry of nvecs.  'shared': all of them views of one parent, two columns apart."""
        out = []
        if self.mode == "shared":
            a = ba.Arena.in_parent(self.ctx, N, sum(nvecs) + GUARD_COLS * (len(nvecs) + 1))
            self.arenas.append(a)
            first = GUARD_COLS
            for k in nvecs:
                out.append(a.window(first, k))
                first += k + GUARD_COLS
            return out
        for k in nvecs:
            if self.mode == "view":
                a = ba.Arena.in_parent(self.ctx, N, k + 3 + GUARD_COLS)
                w = a.window(3, k)
            else:
                extra = {"wrap_ld0": 0, "wrap_ld32": 32, "wrap_ld96": 96}[self.mode]
                a = ba.Arena.wrapped(self.ctx, N, k + 2 * GUARD_COLS, ld=ba.round_up(N, 32) + extra)
                w = a.window(GUARD_COLS, k)
            self.arenas.append(a)
            out.append(w)
        return out

    def block(self, N, k, data=None):
        (w,) = self.blocks(N, k)
        if data is not None:
            put(w, data)
        return w

    def snapshot(self):
        for a in self.arenas:
            a.snapshot()

    def check(self, written=(), what=""):
        for a in self.arenas:
            a.check(written=[w for w in written if w.arena is a], what="%s [%s]" % (what, self.mode))


def put(w, dense):
    L = _L()
    dense = L.as_f64(dense)
    assert dense.shape == (w.mv.size(), w.mv.nvec())
    L.call("hfmi_block_upload", w.mv.handle, L.ptr(dense), L.LAYOUT_DENSE)


def ints(rng, *shape):
    return rng.integers(-8, 9, size=shape).astype(np.float64)


def exact(got, want_int):
    """integer-valued result == int64 reference, exactly"""
    want = np.asarray(want_int)
    assert want.dtype == np.int64 and np.abs(want).max(initial=0) < 2 ** 53
    bad = got != want.astype(np.float64)
    assert not bad.any(), "%d wrong element(s), first at %s: got %r, expected %r" % (
        bad.sum(), tuple(np.argwhere(bad)[0]), got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


def i64(a):
    return np.asarray(a).astype(np.int64)


def iprod(a, b):
    """int64 product of integer-valued arrays.  Every partial sum is an integer below 2^53 (asserted from the operands), so the fp64
    product is exact in any summation order and BLAS may compute it; sparse operands go through scipy's integer product."""
    import scipy.sparse as sp
    if sp.issparse(a):
        return np.asarray(a.astype(np.int64) @ i64(b))
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(a, np.rint(a)) and np.array_equal(b, np.rint(b))
    assert np.abs(a).max(initial=0) * np.abs(b).max(initial=0) * a.shape[-1] < 2.0 ** 53
    return i64(a @ b)


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def rng_for(*key):
    return np.random.default_rng(abs(hash(tuple(int(k) for k in key))) % (2 ** 32))


# ====================================================================== element-wise
def w_create(env, N, k):
    """hfmi_block_create: zero-filled, padding rows included (read through an alias of the whole allocation)."""
    hf, L = _hf(), _L()
    mv = hf.MultiVector(N, k, ctx=env.ctx)
    ld = mv.leading_dimension()
    assert ld == ba.round_up(N, 32)
    h = C.c_void_p()
    L.call("hfmi_block_wrap", env.ctx.handle, C.c_void_p(mv.device_ptr()), ld, k, ld, C.byref(h))
    alias = hf.MultiVector(ctx=env.ctx, _handle=h, _parent=mv)
    assert not alias.to_vectors().view(np.uint64).any()


def w_wrap(env, N, k):
    """hfmi_block_wrap zeroes rows [N, ld) of its columns and nothing else (Arena.window asserts it), and refuses what it must."""
    hf, L = _hf(), _L()
    w = env.block(N, k)
    raw = w.bits()
    assert not raw[:, N:].any()
    if w.arena.kind == "wrapped":
        assert np.all(raw[:, :N] == ba.SENTINEL_BITS)
    p, ld = w.mv.device_ptr(), w.mv.leading_dimension()
    for args in ((p + 8, N, k, ld), (p, N, k, ld + 8), (p, ld + 1, k, ld)):
        with pytest.raises(hf.HfmiError):
            L.call("hfmi_block_wrap", env.ctx.handle, C.c_void_p(args[0]), args[1], args[2], args[3], C.byref(C.c_void_p()))


def _elementwise(env, N, k, n_in, op, fresh_op, what):
    """Y (written) and n_in read-only inputs, Gaussian data; the window result equals the same call on fresh blocks, bit for bit."""
    hf = _hf()
    rng = rng_for(N, k, n_in)
    ws = env.blocks(N, *([k] * (1 + n_in)))
    data = [rng.standard_normal((N, k)) for _ in ws]
    for w, d in zip(ws, data):
        put(w, d)
    env.snapshot()
    op(*[w.mv for w in ws])
    env.check(written=[ws[0]], what=what)
    fresh = [hf.MultiVector.from_dense(d, ctx=env.ctx) for d in data]
    fresh_op(*fresh)
    assert np.array_equal(ws[0].mv.to_dense(), fresh[0].to_dense(), equal_nan=True)
    return ws, data


def w_zero(env, N, k):
    ws, _ = _elementwise(env, N, k, 0, lambda y: y.zero(), lambda y: y.zero(), "hfmi_block_zero")
    assert not ws[0].bits()[:, :N].any()


def w_scale(env, N, k):
    _elementwise(env, N, k, 0, lambda y: y.scale(-1.7), lambda y: y.scale(-1.7), "hfmi_block_scale")


def w_axpy(env, N, k):
    _elementwise(env, N, k, 1, lambda y, x: y.axpy(0.37, x), lambda y, x: y.axpy(0.37, x), "hfmi_block_axpy")


def w_copy(env, N, k):
    ws, data = _elementwise(env, N, k, 1, lambda y, x: y.copy_from(x), lambda y, x: y.copy_from(x), "hfmi_block_copy")
    assert np.array_equal(ws[0].mv.to_dense(), data[1])


def w_copy_across_ld(env, N, k):
    """copy between a window and a standalone block: the two leading dimensions differ in the ld+32 / ld+96 forms"""
    hf = _hf()
    rng = rng_for(N, k, 9)
    a, b = rng.standard_normal((N, k)), rng.standard_normal((N, k))
    w = env.block(N, k, a)
    s = hf.MultiVector.from_dense(b, ctx=env.ctx)
    t = hf.MultiVector(N, k, ctx=env.ctx)
    env.snapshot()
    t.copy_from(w.mv)
    env.check(written=[], what="hfmi_block_copy from a window")
    assert np.array_equal(t.to_dense(), a)
    w.mv.copy_from(s)
    env.check(written=[w], what="hfmi_block_copy into a window")
    assert np.array_equal(w.mv.to_dense(), b)


def w_swap(env, N, k):
    """MultiVector.swap exchanges storage: a write through the first name lands in the second window, and only there."""
    rng = rng_for(N, k, 2)
    a, b = env.blocks(N, k, k)
    da, db = rng.standard_normal((N, k)), rng.standard_normal((N, k))
    put(a, da)
    put(b, db)
    env.snapshot()
    a.mv.swap(b.mv)
    env.check(written=[], what="MultiVector.swap")
    assert np.array_equal(a.mv.to_dense(), db) and np.array_equal(b.mv.to_dense(), da)
    a.mv.scale(2.0)                      # a.mv now names b's columns
    env.check(written=[b], what="scale after MultiVector.swap")
    assert np.array_equal(a.mv.to_dense(), 2.0 * db) and np.array_equal(b.mv.to_dense(), da)
    a.mv.swap(b.mv)                      # handles back to their windows before they are destroyed


def w_randn(env, N, k):
    """hfmi_randn_fill.  launch_randn takes its 32-byte-vector kernel when the pointer is 32-byte aligned and ld % 4 == 0: with
    ld % 32 == 0 and 128-byte aligned columns enforced by create / wrap / view, that is every block the C ABI can make -- the scalar
    kernel is unreachable from outside and cannot be given a case."""
    hf, L = _hf(), _L()
    w = env.block(N, k, np.ones((N, k)))
    env.snapshot()
    L.call("hfmi_randn_fill", w.mv.handle, 12345, 7, 1.5)
    env.check(written=[w], what="hfmi_randn_fill")
    fresh = hf.MultiVector(N, k, ctx=env.ctx)
    L.call("hfmi_randn_fill", fresh.handle, 12345, 7, 1.5)
    got = w.mv.to_dense()
    assert np.array_equal(got, fresh.to_dense()) and np.all(np.isfinite(got))
    L.call("hfmi_randn_fill", w.mv.handle, 12345, 7, 0.0)          # sigma == 0: the fill kernel
    env.check(written=[w], what="hfmi_randn_fill sigma=0")
    assert not w.bits()[:, :N].any()


def w_matern(env, N, k):
    """hfmi_block_fill_matern32 needs a square block: N vectors of length N (k is ignored)."""
    hf, L = _hf(), _L()
    if N > 1100:
        N = 1025
    nx = max(2, int(np.ceil(np.sqrt(N))))
    w = env.block(N, N, np.ones((N, N)))
    env.snapshot()
    L.call("hfmi_block_fill_matern32", w.mv.handle, nx, nx + 1, 1.3, 0.2)
    env.check(written=[w], what="hfmi_block_fill_matern32")
    fresh = hf.MultiVector(N, N, ctx=env.ctx)
    L.call("hfmi_block_fill_matern32", fresh.handle, nx, nx + 1, 1.3, 0.2)
    got = w.mv.to_dense()
    assert np.array_equal(got, fresh.to_dense())
    np.testing.assert_allclose(np.diag(got), 1.3 ** 2, rtol=1e-15)
    np.testing.assert_allclose(got, got.T, rtol=1e-13)


# ====================================================================== transfers
def w_upload(env, N, k):
    L = _L()
    rng = rng_for(N, k, 3)
    w = env.block(N, k)
    for layout, host in ((L.LAYOUT_DENSE, rng.standard_normal((N, k))), (L.LAYOUT_VECTORS, rng.standard_normal((k, N)))):
        env.snapshot()
        L.call("hfmi_block_upload", w.mv.handle, L.ptr(host), layout)
        env.check(written=[w], what="hfmi_block_upload layout %d" % layout)
        cols = host if layout == L.LAYOUT_DENSE else host.T
        assert np.array_equal(w.bits()[:, :N], np.ascontiguousarray(cols.T).view(np.uint64))


def w_upload_async(env, N, k):
    """hfmi_block_upload_async from pinned memory, whole window and views of one item each.  The second half RESTATES the loop of
    multivector.ingest_stream against views of the window, because ingest_stream itself allocates its block and cannot be handed
    one: if that loop changes, this copy does not follow it (w_ingest_stream runs the real function, without neighbours)."""
    L = _L()
    rng = rng_for(N, k, 4)
    w = env.block(N, k)
    for layout in ("vectors", "dense"):
        buf = L.pinned_empty((k, N) if layout == "vectors" else (N, k))
        buf[...] = rng.standard_normal(buf.shape)
        env.snapshot()
        env.ctx.ingest_wait(w.mv.upload_async(buf, layout=layout))
        env.ctx.ingest_fence()
        env.check(written=[w], what="hfmi_block_upload_async %s" % layout)
        assert np.array_equal(w.mv.to_dense(), buf.T if layout == "vectors" else buf)
    per = 2 if k % 2 == 0 and k > 1 else 1
    items = rng.standard_normal((k // per, per, N))
    bufs = [L.pinned_empty((per, N)) for _ in range(2)]
    tickets = [None, None]
    env.snapshot()
    for i in range(k // per):                                       # the loop of multivector.ingest_stream, into views of the window
        b = i % 2
        if tickets[b] is not None:
            env.ctx.ingest_wait(tickets[b])
        np.copyto(bufs[b], items[i])
        tickets[b] = w.mv.view(i * per, per).upload_async(bufs[b])
    for t in tickets:
        if t is not None:
            env.ctx.ingest_wait(t)
    env.ctx.ingest_fence()
    env.check(written=[w], what="upload_async into views")
    assert np.array_equal(w.mv.to_vectors(), items.reshape(k, N))


def w_ingest_stream(env, N, k):
    """The real multivector.ingest_stream.  It allocates its own block, so there are no neighbour columns to protect: result and
    padding rows (through an alias of the allocation).  Its loop on views that HAVE neighbours is restated in w_upload_async."""
    hf, L = _hf(), _L()
    rng = rng_for(N, k, 5)
    items = rng.standard_normal((k, 1, N))
    blk = hf.ingest_stream(iter(items), k, 1, N, ctx=env.ctx)
    assert np.array_equal(blk.to_vectors(), items.reshape(k, N))
    ld = blk.leading_dimension()
    h = C.c_void_p()
    L.call("hfmi_block_wrap", env.ctx.handle, C.c_void_p(blk.device_ptr()), ld, k, ld, C.byref(h))
    alias = hf.MultiVector(ctx=env.ctx, _handle=h, _parent=blk)
    assert not alias.to_vectors().view(np.uint64)[:, N:].any()


def w_download(env, N, k):
    """hfmi_block_download of a window returns exactly the window and writes nothing on the device."""
    rng = rng_for(N, k, 6)
    data = rng.standard_normal((N, k))
    w = env.block(N, k, data)
    env.snapshot()
    d, v = w.mv.to_dense(), w.mv.to_vectors()
    env.check(written=[], what="hfmi_block_download")
    assert d.shape == (N, k) and v.shape == (k, N) and np.array_equal(d, data) and np.array_equal(v, data.T)


# ====================================================================== contractions
def _gemm_small(env, N, m, r, entry="hfmi_block_gemm_small"):
    L = _L()
    rng = rng_for(N, m, r)
    A, S, Y0 = ints(rng, N, m), ints(rng, m, r), ints(rng, N, r)
    a, y = env.blocks(N, m, r)
    put(a, A)
    put(y, Y0)
    ref = iprod(A, S)
    env.snapshot()
    if entry == "hfmi_bench_tsgemm_nn":
        ms = C.c_double(0)
        L.call(entry, a.mv.handle, L.ptr(S), y.mv.handle, 1, C.byref(ms))
        env.check(written=[y], what=entry)
        exact(y.mv.to_dense(), ref)
        return
    L.call(entry, a.mv.handle, L.ptr(S), 1.0, 0.0, y.mv.handle)                 # beta = 0: MvDSmatMult
    env.check(written=[y], what="gemm_small beta=0 N=%d m=%d r=%d" % (N, m, r))
    exact(y.mv.to_dense(), ref)
    put(y, Y0)
    L.call(entry, a.mv.handle, L.ptr(S), 2.0, -3.0, y.mv.handle)                # beta != 0
    env.check(written=[y], what="gemm_small beta=-3 N=%d m=%d r=%d" % (N, m, r))
    exact(y.mv.to_dense(), 2 * ref - 3 * i64(Y0))


def w_gemm_small(env, N, k):
    _gemm_small(env, N, k, K_LIST[(K_LIST.index(k) + 2) % len(K_LIST)])


def w_bench_tsgemm_nn(env, N, k):
    _gemm_small(env, N, k, K_LIST[(K_LIST.index(k) + 1) % len(K_LIST)], entry="hfmi_bench_tsgemm_nn")


def w_reduce(env, N, k):
    """MultiVector.reduce: y += sum_i alpha_i A_i into ONE column of a window (a Vector of the window): the other columns are guards."""
    hf = _hf()
    rng = rng_for(N, k, 8)
    A, Y0, alpha = ints(rng, N, k), ints(rng, N, 3), ints(rng, k)
    a, y = env.blocks(N, k, 3)
    put(a, A)
    put(y, Y0)
    env.snapshot()
    a.mv.reduce(y.mv[1], alpha)
    env.check(written=[y], what="MultiVector.reduce")
    want = i64(Y0)
    want[:, 1] += iprod(A, alpha)
    exact(y.mv.to_dense(), want)


def _dot(env, N, m, k, nsplits=()):
    """hfmi_block_dot (A^T B and the Gram form A^T A) and hfmi_block_norms on read-only windows; ``nsplits``: also the same product
    through hfmi_bench_tsgemm_tn with these explicit split counts (> 1: partial sums + launch_reduce_partials, whatever the library's
    own plan would pick)."""
    L = _L()
    rng = rng_for(N, m, k, 1)
    A, B = ints(rng, N, m), ints(rng, N, k)
    a, b = env.blocks(N, m, k)
    put(a, A)
    put(b, B)
    env.snapshot()
    got = a.mv.dot_mv(b.mv)
    gram = a.mv.dot_mv(a.mv)
    norms = a.mv.norm()
    forced = []
    for ns in nsplits:
        out = np.empty((m, k))
        L.call("hfmi_bench_tsgemm_tn", a.mv.handle, b.mv.handle, int(ns), 0, L.ptr(out), None)
        forced.append(out)
    env.check(written=[], what="hfmi_block_dot / hfmi_block_norms N=%d m=%d k=%d" % (N, m, k))
    for out in forced:
        exact(out, iprod(A.T, B))
    exact(got, iprod(A.T, B))
    exact(gram, iprod(A.T, A))
    assert np.array_equal(norms, np.sqrt(np.sum(i64(A) ** 2, axis=0).astype(np.float64)))   # sqrt of an exact integer, correctly rounded


def w_dot_norms(env, N, k):
    _dot(env, N, K_LIST[(K_LIST.index(k) + 3) % len(K_LIST)], k)


def w_gram_eig(env, N, k):
    """hfmi_block_gram_eig with window inputs (read-only): the assertions of test_gram_eig_of_two_blocks_stays_on_the_device."""
    rng = rng_for(N, k, 11)
    n = k
    X = rng.standard_normal((N, min(n, 60))) @ (rng.standard_normal((min(n, 60), n)) * np.exp(-0.1 * np.arange(min(n, 60)))[:, None])
    wgt = rng.uniform(0.5, 2.0, N)
    a, b = env.blocks(N, n, n)
    put(a, X)
    put(b, X * wgt[:, None])
    env.snapshot()
    d, V = a.mv.gram_eig(b.mv, n)
    env.check(written=[], what="hfmi_block_gram_eig")
    G = X.T @ (X * wgt[:, None])
    wr = np.linalg.eigvalsh(G)[::-1]
    assert np.abs(d - wr).max() <= 1e-12 * wr[0]
    lead = min(n, 40)
    assert np.abs(G @ V[:, :lead] - V[:, :lead] * d[:lead]).max() <= 2e-12 * wr[0]
    assert np.abs(V[:, :lead].T @ V[:, :lead] - np.eye(lead)).max() <= 1e-12


# ====================================================================== operators (hfmi_op_apply, accumulate 0 and 1)
def _apply(env, op, w, y, W, Y0, ref, what):
    """Y = op(W), then Y += op(W): W read-only, Y written, both exact."""
    put(w, W)
    put(y, Y0)
    env.snapshot()
    op.matMvMult(w.mv, y.mv)
    env.check(written=[y], what=what + " accumulate=0")
    exact(y.mv.to_dense(), ref)
    put(y, Y0)
    op.matMvMult(w.mv, y.mv, accumulate=True)
    env.check(written=[y], what=what + " accumulate=1")
    exact(y.mv.to_dense(), ref + i64(Y0))


def _band(N, rng):
    """integer band matrix, 5 diagonals: regular rows -> the ELL kernel"""
    import scipy.sparse as sp
    offs = [o for o in (-2, -1, 0, 1, 2) if abs(o) < N]
    return sp.diags([ints(rng, N - abs(o)) for o in offs], offs, format="csr")


def _irregular(N, rng):
    """one dense row, empty rows (the matrix of test_csr_irregular_rows_use_the_csr_kernel, in integers): no ELL image"""
    import scipy.sparse as sp
    R = sp.random(N, N, density=min(1.0, 6.0 / N), random_state=3, format="lil", data_rvs=lambda n: ints(rng, n))
    R[min(7, N - 1), :] = ints(rng, N)
    if N > 11:
        R[11, :] = 0.0
        R[N - 1, :] = 0.0
    return R.tocsr()


def _csr_case(env, N, k, make, what):
    hf = _hf()
    rng = rng_for(N, k, len(what))
    M = make(N, rng)
    w, y = env.blocks(N, k, k)
    W, Y0 = ints(rng, N, k), ints(rng, N, k)
    ref = iprod(M, W)
    _apply(env, hf.CsrOperator(M, ctx=env.ctx), w, y, W, Y0, ref, what)


def w_csr_ell(env, N, k):
    _csr_case(env, N, k, _band, "hfmi_op_csr (ELL)")


def w_csr_irregular(env, N, k):
    _csr_case(env, N, k, _irregular, "hfmi_op_csr (k_csr_spmm)")


def w_dense_sym(env, N, k):
    hf = _hf()
    if N > 1100:
        N = 1025
    rng = rng_for(N, k, 21)
    Cm = np.triu(ints(rng, N, N))
    Cm = Cm + np.triu(Cm, 1).T
    c, w, y = env.blocks(N, N, k, k)
    put(c, Cm)
    W, Y0 = ints(rng, N, k), ints(rng, N, k)
    _apply(env, hf.npToDeviceOperator(c.mv), w, y, W, Y0, iprod(Cm, W), "hfmi_op_dense_sym")


def w_snapshot_gram(env, N, k):
    hf = _hf()
    rng = rng_for(N, k, 22)
    n = K_LIST[(K_LIST.index(k) + 1) % len(K_LIST)]
    X, W, Y0 = ints(rng, N, n), ints(rng, N, k), ints(rng, N, k)
    x, w, y = env.blocks(N, n, k, k)
    put(x, X)
    _apply(env, hf.SnapshotGramOperator(x.mv, scale=1.0), w, y, W, Y0, iprod(X, iprod(X.T, W)), "hfmi_op_snapshot_gram")


def w_low_rank(env, N, k):
    hf = _hf()
    rng = rng_for(N, k, 23)
    n = K_LIST[(K_LIST.index(k) + 4) % len(K_LIST)]
    U, d, W, Y0 = ints(rng, N, n), ints(rng, n), ints(rng, N, k), ints(rng, N, k)
    u, w, y = env.blocks(N, n, k, k)
    put(u, U)
    _apply(env, hf.LowRankOperator(d, u.mv), w, y, W, Y0, iprod(U * d[None, :], iprod(U.T, W)), "hfmi_op_low_rank")


def w_jtj(env, N, k):
    """mean J^T Gamma^-1 J with the noise precision (scale 1: integers stay integers)"""
    hf = _hf()
    rng = rng_for(N, k, 24)
    ndata, q = 3, 5
    J, W, Y0 = ints(rng, N, ndata * q), ints(rng, N, k), ints(rng, N, k)
    G = ints(rng, q, q)
    G = G + G.T
    j, w, y = env.blocks(N, ndata * q, k, k)
    put(j, J)
    Ji = J.reshape(N, ndata, q)
    ref = sum(iprod(Ji[:, i], iprod(G, iprod(Ji[:, i].T, W))) for i in range(ndata))
    op = hf.MeanJTJfromDataOperator.from_block(j.mv, ndata, q, noise_cov_inv=G, scale=1.0)
    _apply(env, op, w, y, W, Y0, ref, "hfmi_op_jtj")


def w_jjt(env, N, k):
    """mean J J^T acts on blocks of length q: W and Y are q-row windows, J an N-row window (read-only).  hfmi_op_jjt takes no noise
    precision (only hfmi_op_jtj does: w_jtj)."""
    hf = _hf()
    rng = rng_for(N, k, 25)
    ndata, q = 3, 33
    J, W, Y0 = ints(rng, N, ndata * q), ints(rng, q, k), ints(rng, q, k)
    j = env.block(N, ndata * q, J)
    w, y = env.blocks(q, k, k)
    Ji = J.reshape(N, ndata, q)
    ref = sum(iprod(Ji[:, i].T, iprod(Ji[:, i], W)) for i in range(ndata))
    _apply(env, hf.MeanJJTfromDataOperator((j.mv, ndata, q), scale=1.0), w, y, W, Y0, ref, "hfmi_op_jjt")


def w_compose3(env, N, k):
    """c(b(a W)) and the nested form compose3(compose3(a, b, c), a, b): the intermediates are the library's own blocks"""
    hf = _hf()
    rng = rng_for(N, k, 26)
    Ms = [_band(N, rng) for _ in range(3)]
    a, b, c = [hf.CsrOperator(M, ctx=env.ctx) for M in Ms]
    w, y = env.blocks(N, k, k)
    W, Y0 = ints(rng, N, k), ints(rng, N, k)
    abc = hf.ComposedOperator(a, b, c)
    _apply(env, abc, w, y, W, Y0, iprod(Ms[2], iprod(Ms[1], iprod(Ms[0], W))), "hfmi_op_compose3")
    nested = hf.ComposedOperator(abc, a, b)
    _apply(env, nested, w, y, W, Y0, iprod(Ms[1], iprod(Ms[0], iprod(Ms[2], iprod(Ms[1], iprod(Ms[0], W))))), "hfmi_op_compose3 nested")


def w_host_callback(env, N, k):
    hf = _hf()
    rng = rng_for(N, k, 27)
    M = _band(N, rng)
    w, y = env.blocks(N, k, k)
    W, Y0 = ints(rng, N, k), ints(rng, N, k)
    ref = iprod(M, W)
    _apply(env, hf.HostCallbackOperator(lambda X: M @ X, N=N, ctx=env.ctx), w, y, W, Y0, ref, "hfmi_op_host_callback")
    _apply(env, hf.HostCallbackOperator(lambda X: M @ X, N=N, ctx=env.ctx, chunk_vectors=4), w, y, W, Y0, ref,
           "hfmi_op_host_callback chunked")


def _fem(N):
    import scipy.sparse as sp
    h = 1.0 / (N - 1)
    main = np.full(N, 4 * h / 6)
    main[[0, -1]] = 2 * h / 6
    M = sp.diags([np.full(N - 1, h / 6), main, np.full(N - 1, h / 6)], [-1, 0, 1], format="csr")
    kd = np.full(N, 2 / h)
    kd[[0, -1]] = 1 / h
    K = sp.diags([np.full(N - 1, -1 / h), kd, np.full(N - 1, -1 / h)], [-1, 0, 1], format="csr")
    return M, K


def _solve_case(env, S, N, k, tol, what, method=None):
    """window solve == the same solve on standalone blocks, at the tolerance of the operation's existing test"""
    hf = _hf()
    rng = rng_for(N, k, 31)
    B = rng.standard_normal((N, k))
    w, y = env.blocks(N, k, k)
    put(w, B)
    put(y, np.ones((N, k)))
    env.snapshot()
    S.matMvMult(w.mv, y.mv)
    env.check(written=[y], what=what)
    if method is not None:
        assert S.info()["method"] == method
    Ys = hf.MultiVector(N, k, ctx=env.ctx)
    S.matMvMult(hf.MultiVector.from_dense(B, ctx=env.ctx), Ys)
    assert rel(y.mv.to_dense(), Ys.to_dense()) <= tol
    return B, y


def w_csr_pcg(env, N, k):
    """hfmi_op_csr_pcg: a mass matrix goes the Chebyshev route (1e-11 against the direct solve in
    test_sparse_solver_chebyshev_and_cg_routes), a stiffness-dominated one the block CG (residual 1e-10 there)."""
    hf = _hf()
    N = max(N, 50)
    M, K = _fem(N)
    B, y = _solve_case(env, hf.CsrPCGSolver(M, rel_tol=1e-13, ctx=env.ctx), N, k, 1e-11, "hfmi_op_csr_pcg (Chebyshev)", "chebyshev")
    res = M @ y.mv.to_dense() - B
    assert np.all(np.linalg.norm(res, axis=0) <= 2e-13 * np.linalg.norm(B, axis=0))
    stiff = (M + 1e-4 * K).tocsr()
    # the bracket of D^-1 (M + 1e-4 K) widens like 1 + 1.2e-3 / h^2: too wide for Chebyshev on the meshes of a few thousand nodes, where
    # the CG route is asserted; on the 63-node mesh the library may serve it either way and only the result is checked
    route = "cg" if N >= 2000 else None
    B, y = _solve_case(env, hf.CsrPCGSolver(stiff, rel_tol=1e-12, max_iter=4000, ctx=env.ctx), N, k, 1e-10, "hfmi_op_csr_pcg (CG)", route)
    res = stiff @ y.mv.to_dense() - B
    assert np.all(np.linalg.norm(res, axis=0) <= 1e-10 * np.linalg.norm(B, axis=0))


_AMG = {}


def _amg(ctx, nx):
    from hippyflow_amd import workloads
    if nx not in _AMG:
        A = (workloads.grid_mass_matrix(nx, nx) + 0.1 * workloads.grid_stiffness_matrix(nx, nx)).tocsr()
        _AMG[nx] = (A, _hf().CsrAMGSolver(A, rel_tol=1e-12, ctx=ctx))
    return _AMG[nx]


def w_amg_pcg(env, nx, k):
    """hfmi_op_amg_pcg: residual 1e-12 and 1e-9 against the direct solve in test_amg_solver_accuracy_and_iterations"""
    A, S = _amg(env.ctx, nx)
    B, y = _solve_case(env, S, A.shape[0], k, 1e-9, "hfmi_op_amg_pcg", "amg-cg")
    res = np.linalg.norm(B - A @ y.mv.to_dense(), axis=0) / np.linalg.norm(B, axis=0)
    assert res.max() <= 1e-12


def w_amg_vcycle(env, nx, k):
    """hfmi_amg_vcycle: 1e-12 against the CPU twin in test_device_vcycle_equals_cpu_twin"""
    hf = _hf()
    A, S = _amg(env.ctx, nx)
    N = A.shape[0]
    B = rng_for(N, k, 32).standard_normal((N, k))
    b, x = env.blocks(N, k, k)
    put(b, B)
    put(x, np.ones((N, k)))
    env.snapshot()
    S.vcycle(b.mv, x.mv)
    env.check(written=[x], what="hfmi_amg_vcycle")
    Xs = hf.MultiVector(N, k, ctx=env.ctx)
    S.vcycle(hf.MultiVector.from_dense(B, ctx=env.ctx), Xs)
    assert rel(x.mv.to_dense(), Xs.to_dense()) <= 1e-12


def w_amg_pcg_error(env, nx, k):
    """include/hfmi.h: 'Y is zero-filled on error' (hfmi_op_amg_pcg; the only entry point whose header says so).  A NaN in the
    right-hand side is HFMI_ERR_NUMERIC: error raised, window all zero, guards and padding intact, input untouched."""
    hf = _hf()
    A, S = _amg(env.ctx, nx)
    N = A.shape[0]
    B = rng_for(N, k, 33).standard_normal((N, k))
    B[N // 2, k // 2] = np.nan
    w, y = env.blocks(N, k, k)
    put(w, B)
    put(y, np.ones((N, k)))
    env.snapshot()
    with pytest.raises(hf.HfmiError) as e:
        S.matMvMult(w.mv, y.mv)
    assert e.value.code == -4, e.value
    env.check(written=[y], what="hfmi_op_amg_pcg on a NaN right-hand side")
    assert not y.bits().any(), "Y is not zero-filled after the error"


# ====================================================================== factorisations
def _graded(rng, N, k, decades):
    return rng.standard_normal((N, k)) @ np.diag(np.logspace(0, -decades, k)) @ np.linalg.qr(rng.standard_normal((k, k)))[0]


def w_orthogonalize(env, N, k):
    """hfmi_borth_qr, B = NULL, methods chol and mgs: the assertions of test_orthogonalize_matches_reference_mgs, and the window
    result against the same call on a standalone block"""
    hf, L = _hf(), _L()
    Z = _graded(rng_for(N, k, 41), N, k, 3)
    for method in (L.QR_CHOL, L.QR_MGS):
        q = env.block(N, k, Z)
        env.snapshot()
        R = q.mv.orthogonalize(method)
        env.check(written=[q], what="hfmi_borth_qr method %d" % method)
        Qd = q.mv.to_dense()
        assert np.linalg.norm(Qd.T @ Qd - np.eye(k)) / np.sqrt(k) < 1e-13
        assert np.allclose(np.tril(R, -1), 0) and np.all(np.diag(R) > 0)
        assert rel(Qd @ R, Z) < 1e-12
        Qs = hf.MultiVector.from_dense(Z, ctx=env.ctx)
        Rs = Qs.orthogonalize(method)
        assert np.abs(Qd - Qs.to_dense()).max() < 1e-12 and rel(R, Rs) < 1e-12


def w_orthogonalize_rank_deficient(env, N, k):
    """a dependent column: Cholesky breaks down, the shifted retry runs and AUTO falls back to MGS, which zeroes the column
    (test_orthogonalize_mgs_method_and_rank_deficiency)"""
    L = _L()
    Z = rng_for(N, k, 42).standard_normal((N, k))
    Z[:, 3] = Z[:, 0] - 2 * Z[:, 1]
    q = env.block(N, k, Z)
    env.snapshot()
    R = q.mv.orthogonalize(L.QR_AUTO)
    env.check(written=[q], what="hfmi_borth_qr AUTO on a rank-deficient block")
    Qd = q.mv.to_dense()
    assert R[3, 3] == 0.0 and not Qd[:, 3].any() and np.all(np.isfinite(Qd))
    keep = [j for j in range(k) if j != 3]
    assert np.abs(Qd[:, keep].T @ Qd[:, keep] - np.eye(k - 1)).max() < 1e-10


def w_borthogonalize(env, N, k):
    """hfmi_borth_qr with B: Q and BQ both windows (test_Borthogonalize: 1e-12 orthonormality and BQ, 1e-11 QR = Z)"""
    hf, L = _hf(), _L()
    M, K = _fem(N)
    Bm = (M + 1e-3 * K).tocsr()
    Bop = hf.CsrOperator(Bm, ctx=env.ctx)
    Z = rng_for(N, k, 43).standard_normal((N, k)) @ np.diag(np.logspace(0, -4, k))
    for method in (L.QR_CHOL, L.QR_MGS):
        q, bq = env.blocks(N, k, k)
        put(q, Z)
        put(bq, np.ones((N, k)))
        R, passes = np.zeros((k, k)), C.c_int(0)
        env.snapshot()
        L.call("hfmi_borth_qr", q.mv.handle, Bop._op, bq.mv.handle, L.ptr(R), int(method), C.byref(passes))
        env.check(written=[q, bq], what="hfmi_borth_qr with B, method %d" % method)
        Qd = q.mv.to_dense()
        assert np.linalg.norm(Qd.T @ (Bm @ Qd) - np.eye(k)) / np.sqrt(k) < 1e-12
        assert rel(bq.mv.to_dense(), Bm @ Qd) < 1e-12
        assert rel(Qd @ R, Z) < 1e-11


# ====================================================================== solvers
def _solver_problem(env, N, k):
    """snapshot-Gram operator with a decaying spectrum, mass matrix B, its solver, Gaussian probes (as tests/test_gpu_single_pass.py)"""
    hf = _hf()
    rng = rng_for(N, k, 51)
    n = 40
    X = (np.linalg.qr(rng.standard_normal((N, n)))[0] * np.exp(-0.4 * np.arange(n))).T
    A = hf.SnapshotGramOperator(hf.MultiVector.from_vectors(X, ctx=env.ctx), scale=1.0)
    M, _ = _fem(N)
    return A, hf.CsrOperator(M, ctx=env.ctx), hf.CsrPCGSolver(M, rel_tol=1e-13, ctx=env.ctx), rng.standard_normal((N, k))


def _solver_case(env, N, k, entry, generalized, s=2):
    """U written into a window, Omega a read-only window; eigenvalues and vectors against the same call on standalone blocks
    (1e-10 / 1e-8: test_device_equals_restatement)"""
    hf, L = _hf(), _L()
    A, B, Binv, Om = _solver_problem(env, N, k)
    r = k - 4
    om, u = env.blocks(N, k, r)
    put(om, Om)
    put(u, np.ones((N, r)))

    def run(omega, U):
        d = np.empty(r)
        if generalized:
            L.call(entry + "_g", A._op, B._op, Binv._op, omega.handle, r, s, 0, L.ptr(d), U.handle)
        else:
            L.call(entry, A._op, omega.handle, r, s, 0, L.ptr(d), U.handle)
        return d

    env.snapshot()
    d = run(om.mv, u.mv)
    env.check(written=[u], what=entry + ("_g" if generalized else ""))
    Us = hf.MultiVector(N, r, ctx=env.ctx)
    ds = run(hf.MultiVector.from_dense(Om, ctx=env.ctx), Us)
    assert np.abs(d - ds).max() <= 1e-10 * np.abs(ds).max()
    Ud, Usd = u.mv.to_dense(), Us.to_dense()
    for j in range(5):
        assert min(rel(Ud[:, j], Usd[:, j]), rel(-Ud[:, j], Usd[:, j])) <= 1e-8
    return A, B, Binv, Om


def w_double_pass(env, N, k):
    _solver_case(env, N, k, "hfmi_double_pass", False)


def w_double_pass_g(env, N, k):
    _solver_case(env, N, k, "hfmi_double_pass", True)


def w_single_pass(env, N, k):
    _solver_case(env, N, k, "hfmi_single_pass", False)


def w_single_pass_g(env, N, k):
    _solver_case(env, N, k, "hfmi_single_pass", True)


def w_sketch_eig(env, N, k):
    """hfmi_sketch_eig: P and Y read-only windows, U a window; equals hfmi_single_pass with s = 1 on the same probes
    (1e-11 / 1e-8: test_streamed_sketch_snapshots)"""
    hf, L = _hf(), _L()
    A, B, Binv, Om = _solver_problem(env, N, k)
    r = k - 4
    p, y, u = env.blocks(N, k, k, r)
    put(p, Om)
    put(u, np.ones((N, r)))
    A.matMvMult(p.mv, y.mv)
    d = np.empty(r)
    env.snapshot()
    L.call("hfmi_sketch_eig", p.mv.handle, y.mv.handle, None, None, r, 0, L.ptr(d), u.mv.handle)
    env.check(written=[u], what="hfmi_sketch_eig")
    Us, ds = hf.MultiVector(N, r, ctx=env.ctx), np.empty(r)
    Oms = hf.MultiVector.from_dense(Om, ctx=env.ctx)
    L.call("hfmi_single_pass", A._op, Oms.handle, r, 1, 0, L.ptr(ds), Us.handle)
    assert np.abs(d - ds).max() <= 1e-11 * np.abs(ds).max()
    Ud, Usd = u.mv.to_dense(), Us.to_dense()
    for j in range(5):
        assert min(rel(Ud[:, j], Usd[:, j]), rel(-Ud[:, j], Usd[:, j])) <= 1e-8


def w_single_pass_singular(env, N, k):
    """include/hfmi.h on hfmi_single_pass[_g] / the sketch: 'A singular or non-finite Wt (... dependent probe vectors) is
    HFMI_ERR_NUMERIC, never NaN eigenpairs'.  Dependent probes: error raised, no NaN or Inf in U, guards and padding intact."""
    hf, L = _hf(), _L()
    A, B, Binv, Om = _solver_problem(env, N, k)
    Om[:, 1] = Om[:, 0]
    Om[:, 2] = 0.0
    r = k - 4
    for entry in ("hfmi_single_pass", "hfmi_single_pass_g", "hfmi_sketch_eig"):
        om, y, u = env.blocks(N, k, k, r)
        put(om, Om)
        put(u, np.ones((N, r)))
        A.matMvMult(om.mv, y.mv)
        d = np.full(r, 7.0)
        env.snapshot()
        with pytest.raises(hf.HfmiError) as e:
            if entry == "hfmi_single_pass":
                L.call(entry, A._op, om.mv.handle, r, 1, 0, L.ptr(d), u.mv.handle)
            elif entry == "hfmi_single_pass_g":
                L.call(entry, A._op, B._op, Binv._op, om.mv.handle, r, 1, 0, L.ptr(d), u.mv.handle)
            else:
                L.call(entry, om.mv.handle, y.mv.handle, None, None, r, 0, L.ptr(d), u.mv.handle)
        assert e.value.code == -4, e.value
        env.check(written=[u], what=entry + " with a singular Wt")
        assert np.all(np.isfinite(u.mv.to_dense())) and np.all(np.isfinite(d))


# ====================================================================== collectives (one rank)
_COMMS = {}


def _comm(ctx, transport):
    """one communicator of one rank per transport for the whole module (HFMI_COMM_TRANSPORT is read when it is made)"""
    hf = _hf()
    if transport not in _COMMS:
        old = os.environ.get("HFMI_COMM_TRANSPORT")
        if transport == "p2p":
            os.environ["HFMI_COMM_TRANSPORT"] = "p2p"
        try:
            _COMMS[transport] = hf.NativeCollective.from_unique_id(hf.NativeCollective.unique_id(), 1, 0, ctx=ctx)
        finally:
            if transport == "p2p":
                if old is None:
                    del os.environ["HFMI_COMM_TRANSPORT"]
                else:
                    os.environ["HFMI_COMM_TRANSPORT"] = old
    return _COMMS[transport]


def w_collectives(env, N, k):
    """hfmi_allreduce / hfmi_bcast over one rank, RCCL and p2p loop-back (the routes test_gpu_comm.py opens): the same bits back,
    nothing else touched"""
    hf = _hf()
    data = rng_for(N, k, 61).standard_normal((N, k))
    w = env.block(N, k, data)
    for transport in ("rccl", "p2p"):
        coll = _comm(env.ctx, transport)
        assert coll.transport == transport
        env.snapshot()
        for op in ("sum", "avg"):
            coll.allReduce(w.mv, op)
            env.check(written=[w], what="hfmi_allreduce %s over %s" % (op, transport))
            assert np.array_equal(w.mv.to_dense(), data)
        coll.bcast(w.mv, root=0)
        env.check(written=[w], what="hfmi_bcast over %s" % transport)
        assert np.array_equal(w.mv.to_dense(), data)


# ====================================================================== the table
class Writer:
    def __init__(self, name, covers, run, shapes=None, modes=None):
        self.name, self.covers, self.run = name, tuple(covers), run
        self.shapes = SHAPES if shapes is None else shapes
        self.modes = MODES if modes is None else modes


APPLY = ("hfmi_op_apply",)
SQUARE = [(31, 1), (33, 1), (34, 1), (35, 1), (64, 1), (1025, 1)]                        # N x N blocks
# hfmi_block_dot through tn_panel WITH partial sums, so that launch_reduce_partials runs: m or k above 160 keeps the product off the
# skinny x skinny kernel, and N = 4225 gives 133 stages of 32 rows, enough for the split search to take nsplit > 1 (it stops at
# fewer than 16 stages per split).  256 x 256 = 65536 elements takes the vector reduction, 255 x 256 = 65280 the scalar one;
# 300 x 260 splits into a 256-column and a 4-column panel (k > 256) and reduces rows that are not back to back.  Each shape is also run
# with explicit split counts.  (35, 256, 256) is the small-N case of the same result size: one split, stored directly, no reduction.
DOT_EXTRA = [(4225, 256, 256), (4225, 255, 256), (4225, 300, 260), (4225, 257, 258), (35, 256, 256)]
# the LDS-resident and the split paths of tsgemm_nn, from NN_SHAPES of test_gpu_kernels.py
NN_EXTRA = [(4225, 256, 30), (1000, 300, 260), (3000, 2048, 138), (20011, 74, 64), (5000, 300, 84), (4000, 50, 9)]
SOLVER_SHAPES = [(4225, 18), (2017, 12), (1000, 21)]
QR_SHAPES = [(33, 5), (63, 16), (4225, 17), (4225, 74), (65539, 138), (2000, 25)]
AMG_SHAPES = [(65, 1), (65, 17), (65, 138), (30, 5)]                                    # (nx, k): N = nx^2 = 4225, 900

WRITERS = [
    Writer("create", ("hfmi_block_create",), w_create, modes=["view"]),
    Writer("wrap", ("hfmi_block_wrap",), w_wrap),
    Writer("zero", ("hfmi_block_zero",), w_zero),
    Writer("scale", ("hfmi_block_scale",), w_scale),
    Writer("axpy", ("hfmi_block_axpy",), w_axpy),
    Writer("copy", ("hfmi_block_copy",), w_copy),
    Writer("copy_across_ld", ("hfmi_block_copy",), w_copy_across_ld),
    Writer("swap", (), w_swap),
    Writer("randn_fill", ("hfmi_randn_fill",), w_randn),
    Writer("fill_matern32", ("hfmi_block_fill_matern32",), w_matern, shapes=SQUARE),
    Writer("upload", ("hfmi_block_upload",), w_upload),
    Writer("upload_async", ("hfmi_block_upload_async",), w_upload_async),
    Writer("ingest_stream", ("hfmi_block_upload_async",), w_ingest_stream, shapes=SMALL_SHAPES, modes=["view"]),
    Writer("download", (), w_download),
    Writer("gemm_small", ("hfmi_block_gemm_small",), w_gemm_small),
    Writer("gemm_small_paths", ("hfmi_block_gemm_small",), lambda env, N, m, r: _gemm_small(env, N, m, r), shapes=NN_EXTRA),
    Writer("reduce", ("hfmi_block_gemm_small",), w_reduce),
    Writer("bench_tsgemm_nn", ("hfmi_bench_tsgemm_nn",), w_bench_tsgemm_nn, shapes=SMALL_SHAPES),
    Writer("dot_norms", (), w_dot_norms),
    Writer("dot_paths", (), lambda env, N, m, k: _dot(env, N, m, k, nsplits=(1, 4, 7)), shapes=DOT_EXTRA),
    Writer("gram_eig", (), w_gram_eig, shapes=[(2017, 17), (4225, 74), (35, 16)]),
    Writer("op_csr_ell", APPLY, w_csr_ell),
    Writer("op_csr_irregular", APPLY, w_csr_irregular, shapes=SMALL_SHAPES + [(3001, 74)]),
    Writer("op_dense_sym", APPLY, w_dense_sym, shapes=[(31, 5), (33, 17), (34, 1), (35, 74), (1025, 138), (64, 16)]),
    Writer("op_snapshot_gram", APPLY, w_snapshot_gram),
    Writer("op_low_rank", APPLY, w_low_rank),
    Writer("op_jtj", APPLY, w_jtj),
    Writer("op_jjt", APPLY, w_jjt, shapes=SMALL_SHAPES),
    Writer("op_compose3", APPLY, w_compose3, shapes=SMALL_SHAPES),
    Writer("op_host_callback", APPLY, w_host_callback, shapes=SMALL_SHAPES),
    Writer("op_csr_pcg", APPLY, w_csr_pcg, shapes=[(63, 5), (4225, 17), (2017, 138)]),
    Writer("op_amg_pcg", APPLY, w_amg_pcg, shapes=AMG_SHAPES),
    Writer("op_amg_pcg_error", APPLY, w_amg_pcg_error, shapes=[(65, 17), (30, 5)]),
    Writer("amg_vcycle", ("hfmi_amg_vcycle",), w_amg_vcycle, shapes=AMG_SHAPES),
    Writer("orthogonalize", ("hfmi_borth_qr",), w_orthogonalize, shapes=QR_SHAPES),
    Writer("orthogonalize_rank_deficient", ("hfmi_borth_qr",), w_orthogonalize_rank_deficient, shapes=[(500, 6), (4225, 17)]),
    Writer("Borthogonalize", ("hfmi_borth_qr",), w_borthogonalize, shapes=[(2000, 25), (4225, 17), (63, 5)]),
    Writer("double_pass", ("hfmi_double_pass",), w_double_pass, shapes=SOLVER_SHAPES),
    Writer("double_pass_g", ("hfmi_double_pass_g",), w_double_pass_g, shapes=SOLVER_SHAPES),
    Writer("single_pass", ("hfmi_single_pass",), w_single_pass, shapes=SOLVER_SHAPES),
    Writer("single_pass_g", ("hfmi_single_pass_g",), w_single_pass_g, shapes=SOLVER_SHAPES),
    Writer("sketch_eig", ("hfmi_sketch_eig",), w_sketch_eig, shapes=SOLVER_SHAPES),
    Writer("single_pass_singular", ("hfmi_single_pass", "hfmi_single_pass_g", "hfmi_sketch_eig"), w_single_pass_singular,
           shapes=[(2017, 12)]),
    Writer("collectives", ("hfmi_allreduce", "hfmi_bcast"), w_collectives, shapes=[(33, 5), (4225, 17), (65539, 16)]),
]

# prototypes of include/hfmi.h with a non-const hfmi_block* that do NOT store into block memory, and why
NOT_A_WRITER = {
    "hfmi_block_view": "makes a handle onto the parent's columns; no device work",
    "hfmi_block_destroy": "frees the handle (and the allocation of an owner); stores nothing",
    "hfmi_philox_raw": "the block gives the shape only; the stream is written to a host array",
    "hfmi_post_apply_fn": "a callback typedef: the callee is the caller's code (hfmi_allreduce is covered on its own)",
}

CASES = [pytest.param(w, mode, shape, id="%s-%s-%s" % (w.name, mode, "x".join(map(str, shape))))
         for w in WRITERS for shape in w.shapes for mode in w.modes]


@pytest.mark.parametrize("writer,mode,shape", CASES)
def test_block_contract(ctx, writer, mode, shape):
    writer.run(Env(ctx, mode), *shape)
