"""Failed creates free all.  Every device buffer, pinned buffer, event and stream of the library comes from one choke point
(csrc/hfmi_own.h) that counts them and that hfmi_test_own_fail can make fail on the host (nothing is launched, nothing faults).

Every case is a short sequence of C-ABI calls that starts with a SECOND context on the device, so that the parts a context makes
lazily (workspace slots, cached temporaries, pinned staging, the wide arena, the ingest ring, the transfer ring, the late-check
buffer) are made inside the sequence, and ends with everything destroyed.  The sequence is run clean (warm-up), clean again to
count its A acquisitions and record its output, then once for every first = 1 .. A with acquisitions first and first + 1 failing
(two, because an allocation is retried once after the block pool was flushed).  A call that fails must return HFMI_ERR_HIP and
leave *out as it was; the sequence stops there and destroys what it made.  A sequence that still succeeds (the retry or the
grid covariance's fall-back to chunks absorbed the failure) must give the clean output bit for bit.  Either way live - pooled is
back at the baseline for every kind, and at no point is live below what the sequence itself holds (a double release)."""
import ctypes as C
import gc

import numpy as np
import pytest

from hippyflow_amd import _lib as L

pytestmark = pytest.mark.gpu

ERR_HIP = -2
SENTINEL = 0x5A5A5A50
# what an object holds at least, per kind: a context its small arena and status words, its pinned status words, the events of
# hfmi_ctx_create (ev0, ev1, status, side, 4 callback, 8 panel, join) and its two streams
HOLDS = {"ctx": (2, 1, 17, 2), "block": (1, 0, 0, 0), "csr": (3, 0, 0, 0), "pinned": (0, 1, 0, 0)}
DESTROY = {"ctx": "hfmi_ctx_destroy", "block": "hfmi_block_destroy", "csr": "hfmi_csr_destroy", "op": "hfmi_op_destroy",
           "amg": "hfmi_amg_destroy", "pchol": "hfmi_pchol_destroy", "pinned": "hfmi_host_free_pinned"}


def counts(ctx=None):
    live, acquired, pooled = (C.c_int64 * 4)(), (C.c_int64 * 4)(), C.c_int64(0)
    L.call("hfmi_test_own_counts", ctx, live, acquired, C.byref(pooled))
    return list(live), list(acquired), pooled.value


class CallFailed(Exception):
    pass


class Sequence:
    """One run of a case: makes the second context, tracks what it made, destroys it in reverse order."""

    def __init__(self, base_live):
        self.lib = L.load()
        self.base_live = base_live
        self.made = []                      # (kind of object, handle)
        self.held = [0, 0, 0, 0]
        self.ctx = None

    def check_held(self):
        live, _, _ = counts(self.ctx)
        for k in range(4):
            assert live[k] - self.base_live[k] >= self.held[k], "kind %d: %d live, the sequence holds %d" % (k, live[k] - self.base_live[k], self.held[k])

    def call(self, name, *args):
        status = getattr(self.lib, name)(*args)
        self.check_held()
        if status != 0:
            raise CallFailed("%s -> %d: %s" % (name, status, self.lib.hfmi_last_error().decode("utf-8", "replace")), status)

    def make(self, what, name, *args):
        """a call whose last argument is the out handle"""
        out = C.c_void_p(SENTINEL)
        try:
            self.call(name, *(args + (C.byref(out),)))
        except CallFailed:
            assert out.value == SENTINEL, "%s failed and wrote *out" % name
            raise
        assert out.value not in (None, SENTINEL)
        self.made.append((what, out))
        self.held = [h + d for h, d in zip(self.held, HOLDS.get(what, (0, 0, 0, 0)))]
        return out

    def start(self):
        self.ctx = self.make("ctx", "hfmi_ctx_create", 0)
        return self.ctx

    def block(self, host):
        """host: (nvec, N) array -> an N x nvec block holding it"""
        host = L.as_f64(host)
        b = self.make("block", "hfmi_block_create", self.ctx, host.shape[1], host.shape[0])
        self.call("hfmi_block_upload", b, L.ptr(host), L.LAYOUT_VECTORS)
        return b

    def empty(self, N, nvec):
        return self.make("block", "hfmi_block_create", self.ctx, N, nvec)

    def download(self, b, N, nvec):
        host = np.empty((nvec, N))
        self.call("hfmi_block_download", b, L.ptr(host), L.LAYOUT_VECTORS)
        return host.tobytes()

    def csr(self, dense):
        dense = np.asarray(dense, dtype=np.float64)
        indptr, indices, data = [0], [], []
        for row in dense:
            nz = np.nonzero(row)[0]
            indices += list(nz)
            data += list(row[nz])
            indptr.append(len(indices))
        ip, ix, dv = np.array(indptr, np.int64), np.array(indices, np.int32), np.array(data, np.float64)
        return self.make("csr", "hfmi_csr_create", self.ctx, dense.shape[0], dense.shape[1], len(dv), L.ptr(ip), L.ptr(ix), L.ptr(dv))

    def drop(self, handle):
        """destroy one object ahead of the end"""
        i = [j for j, (_, h) in enumerate(self.made) if h is handle][0]
        self.destroy(*self.made.pop(i))

    def destroy(self, what, handle):
        assert getattr(self.lib, DESTROY[what])(handle) == 0
        self.held = [h - d for h, d in zip(self.held, HOLDS.get(what, (0, 0, 0, 0)))]
        if what == "ctx":
            self.ctx = None
        self.check_held()

    def finish(self):
        while self.made:
            self.destroy(*self.made.pop())


# ------------------------------------------------------------------ the cases
RNG = np.random.default_rng(20261020)
W33 = RNG.standard_normal((2, 33))
W50 = RNG.standard_normal((5, 50))
W64 = RNG.standard_normal((5, 64))
POINTS = RNG.random((50, 2))
TARGETS = RNG.random((20, 2))
X64x8 = RNG.standard_normal((8, 64))
T1025 = RNG.standard_normal((1025, 1025))
T1025 = (T1025 + T1025.T) / 2


def tridiag(n, diag=2.0):
    return diag * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)


def case_context(s):
    return b""


def apply_csr(s, dense, W):
    m = s.csr(dense)
    op = s.make("op", "hfmi_op_csr", s.ctx, m)
    w, y = s.block(W), s.empty(dense.shape[0], W.shape[0])
    s.call("hfmi_op_apply", op, w, y, 0)
    return s.download(y, dense.shape[0], W.shape[0])


def case_csr_tridiagonal(s):          # rows of 3: the ELL image is taken
    return apply_csr(s, tridiag(33), W33)


def case_csr_dense_row(s):            # a first row of 66 entries: the ELL image is refused
    a = tridiag(66)
    a[0, :] = 1.0 + np.arange(66)
    return apply_csr(s, a, RNG_W66)


RNG_W66 = np.random.default_rng(7).standard_normal((2, 66))


def case_low_rank(s):
    s.drop(s.empty(64, 3))            # into the pool: the block below comes out of it, later failures flush and retry
    u = s.block(W64[:3])
    d = np.array([3.0, 2.0, 1.0])
    op = s.make("op", "hfmi_op_low_rank", s.ctx, u, L.ptr(d))
    w, y = s.block(W64[3:]), s.empty(64, 2)
    s.call("hfmi_op_apply", op, w, y, 0)
    return s.download(y, 64, 2)


def case_jtj(s):
    j = s.block(np.random.default_rng(3).standard_normal((6, 40)))       # ndata = 2 samples of q = 3 rows
    g = np.array([[2.0, 0.5, 0.0], [0.5, 1.5, 0.25], [0.0, 0.25, 1.0]])
    op = s.make("op", "hfmi_op_jtj", s.ctx, j, 2, 3, L.ptr(g), 0.5)
    w, y = s.block(np.random.default_rng(4).standard_normal((2, 40))), s.empty(40, 2)
    s.call("hfmi_op_apply", op, w, y, 0)
    return s.download(y, 40, 2)


def kernel_cov(s):
    return s.make("op", "hfmi_op_kernel_cov", s.ctx, L.ptr(POINTS), 50, 2, 1, 1.3, 0.4, 1e-3)


def case_kernel_cov(s):
    op = kernel_cov(s)
    w, y = s.block(W50[:2]), s.empty(50, 2)
    s.call("hfmi_op_apply", op, w, y, 0)
    return s.download(y, 50, 2)


def case_kernel_cross_cov(s):
    op = s.make("op", "hfmi_op_kernel_cross_cov", s.ctx, L.ptr(TARGETS), 20, L.ptr(POINTS), 50, 2, 1, 1.3, 0.4, 0.0, L.KERNEL_NO_DIAGONAL)
    w, y = s.block(W50[:2]), s.empty(20, 2)
    s.call("hfmi_op_apply", op, w, y, 0)
    return s.download(y, 20, 2)


def case_kernel_cov_grid(s):          # 50 of the 64 nodes of an 8 x 8 grid; 5 vectors: the work buffer grows at the first apply
    n, h = np.array([8, 8], np.int64), np.array([0.1, 0.1])
    nodes = np.sort(np.random.default_rng(5).permutation(64)[:50]).astype(np.int64)
    op = s.make("op", "hfmi_op_kernel_cov_grid", s.ctx, 2, L.ptr(n), L.ptr(h), L.ptr(nodes), 50, 1, 1.3, 0.4, 1e-3)
    w, y = s.block(W50), s.empty(50, 5)
    s.call("hfmi_op_apply", op, w, y, 0)
    return s.download(y, 50, 5)


def case_amg(s):                      # 33 -> 17 rows of the 1-D Laplacian, linear interpolation; the first V-cycle reserves the work arrays
    a = tridiag(33)
    p = np.zeros((33, 17))
    for c in range(17):
        p[2 * c, c] = 1.0
        if c > 0:
            p[2 * c - 1, c] = 0.5
        if c < 16:
            p[2 * c + 1, c] = 0.5
    ac = p.T @ a @ p
    ac[np.abs(ac) < 1e-14] = 0.0
    A, P, R, Ac = s.csr(a), s.csr(p), s.csr(p.T.copy()), s.csr(ac)
    g = s.make("amg", "hfmi_amg_create", s.ctx, A, 0.5, 2.2, 2)
    s.call("hfmi_amg_add_level", g, P, R, Ac, 0.5, 2.2)
    inv = np.ascontiguousarray(np.linalg.inv(ac))
    s.call("hfmi_amg_set_coarse", g, 17, L.ptr(inv))
    b, x = s.block(W33), s.empty(33, 2)
    s.call("hfmi_amg_vcycle", g, b, x)
    return s.download(x, 33, 2)


def case_pchol(s):
    op = kernel_cov(s)
    f = s.make("pchol", "hfmi_pchol_create", op, 8, 0.0)
    rank, piv, trace = C.c_int(0), np.zeros(8, np.int64), np.zeros(9)
    s.call("hfmi_pchol_info", f, C.byref(rank), None, None)
    s.call("hfmi_pchol_read", f, L.ptr(piv), L.ptr(trace))
    factor = C.c_void_p()
    s.call("hfmi_pchol_factor", f, C.byref(factor))
    return piv.tobytes() + trace.tobytes() + s.download(factor, 50, rank.value)


def case_sparse_solve(s):             # the first solve: inv_diag, cached temporaries, workspace slots
    m = s.csr(tridiag(33, 2.5))
    op = s.make("op", "hfmi_op_csr_pcg", s.ctx, m, 1e-12, 200)
    w, y = s.block(W33), s.empty(33, 2)
    s.call("hfmi_op_apply", op, w, y, 0)
    return s.download(y, 33, 2)


def case_wide_qr(s):                  # 257 vectors: the first wide call makes the wide arena and the out-of-place temporary
    q = s.empty(512, 257)
    s.call("hfmi_randn_fill", q, 11, 0, 1.0)
    r, passes = np.zeros((257, 257)), C.c_int(0)
    s.call("hfmi_borth_qr", q, None, None, L.ptr(r), L.QR_CHOL, C.byref(passes))
    return r.tobytes() + s.download(q, 512, 257)


def _twice(user, w_host, y_host, N, k):
    for i in range(N * k):
        y_host[i] = 2.0 * w_host[i]
    return 0


TWICE = L.HOST_APPLY_FN(_twice)


def case_host_callback(s):            # slabs of 2 of 5 vectors: the double-buffered pinned slabs are made at the first apply
    op = s.make("op", "hfmi_op_host_callback", s.ctx, TWICE, None, 64)
    s.call("hfmi_op_host_set_chunk", op, 2)
    w, y = s.block(W64), s.empty(64, 5)
    s.call("hfmi_op_apply", op, w, y, 0)
    return s.download(y, 64, 5)


def case_ingest(s):                   # the first asynchronous upload makes the ingest stream, its ring of events and its staging buffer
    pin = s.make("pinned", "hfmi_host_alloc_pinned", C.c_size_t(64 * 3 * 8))
    np.frombuffer((C.c_char * (64 * 3 * 8)).from_address(pin.value), dtype=np.float64)[:] = np.ascontiguousarray(W64[:3].T).ravel()
    b = s.empty(64, 3)
    ticket = C.c_int64(-1)
    s.call("hfmi_block_upload_async", b, pin, L.LAYOUT_DENSE, C.byref(ticket))
    s.call("hfmi_ingest_wait", s.ctx, ticket.value)
    s.call("hfmi_ingest_fence", s.ctx)
    return s.download(b, 64, 3)


def case_double_pass(s):              # the second Cholesky-QR pass is taken on trust: the late-check buffer
    x = s.block(X64x8)
    op = s.make("op", "hfmi_op_snapshot_gram", s.ctx, x, 1.0)
    omega, u = s.block(W64), s.empty(64, 3)
    d = np.zeros(3)
    s.call("hfmi_double_pass", op, omega, 3, 1, 0, L.ptr(d), u)
    return d.tobytes() + s.download(u, 64, 3)


def case_large_transfer(s):           # 1025^2 doubles of eigenvectors: the first output beyond the 8 MB threshold of the transfer ring
    d, v = np.empty(1025), np.empty((1025, 1025))
    s.call("hfmi_sym_eig_small", s.ctx, L.ptr(T1025), 1025, 0, L.ptr(d), L.ptr(v))
    return d.tobytes() + v.tobytes()


CASES = [case_context, case_csr_tridiagonal, case_csr_dense_row, case_low_rank, case_jtj, case_kernel_cov, case_kernel_cross_cov,
         case_kernel_cov_grid, case_amg, case_pchol, case_sparse_solve, case_wide_qr, case_host_callback, case_ingest, case_double_pass,
         case_large_transfer]


def run(case, base_live, first=0):
    """-> (output, None) or (None, the failure); everything the sequence made is destroyed either way"""
    s = Sequence(base_live)
    L.call("hfmi_test_own_fail", first, 2)
    try:
        s.start()
        return case(s), None
    except CallFailed as e:
        return None, e
    finally:
        L.call("hfmi_test_own_fail", 0, 0)
        s.finish()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__[5:])
def test_failed_creates_free_all(case):
    L.Context.default()                                   # the first context on the device: the sequences make the second
    gc.collect()                                          # what earlier tests dropped goes now, not in the middle of the count
    base_live, _, base_pooled = counts(L.Context.default().handle)
    baseline = [base_live[0] - base_pooled] + base_live[1:]

    def at_baseline():
        live, _, pooled = counts(L.Context.default().handle)
        return [live[0] - pooled] + live[1:] == baseline

    out, failure = run(case, base_live)                   # warm-up
    assert failure is None, failure
    acquired0 = counts()[1]
    clean, failure = run(case, base_live)
    assert failure is None and clean == out and at_baseline()
    A = sum(counts()[1]) - sum(acquired0)
    assert A >= sum(HOLDS["ctx"])
    failed, where = 0, {}
    for first in range(1, A + 1):
        out, failure = run(case, base_live, first)
        if failure is not None:
            assert failure.args[1] == ERR_HIP, failure
            failed += 1
            where[failure.args[0].split(" ")[0]] = where.get(failure.args[0].split(" ")[0], 0) + 1
        else:
            assert out == clean, "first = %d: absorbed, but another result" % first
        assert at_baseline(), "first = %d: live - pooled is not back at the baseline" % first
    print("%s: A = %d acquisitions, %d runs failed %s, %d absorbed the failure" % (case.__name__[5:], A, failed, where, A - failed))
    assert failed > 0
    out, failure = run(case, base_live)
    assert failure is None and out == clean and at_baseline()
