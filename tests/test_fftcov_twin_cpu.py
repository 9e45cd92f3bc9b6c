"""The numpy statement of the grid operator (tests/helpers/fftcov_twin.py: embedding, node map, pairing, nugget, ``numpy.fft``) against
the dense host covariance ``hf.kernel_cov_host(points, ...) @ W`` over the case table of the GPU suite, under the GPU suite's bound
per column
    ||Y_j - Yref_j||_2 <= 32 max(1, log2 P) eps sqrt(P) ||c||_2 ||W_j||_2 + 8 N eps || |C| |W_j| ||_2 .
The circulant embedding is exact, so what is left is rounding; the twin uses a small fraction of the bound, which is the room the
device's own transforms have."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import fftcov_twin as tw                          # noqa: E402

hf = pytest.importorskip("hippyflow_amd")

SIGMA = 1.3
CASES = tw.cases()


def test_case_table_covers_what_it_should():
    shapes = {c[1] for c in CASES}
    assert shapes == set(tw.SHAPES) and len(CASES) == 2 * len(tw.SHAPES) + 1
    P = sorted({tw.embed_len(n) for s in shapes for n in s})
    assert P[0] == 1 and P[-1] == 4096 and {32, 64, 128} <= set(P)                   # 16 -> 32, 17 -> 64; 32 -> 64, 33 -> 128
    assert {c[4] for c in CASES} >= {1, 2, 5, 17, 74, 290}
    assert {c[5] for c in CASES} == set(tw.FAMILIES) and {c[6] for c in CASES} == {0.05, 1.0} and {c[7] for c in CASES} == {0.0, 0.3}
    assert {c[8] for c in CASES} == {0, 1}
    assert [tw.embed_len(n) for n in (1, 2, 3, 16, 17, 32, 33, 2048)] == [1, 4, 8, 32, 64, 64, 128, 4096]


@pytest.mark.parametrize("cid,shape,spacing,kind,nvec,family,ell,nugget,accumulate", CASES, ids=[c[0] for c in CASES])
def test_twin_against_the_dense_covariance(cid, shape, spacing, kind, nvec, family, ell, nugget, accumulate):
    nodes = tw.nodes_of(shape, kind)
    pts = tw.points(shape, spacing, nodes)
    N = pts.shape[0]
    if nodes is not None:
        assert np.unique(nodes).size == N and (kind != "subset" or N == max(1, 3 * int(np.prod(shape)) // 4))
    nvec = min(nvec, 6) if N > tw.DENSE_MAX_N else nvec              # the host's share of the large shapes; the GPU suite keeps nvec
    W = np.random.default_rng(1000 + N + nvec).standard_normal((N, nvec))
    rows = tw.reference_rows(N)
    CW, absCW = tw.host_products(hf, pts, family, SIGMA, ell, nugget, W, rows=rows)
    Y = tw.apply(shape, spacing, family, SIGMA, ell, nugget, W, nodes)
    Y = Y if rows is None else Y[rows]
    ratio = np.linalg.norm(Y - CW, axis=0) / tw.column_bounds(shape, spacing, family, SIGMA, ell, nugget, W, absCW)
    print("fftcov twin %s: N=%d k=%d worst err/bound = %.3g" % (cid, N, nvec, ratio.max()))
    assert ratio.max() <= 1.0


def test_pairing_changes_only_the_last_bits():
    shape, spacing = (17, 9), (0.013, 0.021)
    W = np.random.default_rng(3).standard_normal((17 * 9, 4))
    Y = tw.apply(shape, spacing, "matern32", SIGMA, 0.3, 0.1, W)
    Y1 = tw.apply(shape, spacing, "matern32", SIGMA, 0.3, 0.1, W[:, 1:])           # columns 1, 2, 3 with other partners
    assert np.abs(Y[:, 1:] - Y1).max() <= 1e-13 * np.abs(Y).max()
