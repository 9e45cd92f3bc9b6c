"""Host side of the rectangular kernel covariance (no GPU): kernel_cross_cov_host against kernel_cov_host, where the nugget lands,
shard_rows, and the argument errors the Python classes raise before they touch a device."""
import numpy as np
import pytest

hf = pytest.importorskip("hippyflow_amd")

FAMILIES = ["matern12", "matern32", "matern52", "sqexp"]


def scattered(N, d, seed):
    """seeded points in the unit cube, two of them coincident"""
    pts = np.random.default_rng(seed).random((N, d))
    if N > 3:
        pts[N - 1] = pts[1]
    return pts


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d", [1, 2, 3])
def test_slices_of_the_square_matrix(family, d):
    N, sigma, ell, nugget = 41, 1.3, 0.3, 0.25
    pts = scattered(N, d, seed=d)
    full = hf.kernel_cov_host(pts, family, sigma, ell, nugget)
    for r0, r1 in ((0, N), (0, 1), (7, 30), (N - 1, N)):
        K = hf.kernel_cross_cov_host(pts[r0:r1], pts, family, sigma, ell, nugget, diag_offset=r0)
        assert K.shape == (r1 - r0, N)
        assert np.array_equal(K, hf.kernel_cov_host(pts, family, sigma, ell, nugget, rows=range(r0, r1)))
        assert np.array_equal(K, full[r0:r1])


@pytest.mark.parametrize("family", FAMILIES)
def test_disjoint_sets(family):
    """K(T, S) is the off-diagonal block of the covariance of the union; a 1-D array is points on a line"""
    sigma, ell = 0.8, 0.4
    S, T = scattered(23, 2, seed=1), scattered(9, 2, seed=2)
    K = hf.kernel_cross_cov_host(T, S, family, sigma, ell)
    union = hf.kernel_cov_host(np.concatenate([T, S]), family, sigma, ell)
    assert K.shape == (9, 23) and np.array_equal(K, union[:9, 9:])
    assert np.array_equal(hf.kernel_cross_cov_host(S, T, family, sigma, ell), K.T)
    line = hf.kernel_cross_cov_host(np.array([0.0, 0.5]), np.array([0.0, 0.25, 1.0]), family, sigma, ell)
    assert line.shape == (2, 3) and line[0, 0] == sigma ** 2


def test_the_diagonal_is_on_the_index_not_on_coincident_points():
    N, nugget = 12, 0.5
    pts = scattered(N, 2, seed=3)                       # points 1 and N - 1 coincide
    K0 = hf.kernel_cross_cov_host(pts[1:5], pts, "matern32", 1.0, 0.2, 0.0, diag_offset=1)
    K = hf.kernel_cross_cov_host(pts[1:5], pts, "matern32", 1.0, 0.2, nugget, diag_offset=1)
    expect = np.zeros_like(K)
    expect[np.arange(4), np.arange(4) + 1] = nugget
    assert np.array_equal(K - K0, expect)
    assert K0[0, N - 1] == K0[0, 1] == 1.0 and K[0, N - 1] == 1.0 and K[0, 1] == 1.0 + nugget
    # the same targets declared to be other sources: the nugget moves with the declaration
    K2 = hf.kernel_cross_cov_host(pts[1:5], pts, "matern32", 1.0, 0.2, nugget, diag_offset=3)
    assert K2[0, 3] == K0[0, 3] + nugget and K2[0, 1] == 1.0


@pytest.mark.parametrize("N", [1, 7, 333])
@pytest.mark.parametrize("size", [1, 2, 3, 8])
def test_shard_rows(N, size):
    ranges = [hf.shard_rows(N, size, r) for r in range(size)]
    assert ranges[0][0] == 0 and ranges[-1][1] == N
    for (a0, a1), (b0, b1) in zip(ranges, ranges[1:]):
        assert a1 == b0                                  # contiguous and disjoint
    sizes = [r1 - r0 for r0, r1 in ranges]
    assert min(sizes) >= 0 and max(sizes) - min(sizes) <= 1 and sum(sizes) == N
    assert sizes == sorted(sizes, reverse=True)          # the first N % size ranks hold the extra row
    assert sizes.count(max(sizes)) == (N % size or size)
    if size > N:
        assert sizes.count(0) == size - N


def test_shard_rows_arguments():
    for bad in ((10, 0, 0), (10, 2, 2), (10, 2, -1), (-1, 2, 0)):
        with pytest.raises(ValueError):
            hf.shard_rows(*bad)


def test_argument_errors_without_a_device():
    S, T = scattered(10, 2, seed=1), scattered(4, 2, seed=2)
    for make in (hf.kernel_cross_cov_host, hf.KernelCrossCovarianceOperator):
        with pytest.raises(ValueError):
            make(T, S, "matern72", 1.0, 0.1)
        with pytest.raises(ValueError):
            make(T, S, "matern32", 1.0, 0.1, 0.1)                          # a nugget without a diagonal
        with pytest.raises(ValueError):
            make(T, S, "matern32", 1.0, 0.1, 0.0, diag_offset=7)           # 7 + 4 > 10
        with pytest.raises(ValueError):
            make(T, S, "matern32", 1.0, 0.1, 0.0, diag_offset=-2)
        with pytest.raises(ValueError):
            make(T[:, :1], S, "matern32", 1.0, 0.1)                        # 1 coordinate against 2
        with pytest.raises(ValueError):
            make(T[:0], S, "matern32", 1.0, 0.1)
        with pytest.raises(ValueError):
            make(np.zeros((2, 2, 2)), S, "matern32", 1.0, 0.1)
    for r0, r1 in ((-1, 3), (3, 2), (0, 11)):
        with pytest.raises(ValueError):
            hf.KernelCovarianceRowsOperator(S, "matern32", 1.0, 0.1, 0.0, r0, r1)
    with pytest.raises(ValueError):
        hf.KernelCovarianceRowsOperator(S, "matern72", 1.0, 0.1, 0.0, 0, 3)
