"""CPU twin of k_kcov (hippyflow_amd/csrc/hfmi_kcov.hip): Y (+)= C W with C evaluated entry by entry, in the kernel's order.

Same structure as the device code: column panels of ``PANEL`` = 144 columns, row tiles of 16, the sweep over j in LDS chunks of ``JC`` = 64
rows cut into slabs of 4 (one v_mfma_f64_16x16x4_f64 step: the four products of a slab are added to the accumulator one after the other,
k = 0..3), accumulators started at zero and added to Y at the end when ``accumulate``.  The entry formula is the kernel's branch-free
one: a = ca |x_i - x_j| / ell, phi = (1 + p1 a + p2 a^2) exp(-a (g1 + g2 a)), plus the nugget where the indices are equal.  numpy has no
fused multiply-add, so an element can differ from the device in the last bits; the order of the sum is the same.
"""
import numpy as np

JC, SLAB, ROWS, PANEL = 64, 4, 16, 144
COEFFS = {                      # family: (ca, p1, p2, g1, g2)
    "matern12": (1.0, 0.0, 0.0, 1.0, 0.0),
    "matern32": (1.7320508075688772, 1.0, 0.0, 1.0, 0.0),
    "matern52": (2.23606797749979, 1.0, 1.0 / 3.0, 1.0, 0.0),
    "sqexp": (1.0, 0.0, 0.0, 0.0, 0.5),
}


def entries(points, rows, cols, family, sigma, ell, nugget):
    """C[rows, cols] by the kernel's formula (rows, cols: index arrays)."""
    ca, p1, p2, g1, g2 = COEFFS[family]
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim == 1:
        pts = pts[:, None]
    r2 = np.zeros((len(rows), len(cols)))
    for c in range(pts.shape[1]):
        dx = pts[rows, c][:, None] - pts[cols, c][None, :]
        r2 = dx * dx + r2
    a = ca * np.sqrt(r2) * (1.0 / ell)
    poly = a * (p2 * a + p1) + 1.0
    g = a * (g2 * a + g1)
    v = sigma * sigma * poly * np.exp(-g)
    v[rows[:, None] == cols[None, :]] += nugget
    return v


def apply(points, W, family="matern32", sigma=1.0, ell=0.1, nugget=0.0, Y=None, accumulate=False):
    """Y (+)= C W in the device kernel's summation order.  W: (N, k)."""
    W = np.asarray(W, dtype=np.float64)
    N, k = W.shape
    out = np.zeros((N, k)) if (Y is None or not accumulate) else np.array(Y, dtype=np.float64)
    for c0 in range(0, k, PANEL):                                   # one launch per column panel
        Wp = W[:, c0:c0 + PANEL]
        for r0 in range(0, N, ROWS):                                # one wave's 16 rows
            rows = np.arange(r0, min(N, r0 + ROWS))
            acc = np.zeros((len(rows), Wp.shape[1]))
            for j0 in range(0, N, JC):                              # LDS chunk
                for s0 in range(j0, min(N, j0 + JC), SLAB):         # one MFMA step: 16 x 4 slab of C
                    cols = np.arange(s0, min(N, s0 + SLAB))
                    slab = entries(points, rows, cols, family, sigma, ell, nugget)
                    for q in range(len(cols)):                      # k = 0..3 inside the instruction
                        acc = acc + slab[:, q:q + 1] * Wp[cols[q]:cols[q] + 1, :]
            if accumulate and Y is not None:
                out[rows, c0:c0 + PANEL] = out[rows, c0:c0 + PANEL] + acc
            else:
                out[rows, c0:c0 + PANEL] = acc
    return out
