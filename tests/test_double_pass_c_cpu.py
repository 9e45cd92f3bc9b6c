"""The double pass in encoder coordinates (``randomized.doublePassC``: a prior given by its covariance C alone, no R, no solve)
restated in numpy (tests/helpers/grid_factor_twin.py) against the oracle's ``doublePassG`` with R = inv(C) and the same Omega: the same
eigenvalues and decoder, and an encoder that is R U without R ever applied.  No device; the GPU suite scales its tolerances from
the differences measured here."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import grid_factor_twin as tw                     # noqa: E402

hf = pytest.importorskip("hippyflow_amd")


@pytest.mark.parametrize("case", tw.DPC_CASES, ids=["%s-%s-ell%g" % ("x".join(map(str, c[0])), c[2], c[3]) for c in tw.DPC_CASES])
def test_double_pass_c_is_double_pass_g_without_the_precision(case):
    """d to 1e-11 relative (measured <= 1.1e-13), U to 1e-10 after fixing signs (measured <= 3e-13; the smallest relative gap of the
    kept eigenvalues is 3.7e-2), E^T U - I <= 1e-12 (measured 1e-14); E against R U is printed (<= 9e-12 at cond(C) = 1e5)"""
    r = tw.dpc_reference(case)
    k = case[5]
    gaps = np.abs(np.diff(r["d_ref"])) / np.abs(r["d_ref"][:-1])
    print("doublePassC %s: d %.3g, U %.3g, U^T R U - I %.3g, E^T U - I %.3g, E - R U %.3g, cond(C) %.3g, smallest gap %.3g"
          % (case[:4], r["dd"], r["dU"], r["defect"], r["EtU"], np.abs(r["E"] - r["R"] @ r["U"]).max(), np.linalg.cond(r["C"]), gaps.min()))
    assert r["d"].shape == (k,) and r["U"].shape == r["E"].shape == (r["C"].shape[0], k)
    assert np.all(np.diff(r["d"]) <= 0.0) and r["d"][-1] > 0.0
    assert r["dd"] <= 1e-11
    assert r["dU"] <= 1e-10
    assert r["EtU"] <= 1e-12


def test_the_library_has_the_entry_point():
    from hippyflow_amd import randomized
    assert hf.doublePassC is randomized.doublePassC
    import inspect
    assert list(inspect.signature(hf.doublePassC).parameters) == ["A", "C", "Omega", "k", "s", "sort_by_abs", "use_mgs"]
    assert hf.GridKernelPrior is not None
