"""The numpy restatement of row scaling, ORTHOMIN(north) and CG (tests/accel_restate.py) against the
reference build itself (oracle/_ref, lsr_solve): with sequential sums it reproduces the reference's
solution and iteration count BIT FOR BIT, so the same restatement with the GPU's reduction order
(tree=True) is a sound expected value for tests/test_gpu_lasolver_accel.py.  CPU only."""
import numpy as np
import pytest

import accel_restate as R
import lasolver_py as L

needs_ref = pytest.mark.skipif(not L.ref_available(), reason="the reference build (oracle/_ref) is absent")


def _bit(x, y):
    return np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)


@needs_ref
@pytest.mark.parametrize("name", R.SMALL)
def test_orthomin_equals_reference(name):
    s = R.system(name)
    xr, ir = R.ref_solve(s["ia"], s["ja"], s["a"], s["b"], iaccel=1)
    x, it = R.orthomin(s["ia"], s["ja"], s["a"], s["b"], north=10)
    assert ir > 0 and it == ir and _bit(x, xr), (it, ir)
    tol = np.full(len(xr), 1e-3)  # the toler stopping rule
    xr, ir = R.ref_solve(s["ia"], s["ja"], s["a"], s["b"], iaccel=1, toler=tol, resid_reduc=1e-30)
    x, it = R.orthomin(s["ia"], s["ja"], s["a"], s["b"], north=10, toler=tol, resid_reduc=1e-30)
    assert ir > 0 and it == ir and _bit(x, xr), (it, ir)


@needs_ref
@pytest.mark.parametrize("name", R.SMALL)
@pytest.mark.parametrize("iscal", [0, 1])
def test_cg_equals_reference(name, iscal):
    """iscal = 1 is reset by the reference for conjugate gradients: the same result."""
    s = R.system(name)
    xr, ir = R.ref_solve(s["ia"], s["ja"], s["asym"], s["b"], iaccel=-1, iscal=iscal)
    x, it = R.cg(s["ia"], s["ja"], s["asym"], s["b"])
    assert ir > 0 and it == ir and _bit(x, xr), (it, ir)
    if iscal == 0:
        tol = np.full(len(xr), 1e-3)
        xr, ir = R.ref_solve(s["ia"], s["ja"], s["asym"], s["b"], iaccel=-1, toler=tol, resid_reduc=1e-30)
        x, it = R.cg(s["ia"], s["ja"], s["asym"], s["b"], toler=tol, resid_reduc=1e-30)
        assert ir > 0 and it == ir and _bit(x, xr), (it, ir)


@needs_ref
@pytest.mark.parametrize("name", R.SMALL)
@pytest.mark.parametrize("iaccel", [0, 1])
def test_row_scaling_equals_reference(name, iaccel):
    s = R.system(name)
    xr, ir = R.ref_solve(s["ia"], s["ja"], s["abad"], s["bbad"], iaccel=iaccel, iscal=1)
    if iaccel == 1:
        x, it = R.orthomin(s["ia"], s["ja"], s["abad"], s["bbad"], north=10, iscal=1)
    else:  # CG-STAB (the oracle's restatement) on the host-scaled system
        a2, b2, _ = R.scal(s["ia"], s["ja"], s["abad"], s["bbad"])
        x, it, _ = L.solve(s["ia"], s["ja"], a2, b2, resid_reduc=R.RESID)
    assert ir > 0 and it == ir and _bit(x, xr), (it, ir)


@pytest.mark.parametrize("n", [1, 100, 256, 257, 626, 70000])
def test_tree_sum_equals_plain_loops(n):
    t = np.random.default_rng(n).uniform(-1, 1, n)
    assert R.tree_sum(t) == R.tree_sum_loops(t)
