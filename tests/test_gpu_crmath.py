"""The device's exact rounding decision (crmath.h cr_resolve and the xp:: expansion arithmetic, the
only non-inlined device functions, their arrays in scratch) under near-midpoint arguments.

tests/test_gpu_parity.py feeds the exact ops random arguments (which reach cr_resolve with
probability ~2^-42) and accepts a deferral from the fast ops without asking the exact ones; here
every argument of tests/crmath_args.py (the host check's list, tests/test_crmath.py) goes through
both: the exact op must equal the oracle's crpow bit for bit, the fast op must defer (NaN) on at
least MIN_TIES of them -- so cr_resolve ran on the device for those -- and equal the exact op
wherever it does not.  The list holds exact ties (m^2 4^j, m^4 16^j): those must round to even,
which equality with crpow asserts.
"""
import numpy as np
import pytest

import crmath_args as A
import mmadmm_amd as mx
import oracle_py

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("op", A.OPS, ids=[op["name"] for op in A.OPS])
def test_device_exact_path_resolves_near_midpoints(op):
    x = A.in_range(op, n_random=2000)
    ref = np.array([oracle_py.crpow(v, op["y"]) for v in x])
    exact = mx.devmath(op["exact"], x)
    fast = mx.devmath(op["fast"], x)
    deferred = np.isnan(fast)
    print(f"{op['name']}: {len(x)} arguments, {int(deferred.sum())} deferred by the fast path")
    np.testing.assert_array_equal(exact.view(np.uint64), ref.view(np.uint64))
    assert deferred.sum() >= A.MIN_TIES, int(deferred.sum())
    np.testing.assert_array_equal(fast[~deferred].view(np.uint64), exact[~deferred].view(np.uint64))
