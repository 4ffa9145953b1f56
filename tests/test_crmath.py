"""crmath.h's correctly rounded powers on the host against __float128 powq, with arguments that put
the power within 2^-95 of a rounding midpoint, so that cr_resolve and the xp:: expansion arithmetic
(the exact decision) run: tests/cpp/crmath_check.cpp on the argument sets of tests/crmath_args.py.

Compiled with g++, not ROCm's clang++ as tests/test_markstein_host.py is: the program needs
libquadmath and its header, which ship with GCC (ROCm's clang has no quadmath.h of its own).  The
flags are the device translation units': -mfma -ffp-contract=off (explicit fma only).

The device counterpart is tests/test_gpu_crmath.py.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import crmath_args as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = tmp_path_factory.mktemp("crmath") / "crmath_check"
    subprocess.run([gxx, "-std=c++17", "-O2", "-mfma", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "crmath_check.cpp"), "-lquadmath"], check=True,
                   capture_output=True, text=True)
    return str(exe)


def _run(checker, tmp_path, mode, i, x):
    f = tmp_path / f"{mode}{i}.bin"
    np.ascontiguousarray(x, dtype=np.float64).tofile(f)
    r = subprocess.run([checker, mode, str(i), str(f)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    lines = r.stdout.splitlines()
    w = lines[-1].split()
    assert w[0] == "ok" and int(w[1]) == len(x), lines[-1]
    hard = [ln.split()[1:] for ln in lines[:-1]]
    assert len(hard) == int(w[5]) and all(ln.startswith("hard ") for ln in lines[:-1])
    return int(w[3]), hard


@pytest.mark.parametrize("i", range(4), ids=[op["name"] for op in A.OPS])
def test_exact_powers_match_powq_and_ties_are_reached(checker, tmp_path, i):
    """In range: exact == RN(powq) and fast == the same or tie (asserted by the program); the
    arguments whose quad power is within 2^-110 of a midpoint (exact ties above all) are decided
    here in rational arithmetic.  At least MIN_TIES arguments must raise tie: without them the test
    would pass without cr_resolve ever running."""
    op = A.OPS[i]
    ties, hard = _run(checker, tmp_path, "in", i, A.in_range(op))
    print(f"{op['name']}: {ties} ties, {len(hard)} decided exactly")
    for xb, eb, fb, tie in hard:
        x, ex, fa = (np.array([int(b, 16)], dtype=np.uint64).view(np.float64)[0] for b in (xb, eb, fb))
        assert A.correctly_rounded(x, op["num"], op["den"], ex), (float(x).hex(), float(ex).hex())
        assert tie == "1" or fb == eb, (float(x).hex(), float(fa).hex())
    assert ties >= A.MIN_TIES, ties


@pytest.mark.parametrize("i", range(4), ids=[op["name"] for op in A.OPS])
def test_out_of_range_defers_to_libm(checker, tmp_path, i):
    """Outside the double-double range (bounds included): the fast path raises tie, the exact path
    is the library pow, within one ulp of powq (libm's contract, not correct rounding)."""
    _run(checker, tmp_path, "out", i, A.out_of_range(A.OPS[i]))


def test_exact_decision_helper():
    """correctly_rounded itself, on roundings known by construction"""
    assert A.correctly_rounded(4.0, 3, 2, 8.0) and not A.correctly_rounded(4.0, 3, 2, np.nextafter(8.0, 9))
    m = 208065.0  # m^3 is an odd 54-bit integer: x^1.5 of m^2 is an exact tie, the even neighbour wins
    lo = float((208065 ** 3 // 2) * 2)
    even, odd = (lo, lo + 2) if (int(lo) // 2) % 2 == 0 else (lo + 2, lo)
    assert A.correctly_rounded(m * m, 3, 2, even) and not A.correctly_rounded(m * m, 3, 2, odd)
    assert A.correctly_rounded(2.0, -1, 2, 0.5 ** 0.5)
