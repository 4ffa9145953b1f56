"""Arguments that put crmath.h's powers near rounding midpoints, shared by tests/test_crmath.py
(host, against __float128 powq) and tests/test_gpu_crmath.py (device, against the oracle's crpow),
and the exact rounding decision in integer arithmetic.  Test infrastructure only.

A random argument reaches cr_resolve (the exact decision within 2^-95 of a midpoint) with
probability ~2^-42; these do it systematically:
  * 1 + k 2^-52 and 1 + k 2^-53, |k| <= 64: x^y = 1 + y k 2^-52 + O(2^-92), a midpoint or a double
    up to the second-order term;
  * k^2, k^4, (k + 1/2)^2, k < 3000, with both neighbours: perfect powers and their first-order
    neighbourhoods;
  * m^2 4^j and m^4 16^j with m chosen so that m^3, m^5 or m^9 is an odd 54-bit integer: x^1.5,
    x^1.25, x^2.25 are then EXACT ties (round to even);
  * (1 + k 2^-52) 2^e and (1 + k 2^-53) 2^e, |k| <= 200, at the exponents e next to each power's
    double-double range (MMX_CR_RANGE), and the doubles next to the range bounds;
  * random arguments.
"""
from fractions import Fraction

import numpy as np

# exact op, fast op (mmadmm_devmath), exponent y = num / den, MMX_CR_RANGE (lo, hi), edge exponent e
OPS = (
    dict(name="p15", exact=1, fast=6, y=1.5, num=3, den=2, lo=1e-90, hi=1e90, e=296, e_out=(300, 420)),
    dict(name="m05", exact=2, fast=7, y=-0.5, num=-1, den=2, lo=1e-100, hi=1e100, e=328, e_out=(333, 600)),
    dict(name="p225", exact=3, fast=8, y=2.25, num=9, den=4, lo=1e-30, hi=1e30, e=96, e_out=(100, 200)),
    dict(name="p125", exact=4, fast=9, y=1.25, num=5, den=4, lo=1e-50, hi=1e50, e=164, e_out=(167, 500)),
)
MIN_TIES = 15  # per op: fewer near-midpoint arguments would let cr_resolve go untested


def _near_one(kmax):
    k = np.arange(-kmax, kmax + 1, dtype=np.float64)
    return np.concatenate([1.0 + k * 2.0 ** -52, 1.0 + k * 2.0 ** -53])


def common(n_random=6000, seed=7):
    k = np.arange(1.0, 3000.0)
    pp = np.concatenate([k ** 2, k ** 4, (k + 0.5) ** 2])
    pp = np.concatenate([np.nextafter(pp, 0), pp, np.nextafter(pp, np.inf)])
    # exact ties: m^3 (m in (2^(53/3), 2^18]), m^5 (m in (2^10.6, 2^10.8]), m^9 (m = 61, 63) odd, 54 bits
    m2 = 208065.0 + 2.0 * 67.0 * np.arange(400.0)
    m4 = np.concatenate([np.arange(57.0, 66.0, 2.0), np.arange(1553.0, 1782.0, 2.0)])
    ties = [m2 ** 2 * 4.0 ** j for j in (-2, 0, 3)] + [m4 ** 4 * 16.0 ** j for j in (-2, 0, 3)]
    rng = np.random.default_rng(seed)
    return np.concatenate([_near_one(64), pp] + ties + [np.exp(rng.uniform(-20, 20, n_random))])


def in_range(op, n_random=6000):
    """every argument of op's check, strictly inside its MMX_CR_RANGE"""
    edge = np.concatenate([_near_one(200) * 2.0 ** e for e in (op["e"], -op["e"])])
    x = np.concatenate([common(n_random), edge, [np.nextafter(op["lo"], np.inf), np.nextafter(op["hi"], 0)]])
    assert ((x > op["lo"]) & (x < op["hi"])).all()
    return x


def out_of_range(op):
    """arguments outside the range (the bounds themselves included: the range is open)"""
    x = [np.array([op["lo"], op["hi"], np.nextafter(op["lo"], 0), np.nextafter(op["hi"], np.inf)])]
    for e in op["e_out"]:
        x += [_near_one(20) * 2.0 ** e, _near_one(20) * 2.0 ** -e]
    x = np.concatenate(x)
    assert (~((x > op["lo"]) & (x < op["hi"]))).all()
    return x


def _cmp_pow(x, num, den, m):
    """sign(x^(num/den) - m) for doubles x, m > 0, exactly (the comparison cr_resolve makes)"""
    X, M = Fraction(x), Fraction(m)
    d = X ** num - M ** den if num > 0 else 1 - M ** den * X ** (-num)
    return (d > 0) - (d < 0)


def correctly_rounded(x, num, den, r):
    """Is r = RN(x^(num/den)), ties to even?  Exact rational arithmetic (r normal, > 0)."""
    x, r = float(x), float(r)
    lo, hi = np.nextafter(r, 0), np.nextafter(r, np.inf)
    even = (np.float64(r).view(np.uint64) & np.uint64(1)) == 0
    below = _cmp_pow(x, num, den, Fraction(lo) / 2 + Fraction(r) / 2)  # v against the lower midpoint
    above = _cmp_pow(x, num, den, Fraction(r) / 2 + Fraction(hi) / 2)
    return (below > 0 or (below == 0 and even)) and (above < 0 or (above == 0 and even))
