"""Writes tests/golden/lasolver_order/*.npz from the reference build (oracle/_ref/liblasolver_ref.so:
its rcm() under its C++ name, and lsr_solve with ParamIter.order = 1) for the three small systems of
tests/accel_restate.py.  Data only: the reference's RCM ordering and, per setting, its x and nitr,
plus the sums of the generated values as a guard against generator drift (the systems are
regenerated from their seeds, never stored).

  lorder      rcm(ia, ja): lorder[new] = old
  cgs         iaccel 0 (CG-STAB), resid_reduc 1e-8
  omin        iaccel 1 (north 10: the C entry point fixes it)
  cg          iaccel -1 on the symmetric values
  scal_cgs    iaccel 0 with iscal 1 on the rows rescaled by 10**U(-3, 3)
  default     ParamIter's defaults, all of them (order 1, level 1, iscal 1, nitmax 30, resid_reduc 1e-6)

patterns.npz holds lorder alone for the two patterns of tests/order_restate.py ORDER_PATTERNS (a
nonsymmetric one that takes the symmetrise path, a path-like one on which the pseudo-peripheral
search moves the root twice), with their ia / ja.

Run from the repository root after __graft_entry__.build() where the reference checkout is present:
    python tests/golden/make_lasolver_order_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import accel_restate as R  # noqa: E402
import order_restate as O  # noqa: E402


def main():
    out = os.path.join(HERE, "lasolver_order")
    os.makedirs(out, exist_ok=True)
    for name in R.SMALL:
        s = R.system(name)
        ia, ja, b = s["ia"], s["ja"], s["b"]
        runs = {
            "cgs": O.ref_solve(ia, ja, s["a"], b, iaccel=0),
            "omin": O.ref_solve(ia, ja, s["a"], b, iaccel=1),
            "cg": O.ref_solve(ia, ja, s["asym"], b, iaccel=-1),
            "scal_cgs": O.ref_solve(ia, ja, s["abad"], s["bbad"], iaccel=0, iscal=1),
            "default": O.ref_solve(ia, ja, s["a"], b, iaccel=0, iscal=1, level=1, nitmax=30, resid_reduc=1e-6),
        }
        d = {"lorder": O.ref_rcm(ia, ja), "a_sum": s["a"].sum(), "asym_sum": s["asym"].sum(),
             "abad_sum": s["abad"].sum(), "b_sum": b.sum(), "bbad_sum": s["bbad"].sum()}
        for k, (x, nitr) in runs.items():
            assert nitr > 0, (name, k, nitr)
            d[k + "_x"] = x
            d[k + "_nitr"] = np.int32(nitr)
        np.savez(os.path.join(out, name + ".npz"), **d)
        print(name, {k: v[1] for k, v in runs.items()})
    d = {}
    for name, make in O.ORDER_PATTERNS.items():
        ia, ja = make()
        d[name + "_ia"], d[name + "_ja"], d[name + "_lorder"] = ia, ja, O.ref_rcm(ia, ja)
    np.savez(os.path.join(out, "patterns.npz"), **d)
    print("patterns", {k: len(v) for k, v in d.items()})


if __name__ == "__main__":
    main()
