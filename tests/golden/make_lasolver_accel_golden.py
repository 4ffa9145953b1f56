"""Writes tests/golden/lasolver_accel/*.npz from the reference build (oracle/_ref/liblasolver_ref.so,
lsr_solve: the reference's own MatrixIter::solve) for the three small systems of
tests/accel_restate.py.  Data only: per setting the reference's x and nitr, plus the sums of the
generated values as a guard against generator drift (the systems are regenerated from their seeds,
never stored).

  omin / omin_tol        iaccel 1 (north 10: the C entry point fixes it), resid_reduc 1e-8 / the toler rule
  cg / cg_tol            iaccel -1 on the symmetric values
  scal_cgs / scal_omin   iscal 1 with iaccel 0 / 1 on the rows rescaled by 10**U(-3, 3)
  default_l1             ParamIter's defaults with order 0 (level 1, iscal 1, nitmax 30, resid_reduc 1e-6)

Run from the repository root after __graft_entry__.build() where the reference checkout is present:
    python tests/golden/make_lasolver_accel_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import accel_restate as R  # noqa: E402


def main():
    out = os.path.join(HERE, "lasolver_accel")
    os.makedirs(out, exist_ok=True)
    for name in R.SMALL:
        s = R.system(name)
        ia, ja, b = s["ia"], s["ja"], s["b"]
        tol = np.full(len(b), 1e-3)
        runs = {
            "omin": R.ref_solve(ia, ja, s["a"], b, iaccel=1),
            "omin_tol": R.ref_solve(ia, ja, s["a"], b, iaccel=1, toler=tol, resid_reduc=1e-30),
            "cg": R.ref_solve(ia, ja, s["asym"], b, iaccel=-1),
            "cg_tol": R.ref_solve(ia, ja, s["asym"], b, iaccel=-1, toler=tol, resid_reduc=1e-30),
            "scal_cgs": R.ref_solve(ia, ja, s["abad"], s["bbad"], iaccel=0, iscal=1),
            "scal_omin": R.ref_solve(ia, ja, s["abad"], s["bbad"], iaccel=1, iscal=1),
            "default_l1": R.ref_solve(ia, ja, s["a"], b, iaccel=0, iscal=1, level=1, nitmax=30, resid_reduc=1e-6),
        }
        d = {"a_sum": s["a"].sum(), "asym_sum": s["asym"].sum(), "abad_sum": s["abad"].sum(), "b_sum": b.sum(),
             "bbad_sum": s["bbad"].sum()}
        for k, (x, nitr) in runs.items():
            assert nitr > 0, (name, k, nitr)
            d[k + "_x"] = x
            d[k + "_nitr"] = np.int32(nitr)
        np.savez(os.path.join(out, name + ".npz"), **d)
        print(name, {k: v[1] for k, v in runs.items()})


if __name__ == "__main__":
    main()
