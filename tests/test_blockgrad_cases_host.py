"""What the inputs of tests/test_gpu_blockgrad.py (tests/blockgrad_cases.py) cover, checked on the
host against a restatement of findLimInf (src/MeshUtils.h:45-54: (int) cast, then uint32 clamp): the
edge list must visit every monitor cell of every axis, reach the
top cell through the clamp from below the grid (a negative offset) and from above it, and stay
within 0.25 of the grid; the oracle must report the inverted and zero-volume simplices as NaN."""
import numpy as np
import pytest

import blockgrad_cases as C
import huang_mp as H


def find_lim_inf(w, lines):
    q = int((w - lines[0]) / (lines[1] - lines[0]))  # truncation toward zero, as the C cast
    guess = q & 0xFFFFFFFF
    return min(guess, len(lines) - 2)


@pytest.mark.parametrize("name", list(C.CONFIGS))
def test_edge_cases_cover_every_cell_and_the_clamp(name):
    mesh, O = C.make_oracle(name)
    F, lines = O.F(), C.grid_lines(mesh, O)
    D = mesh.dim
    assert all(len(g) - 1 == n for g, n in zip(lines, O.gridN))
    cases = C.edge_cases(name, mesh, F, lines)
    for ax in range(D):
        g = lines[ax]
        top = len(g) - 2
        hit, below_to_top, below_to_zero, above_to_top = set(), 0, 0, 0
        for label, sid, z, dx in cases:
            if not label.startswith(f"axis{ax}_"):
                continue
            assert H.edet(D, z) > 0
            col = z.reshape(D + 1, D)[:, ax]
            assert col.min() >= g[0] - C.OUTSIDE and col.max() <= g[-1] + C.OUTSIDE
            for w in col:
                i = find_lim_inf(w, g)
                hit.add(i)
                below_to_top += w < g[0] and i == top
                below_to_zero += w < g[0] and i == 0
                above_to_top += w > g[-1] and i == top
        assert hit == set(range(top + 1)), (ax, sorted(hit))
        assert below_to_top and below_to_zero and above_to_top


@pytest.mark.parametrize("name", ["rect2d10_mex3", "rect3d4_aniso6"])
def test_bad_cases_are_reported_by_the_oracle(name):
    mesh, O = C.make_oracle(name)
    F = O.F()
    kinds = set()
    for label, kind, sid, z, dx in C.bad_cases(mesh, F):
        kinds.add(kind)
        e, g, _ = O.block_grad(sid, z, dx, True, True)
        assert np.isnan(e), label
        fixed = np.repeat(mesh.mask[F[sid]] == 1, mesh.dim)
        assert np.isnan(g[~fixed]).all() and not g[fixed].any(), label
    assert kinds == set(C.BAD_KINDS)
