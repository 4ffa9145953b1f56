"""The hub meshes (tests/hub_meshes.py) on the host, no GPU: the generators' properties -- positive
orientation, conformity, sizes, hub valence, widest Jacobian row -- and every row of
tests/hub_cases.py run on the oracle alone with the correctly rounded pow, so that each GPU test of
tests/test_gpu_hub_meshes.py compares against a run that completes with finite values."""
import numpy as np
import pytest

import hub_cases as hc
import hub_meshes as hm
import oracle_py


@pytest.fixture(autouse=True)
def _pow_mode():
    oracle_py.set_pow_mode(1)
    yield
    oracle_py.set_pow_mode(0)


@pytest.mark.parametrize("name", list(hc.SIZES))
def test_generator_properties(name):
    m = hc.mesh(name)
    nP, nF, hub, cols = hc.SIZES[name]
    D = m.dim
    assert (m.nP, m.nF) == (nP, nF)
    assert m.F.min() == 0 and m.F.max() == nP - 1 and np.unique(m.F).size == nP
    assert (np.sort(m.F, axis=1)[:, 1:] != np.sort(m.F, axis=1)[:, :-1]).all(), "a simplex repeats a vertex"
    vol = hm.signed_volumes(m.Xp, m.F)
    assert (vol > 0).all(), f"{int((vol <= 0).sum())} simplices are not positively oriented"
    # the simplices fill the polygon / polyhedron of the outermost ring / shell
    outer = m.Xp[m.mask == hm.FIXED] - 0.5
    if D == 2:
        N = hub
        want = 0.5 * N * 0.45 ** 2 * np.sin(2 * np.pi / N)
    else:
        P, T = hm.sphere(*[int(v) for v in name.split("_")[1:3]])
        want = 0.45 ** 3 * np.einsum("ti,ti->t", P[T[:, 0]], np.cross(P[T[:, 1]], P[T[:, 2]])).sum() / 6.0
    fact = 2.0 if D == 2 else 6.0
    assert abs(vol.sum() / fact - want) <= 1e-12 * want  # <= 672 terms of a few roundings each
    assert np.allclose(np.sqrt((outer ** 2).sum(axis=1)), 0.45, rtol=0, atol=1e-15)
    # conformity: every (D-1)-face in one or two simplices, the single ones those of the outer boundary
    occ = hm.face_counts(m.F)
    assert occ.min() >= 1 and occ.max() <= 2
    n_boundary = hub if D == 2 else len(T)
    assert int((occ == 1).sum()) == n_boundary
    faces = np.concatenate([np.sort(np.delete(m.F, j, axis=1), axis=1) for j in range(D + 1)])
    uniq, cnt = np.unique(faces, axis=0, return_counts=True)
    assert (m.mask[uniq[cnt == 1]] == hm.FIXED).all(), "a boundary face has an interior node"
    assert int((m.mask == hm.FIXED).sum()) == (hub if D == 2 else len(P))
    assert set(np.unique(m.mask)) <= {hm.FIXED, hm.INTERIOR} and m.mask[0] == hm.INTERIOR
    val = hm.valence(m)
    assert val[0] == hub and val.argmax() == 0
    # the widest Jacobian row, from the oracle's pattern: the hub's
    O = hc.oracle(name, 1)
    O.backwards_euler_step(hc.DT, 1e-3, tree=True)
    ia = O.jacobian()[0]
    width = np.diff(ia)
    assert (width % D == 0).all()
    assert width.max() // D == cols and width.argmax() == 0
    assert np.array_equal(O.F(), m.F), "the oracle keeps the generators' orientation"


def test_shared_meshes_cover_every_remainder_of_the_chunk_of_four():
    rem = {hc.SIZES[n][2] % 4 for n in hc.SHARED_MESHES}
    assert rem == {0, 1, 2, 3}
    assert sorted(hc.SIZES[n][2] for n in hc.SHARED_MESHES) == [6, 7, 13, 64, 80, 100, 168]


@pytest.mark.parametrize("name,mon,gradUse", hc.ADMM, ids=[f"{n}-mon{m}-grad{int(g)}" for n, m, g in hc.ADMM])
def test_oracle_completes_admm(name, mon, gradUse):
    O = hc.oracle(name, mon, gradUse=gradUse)
    for tol in hc.TOLS:
        O.step(6, tol)
        assert hc.finite(O)


FIXED_ITERS = ([(n, m, 2, 10, False) for n, m in hc.XUP] + [(n, m, 2, hc.PROX_ITERS, False) for n, m in hc.PROX]
               + [(n, m, 5, 6, False) for n, m in hc.PARTITION]
               + [(n, m, 4, 6, True) for n, m in hc.REGRID])


@pytest.mark.parametrize("name,mon,steps,iters,regrid", FIXED_ITERS,
                         ids=[f"{n}-mon{m}-{s}x{i}" + ("-regrid" if r else "") for n, m, s, i, r in FIXED_ITERS])
def test_oracle_completes_fixed_iterations(name, mon, steps, iters, regrid):
    O = hc.oracle(name, mon, regrid=regrid)
    for _ in range(steps):
        O.step(iters, -1.0)
        assert hc.finite(O)
        assert not regrid or np.isfinite(O.get("grid")).all()


BE_ROWS = hc.BE + hc.BE_HARD


@pytest.mark.parametrize("name,mon,dt,rho", BE_ROWS, ids=[f"{n}-mon{m}" + ("-hard" if d else "") for n, m, d, r in BE_ROWS])
def test_oracle_completes_backward_euler(name, mon, dt, rho):
    O = hc.oracle(name, mon, dt, rho)
    dt = dt or hc.DT
    counts = []
    for s in range(3):
        if s == 2:
            O.done()
        counts.append(O.backwards_euler_step(dt, 1e-3, tree=True)[1])
        assert np.isfinite(O.get("x")).all()
    ia, ja, a = O.jacobian()
    assert np.isfinite(a).all() and np.diff(ia).max() // hc.mesh(name).dim == hc.BE_COLS[name]
    print(name, mon, "Newton iterations", counts)
    if dt != hc.DT:
        assert max(counts) >= 4, "the harder row was expected to take several Newton iterations"


@pytest.mark.parametrize("name,mon", hc.EULER, ids=[f"{n}-mon{m}" for n, m in hc.EULER])
def test_oracle_completes_euler(name, mon):
    O = hc.oracle(name, mon)
    for _ in range(3):
        assert np.isfinite(O.euler_step())
        assert np.isfinite(O.get("x")).all()


@pytest.mark.parametrize("name", list(hc.STATIONARY))
def test_oracle_fails_at_the_stationary_fan(name):
    """fan2d(N, 1) under the uniform monitor is stationary for these N: the prox gradient vanishes, the
    BFGS update divides by an underflowed (p . y)^2, x turns NaN and the oracle reports an inverted
    element in a known step.  The steps before it complete with finite values."""
    O = hc.oracle(name, 1)
    fails = hc.STATIONARY[name]
    for s, tol in enumerate(hc.TOLS[:hc.STATIONARY_STEPS]):
        if s == fails:
            with pytest.raises(RuntimeError, match="inverted element"):
                O.step(6, tol)
            break
        O.step(6, tol)
        assert hc.finite(O)
    else:
        pytest.fail("the oracle completed every step")
