"""An object's MMX_* switches are fixed when it is created (mm-admm_amd/csrc/host/knobs.h): two
objects with different options live side by side, a regrid does not re-read the environment, and
the switches that used to be read once per process can be forced per object.  Engine.options() and
MatrixIter.options() report the resolved values."""
import numpy as np
import pytest

import lasolver_py as L
import mmadmm_amd as mx
import oracle_py
from test_gpu_parity import ISO_CASES, cases, make_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _pow_mode_reset():
    yield
    oracle_py.set_pow_mode(0)


@pytest.mark.parametrize("name", ["hexdisc12_mex1", "rect3d_3_mex1"])
def test_two_engines_different_options(name, monkeypatch):
    """G is created before MMX_RED_SPLIT_MIN=1 is set, Gs under it, and both step after it is gone:
    G keeps the one-workgroup reductions, Gs the split ones, and they agree as
    test_split_reductions_small_mesh asks."""
    mk, mon, dt, tau, rho, comp = cases()[name]
    mesh = mk()
    O, G = make_pair(mesh, mon, dt, tau, rho, comp, 1, 1)
    monkeypatch.setenv("MMX_RED_SPLIT_MIN", "1")
    _, Gs = make_pair(mesh, mon, dt, tau, rho, comp, 1, 1)
    _, Gs2 = make_pair(mesh, mon, dt, tau, rho, comp, 1, 1)
    monkeypatch.delenv("MMX_RED_SPLIT_MIN")
    assert G.options()["MMX_RED_SPLIT_MIN"] == "4096" and Gs.options()["MMX_RED_SPLIT_MIN"] == "1"
    for s in range(3):
        for tol in (-1.0, 1e-3):  # the deferred whole-step reduction and the per-iteration one
            ih_o, it_o = O.step(5, tol)[:2]
            ih_g, it_g = G.step(5, tol)
            ih_s, it_s = Gs.step(5, tol)
            ih_s2, it_s2 = Gs2.step(5, tol)
            assert it_s == it_g == it_o and ih_s == ih_s2
            assert abs(ih_s - ih_o) <= 1e-12 * abs(ih_o) and abs(ih_s - ih_g) <= 1e-12 * abs(ih_g)
    assert G.options()["MMX_RED_SPLIT_MIN"] == "4096" and Gs.options()["MMX_RED_SPLIT_MIN"] == "1"
    np.testing.assert_array_equal(Gs.get("x"), O.get("x"))
    assert Gs.stats()["bfgs_iters"] == O.bfgs_iters() == Gs2.stats()["bfgs_iters"]
    assert Gs.stats()["last_primal"] == Gs2.stats()["last_primal"]


def _regrid_engine(name):
    mk, mon, dt, tau, rho, _ = ISO_CASES[name]
    mesh = mk()
    E = mx.Engine(mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(mesh.dim, mon), rho=rho, tau=tau), dt)
    E.set_regrid(True)
    return E


@pytest.mark.parametrize("name,knob,value", [("hexdisc40_movingbump", "MMX_ISO", "0"),
                                             ("rect3d_8_movingbump", "MMX_ISO", "0"),
                                             ("hexdisc40_movingbump", "MMX_FORCE_TIE", "2")])
def test_options_survive_a_regrid(name, knob, value, monkeypatch):
    """MonType 7 rebuilds the monitor grid, and with it the kernels' view of the engine, at every
    step.  A was created under the switch, which is gone before the first step: A keeps its form
    through the rebuilds (the full grid rows; every second prox block recomputed exactly) and its
    state equals the default engine's bit for bit."""
    monkeypatch.setenv(knob, value)
    A = _regrid_engine(name)
    monkeypatch.delenv(knob)
    B = _regrid_engine(name)
    before = A.options()
    assert before[knob] == value and B.options()[knob] != value
    for _ in range(3):
        A.step(5, -1.0)
        B.step(5, -1.0)
    assert A.stats()["regrids"] == 3
    assert A.options() == before
    assert A.stats()["monitor_iso"] == (0 if knob == "MMX_ISO" else 1) and B.stats()["monitor_iso"] == 1
    for f in ("x", "z", "u", "hess"):
        np.testing.assert_array_equal(A.get(f), B.get(f), err_msg=f)
    A.close()
    B.close()


def test_two_matrices_different_options(monkeypatch):
    """A is created under MMX_SWEEP=level and MMX_FACTOR=level, B after they are gone; sfac and the
    solves come later.  A runs the level-scheduled factor and sweeps, B the chain-scheduled ones, and
    factor, ILU solve and CG-STAB iterates agree bit for bit (as test_chain_sweeps_equal_level_sweeps
    and the factor tests of test_gpu_lasolver.py ask of these modes)."""
    import torch  # noqa: F401  (same HIP runtime as the library)
    import lasolver_amd as la

    m = oracle_py.Mesh.rect(2, 20)
    ia, ja = L.mesh_pattern(2, m.nP, m.F)
    N = len(ia) - 1
    rng = np.random.default_rng(7)
    a = rng.uniform(-1, 1, len(ja))
    d = np.nonzero(ja == np.repeat(np.arange(N), np.diff(ia)))[0]
    a[d] = np.add.reduceat(np.abs(a), ia[:-1]) * 0.3 + 1.0
    b = rng.uniform(-1, 1, N)

    def create():
        M = la.MatrixIter(N, ia, ja)
        M.a[:] = a
        M.b[:] = b
        return M

    monkeypatch.setenv("MMX_SWEEP", "level")
    monkeypatch.setenv("MMX_FACTOR", "level")
    A = create()
    monkeypatch.delenv("MMX_SWEEP")
    monkeypatch.delenv("MMX_FACTOR")
    B = create()
    assert (A.options()["MMX_SWEEP"], A.options()["MMX_FACTOR"]) == ("level", "level")
    assert (B.options()["MMX_SWEEP"], B.options()["MMX_FACTOR"]) == ("chain", "auto")
    out = []
    for M in (A, B):
        p = la.ParamIter.mesh()
        M.sfac(p)
        M.factor()
        af = M.get_factor()[2]
        y = M.ilu_solve(b)
        x = np.zeros(N)
        it = M.solve(p, x)
        out.append((af, y, x, it, M.stats()))
    (af_a, y_a, x_a, it_a, st_a), (af_b, y_b, x_b, it_b, st_b) = out
    assert st_a["sweep_mode"] == 0 and st_a["factor_mode"] == 0 and st_b["sweep_mode"] == 1
    assert it_a == it_b and it_a > 0
    assert np.array_equal(af_a, af_b) and np.array_equal(y_a, y_b) and np.array_equal(x_a, x_b)
    assert A.options()["MMX_SWEEP"] == "level" and B.options()["MMX_SWEEP"] == "chain"
    A.close()
    B.close()


def test_formerly_process_static_switches_per_engine(monkeypatch):
    """MMX_GRAD_CACHE and MMX_PROX_BLOCK were read once per process: now an engine created under
    them recomputes the entry gradient and runs the prox in workgroups of 128, in a process whose
    other engines do neither, and stays bit-identical to the oracle (as test_steps_bitwise)."""
    mk, mon, dt, tau, rho, comp = cases()["hexdisc12_mex1"]
    mesh = mk()
    monkeypatch.setenv("MMX_GRAD_CACHE", "0")
    monkeypatch.setenv("MMX_PROX_BLOCK", "128")
    O, G = make_pair(mesh, mon, dt, tau, rho, comp, 1, 1)
    monkeypatch.delenv("MMX_GRAD_CACHE")
    monkeypatch.delenv("MMX_PROX_BLOCK")
    _, D = make_pair(mesh, mon, dt, tau, rho, comp, 1, 1)
    assert (G.options()["MMX_GRAD_CACHE"], G.options()["MMX_PROX_BLOCK"]) == ("0", "128")
    assert (D.options()["MMX_GRAD_CACHE"], D.options()["MMX_PROX_BLOCK"]) == ("1", "64")
    for s in range(3):
        ih_o = O.step(5, -1.0)[0]
        ih_g = G.step(5, -1.0)[0]
        assert abs(ih_o - ih_g) <= 1e-12 * abs(ih_o)
        for f in ("x", "z", "u", "xBar", "xPrev"):
            np.testing.assert_array_equal(G.get(f), O.get(f), err_msg=f"{f} step {s}")
    np.testing.assert_array_equal(G.get("hess"), O.get("hess"))
    assert G.stats()["bfgs_iters"] == O.bfgs_iters()
    assert (G.options()["MMX_GRAD_CACHE"], G.options()["MMX_PROX_BLOCK"]) == ("0", "128")


def test_xup_sweep_above_its_buffer_is_refused(monkeypatch):
    """The sweep's residual form writes 256 x MMX_XUP_SWEEP partial records; a small mesh's buffer
    holds 4096, so 16 is the most it takes: 17 fails the construction with MMADMM_ERR_INVALID and
    names the variable, 16 builds and steps."""
    mesh = mx.MeshData.rect(3, 3)
    M = mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(3, 1), rho=50.0, tau=0.5)
    monkeypatch.setenv("MMX_XUP_SWEEP", "17")
    with pytest.raises(mx.MMADMMError) as e:
        mx.Engine(M, 0.025)
    assert e.value.code == 1 and "MMX_XUP_SWEEP" in str(e.value)
    monkeypatch.setenv("MMX_XUP_SWEEP", "16")
    G = mx.Engine(M, 0.025)
    monkeypatch.delenv("MMX_XUP_SWEEP")
    assert G.options()["MMX_XUP_SWEEP"] == "16"
    ref = mx.Engine(M, 0.025)
    for _ in range(2):
        G.step(5, -1.0)
        ref.step(5, -1.0)
    np.testing.assert_array_equal(G.get("x"), ref.get("x"))
    G.close()
    ref.close()
