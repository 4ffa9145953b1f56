"""The device Huang energy and gradient of ONE simplex (blockGrad in csrc/kernels/admm_device.h,
through mmadmm_debug_blockgrad / Engine.block_grad) against the CPU oracle's blockGrad with
correctly rounded pow: energy, Igt and all K gradient entries bit for bit, at the inputs whole ADMM
steps on well-shaped meshes never produce (tests/blockgrad_cases.py): vertices on, one ulp beside
and outside the monitor grid's lines (findLimInf's (uint32_t)(int) clamp sends a negative offset to
the top cell -- the reference's behaviour), slivers down to aspect 1e-9, inverted, zero-volume and
NaN simplices, every GRAD/REG combination, FIXED-row zeroing, and the isotropic-grid branch against
the full rows on the same input (MMX_ISO).

Bookkeeping differs: the oracle writes Igt only with computeGrad and a valid element, so Igt is
compared only then; with computeGrad false both sides leave the gradient at zeros.
"""
import numpy as np
import pytest

import blockgrad_cases as C
import huang_mp as H
import mmadmm_amd as mx
import oracle_py

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _pow_mode():
    oracle_py.set_pow_mode(1)
    yield
    oracle_py.set_pow_mode(0)


def make_engine(name, mesh):
    _, mon, comp, _ = C.CONFIGS[name]
    M = mx.Mesh(mesh.Vp, mesh.F, mesh.mask, mx.BuiltinMonitor(mesh.dim, mon), rho=C.RHO, tau=C.TAU,
                Xc=mesh.Vp.copy() if comp else None)
    return mx.Engine(M, C.DT)


def make_all(name, monkeypatch):
    """-> (mesh, oracle, F, {label: engine}): an isotropic grid gets one engine per MMX_ISO value"""
    mesh, O = C.make_oracle(name)
    engines = {}
    if C.CONFIGS[name][3]:
        for flag in ("1", "0"):
            monkeypatch.setenv("MMX_ISO", flag)
            engines["iso" + flag] = make_engine(name, mesh)
            assert engines["iso" + flag].stats()["monitor_iso"] == int(flag)
        monkeypatch.delenv("MMX_ISO")
    else:
        engines["rows"] = make_engine(name, mesh)
        assert engines["rows"].stats()["monitor_iso"] == 0
    F = O.F()
    for G in engines.values():
        np.testing.assert_array_equal(G.simplices(), F)
        np.testing.assert_array_equal(G.get("grid"), O.get("grid"))
    return mesh, O, F, engines


def bits(a):
    """the bit patterns, every NaN as one pattern: NaN POSITIONS and signed zeros count, a NaN's sign
    and payload do not (the invalid operations of x86 produce -NaN, those of the device +NaN: a
    vertex far outside the grid extrapolates a monitor that is not positive definite, and the
    square root of its negative determinant is NaN on both sides)"""
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def packed(res, with_igt):
    """(energy, grad, Igt) -> one array (Igt only where both sides define it)"""
    e, g, igt = res
    return np.concatenate([[e], [igt] if with_igt else [], g])


def check_bitwise(O, engines, cases, flags=C.FLAGS):
    """every engine equals the oracle (hence each other) on every case and flag combination"""
    for label, sid, z, dx in cases:
        for grad, reg in flags:
            ref = packed(O.block_grad(sid, z, dx, grad, reg), grad)
            for ename, G in engines.items():
                got = packed(G.block_grad(sid, z, dx, grad, reg), grad)
                np.testing.assert_array_equal(bits(got), bits(ref),
                                              err_msg=f"{label} grad={grad} reg={reg} engine={ename}")
            if not grad:
                assert not ref[1:].any()  # the gradient stays at zeros


@pytest.mark.parametrize("name", list(C.CONFIGS))
def test_shapes_flags_and_fixed_rows_bitwise(name, monkeypatch):
    """0, 1 and D FIXED vertices x slivers of aspect 1 .. 1e-9 x the four GRAD/REG combinations
    (dxpu != z), and the device against the 200-bit restatement at s = 1 and 1e-3 to the bound of
    tests/test_blockgrad_mp_host.py (64 u / s), so a drift of oracle and kernel together shows."""
    mesh, O, F, engines = make_all(name, monkeypatch)
    cases = C.shape_cases(name, mesh, F)
    assert sorted({C.fixed_count(mesh, F, c[1]) for c in cases}) == [0, 1, mesh.dim]
    check_bitwise(O, engines, cases)
    D = mesh.dim
    G = next(iter(engines.values()))
    for (label, sid, z, dx), s in zip(cases, H.SLIVERS * 3):
        if s < 1e-3:
            continue
        mons = [O.eval_monitor(z[i * D:(i + 1) * D]) for i in range(D + 1)]
        xi = mesh.Vp[F[sid]].reshape(-1) if C.CONFIGS[name][2] else None
        for reg in (False, True):
            e_mp, igt_mp, g_mp = H.block_grad_mp(D, len(F), z, mons, dx if reg else None,
                                                 0.5 * np.sqrt(C.RHO) if reg else None, xi)
            for n in range(D + 1):
                if mesh.mask[F[sid][n]] == 1:
                    g_mp[D * n:D * n + D] = [H.mpf(0)] * D
            e, g, igt = G.block_grad(sid, z, dx, True, reg)
            ee, ge = H.rel_errors(e, g, e_mp, g_mp)
            ie = H.rel_errors(igt, g, igt_mp, g_mp)[0]
            print(f"{name} {label} reg={reg}: energy {ee:.2e} Igt {ie:.2e} gradient {ge:.2e}")
            assert max(ee, ie, ge) <= 64 * H.U / s, (label, reg, ee, ie, ge)


@pytest.mark.parametrize("name", list(C.CONFIGS))
def test_monitor_cell_edges_bitwise(name, monkeypatch):
    """One vertex on, and one ulp either side of, every grid line of every axis, both ends of the
    axis, up to 0.25 outside the grid on both sides and the smallest subnormal above its origin:
    the findLimInf / gridCoord / div_nr path, in 3D monLoad3 / monEval3 and their isotropic twins."""
    mesh, O, F, engines = make_all(name, monkeypatch)
    cases = C.edge_cases(name, mesh, F, C.grid_lines(mesh, O))
    check_bitwise(O, engines, cases, flags=[(True, True), (False, False)])


BAD = ["rect2d10_mex3", "hexdisc12_mex2", "rect3d4_aniso6", "circle3d6_compmesh"]


@pytest.mark.parametrize("name", BAD)
def test_inverted_zero_volume_and_nan_simplices_bitwise(name, monkeypatch):
    """Two vertices swapped, a repeated vertex (Edet = 0 exactly) and a NaN coordinate: NaN energy,
    NaN gradient except the zeroed FIXED rows, identical on both sides (fresh engines: the inverted
    flag these leave set must not reach another test)."""
    mesh, O, F, engines = make_all(name, monkeypatch)
    D = mesh.dim
    for label, kind, sid, z, dx in C.bad_cases(mesh, F):
        for grad, reg in C.FLAGS:
            e_o, g_o, _ = O.block_grad(sid, z, dx, grad, reg)
            want = np.zeros(D * (D + 1))
            if grad:
                want[:] = np.nan
                for n in range(D + 1):
                    if mesh.mask[F[sid][n]] == 1:
                        want[D * n:D * n + D] = 0.0
            assert np.isnan(e_o), label
            np.testing.assert_array_equal(np.isnan(g_o), np.isnan(want), err_msg=label)
            for ename, G in engines.items():
                e, g, _ = G.block_grad(sid, z, dx, grad, reg)
                np.testing.assert_array_equal(bits(np.concatenate([[e], g])), bits(np.concatenate([[e_o], g_o])),
                                              err_msg=f"{label} grad={grad} reg={reg} engine={ename}")
    for G in engines.values():
        G.close()


class _HalfNanMonitor(mx.MonitorFunction):
    """identity left of x = 0.6, NaN right of it: every step's energy is NaN with no element inverted"""
    dim = 2

    def __call__(self, x, M):
        M[:] = np.nan if x[0] > 0.6 else np.eye(2)


@pytest.mark.parametrize("kind", ["swapped", "repeated", "nan"])
def test_inverted_flag_set_by_finite_edet_only(kind):
    """GridView::invFlag: a blockGrad that meets a finite Edet <= 0 sets it, a NaN Edet (NaN
    positions) does not.  A step reads the flag when its energy is not finite, to tell an inverted
    element from a non-finite monitor value -- so on an engine whose monitor is NaN on part of the
    domain (the step fails either way, with no element inverted by the step itself) the step after
    a finite Edet <= 0 evaluation reports the inverted-element error and the step after the
    NaN-coordinate evaluation alone reports the non-finite one."""
    m = mx.MeshData.rect(2, 12)
    G = mx.Engine(mx.Mesh(m.Xp, m.F, m.mask, _HalfNanMonitor(), rho=50.0, tau=0.5), 0.055)
    mesh = oracle_py.Mesh(2, m.Xp, G.simplices(), m.mask)
    sid = next(i for i in range(len(mesh.F)) if mesh.Vp[mesh.F[i]][:, 0].max() < 0.4)
    z = C.bad_simplex(kind, mesh.Vp[mesh.F[sid]])
    dx = np.where(np.isnan(z), 0.5, z) + 0.003
    e, g, _ = G.block_grad(sid, z, dx, True, False)
    assert np.isnan(e)
    with pytest.raises(mx.NonFiniteEnergyError if kind == "nan" else mx.InvertedElementError):
        G.step(5, -1.0)
    G.close()


def test_nan_coordinate_leaves_a_good_engine_usable(monkeypatch):
    """after the NaN-coordinate evaluation alone a step on a sound mesh reports nothing"""
    name = "rect2d10_mex3"
    mesh, O, F, engines = make_all(name, monkeypatch)
    case = next(c for c in C.bad_cases(mesh, F) if c[1] == "nan")
    G = engines["iso1"]
    assert np.isnan(G.block_grad(case[2], case[3], case[4], True, True)[0])
    ih_o, ih_g = O.step(5, -1.0)[0], G.step(5, -1.0)[0]
    assert abs(ih_g - ih_o) <= 1e-12 * abs(ih_o)
    np.testing.assert_array_equal(G.get("x"), O.get("x"))
    for G in engines.values():
        G.close()
