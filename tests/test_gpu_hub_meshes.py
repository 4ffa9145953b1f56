"""Every node kernel on meshes with one high-valence hub and on tiny meshes (tests/hub_meshes.py).

The structured meshes of the other modules have at most 8 (2D) or 24 (3D) simplices at a node and
at most 27 column nodes in a Jacobian row, so the chunk tails of the x-update, the wide-row Jacobian
assembly (k_jac_assemble_s: rows of more than 64 column nodes) and prox launches of less than one
wavefront never ran.  Here node 0 has 5 .. 168 incident simplices.  The rows (mesh, monitor,
parameters) come from tests/hub_cases.py; tests/test_hub_meshes_host.py shows that the oracle
completes each of them.  The reference is the oracle with the correctly rounded pow; comparisons are
bit for bit, energies to 1e-12 relative.

* ADMM steps against the oracle, gradUse off and on (k_grad_simplex, k_predict mode 0);
* the x-update's forms (records / CSR, one node per lane / sweep, slot terms, node order, XCD map,
  chunk sizes) against the CSR one-node-per-lane form;
* the prox forms on 5, 63, 64, 65 and 672 simplices against the default;
* backward Euler: the Jacobian (64 column nodes: the widest row the wavefront assembly takes; 65,
  87 and 101: k_jac_assemble_s) and Newton steps against the oracle, the assembly forms against
  each other, the solver forms on the hub's rows of 130 / 202 / 261 entries;
* explicit Euler against the oracle;
* 2 and 4 loopback ranks against one: the hub is a local node with remote slots on every rank;
* the grid rebuilt at every step against the oracle;
* the stationary fan: the engine fails in the step in which the oracle fails."""
import threading

import numpy as np
import pytest

import hub_cases as hc
import mmadmm_amd as mx
import oracle_py
from test_gpu_parity import make_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _pow_mode_reset():
    yield
    oracle_py.set_pow_mode(0)


def pair(name, mon, dt=None, rho=None, gradUse=False):
    d, r = hc.params(name)
    return make_pair(hc.mesh(name), mon, dt or d, hc.TAU, rho or r, False, 1, 1, gradUse=gradUse)


def engine(name, mon):
    m = hc.mesh(name)
    dt, rho = hc.params(name)
    return mx.Engine(mx.Mesh(m.Xp, m.F, m.mask, mx.BuiltinMonitor(m.dim, mon), rho=rho, tau=hc.TAU), dt)


def same_energy(a, b):
    return abs(a - b) <= 1e-12 * abs(b)


# ---------------------------------------------------------------- (a) ADMM steps against the oracle
@pytest.mark.parametrize("name,mon,gradUse", hc.ADMM, ids=[f"{n}-mon{m}-grad{int(g)}" for n, m, g in hc.ADMM])
def test_admm_steps_bitwise_against_oracle(name, mon, gradUse):
    O, G = pair(name, mon, gradUse=gradUse)
    for s, tol in enumerate(hc.TOLS):
        ih_o, it_o = O.step(6, tol)[:2]
        ih_g, it_g = G.step(6, tol)
        assert it_o == it_g, f"step {s}: ADMM iterations {it_g}, oracle {it_o}"
        assert same_energy(ih_g, ih_o), f"step {s}: energy {ih_g}, oracle {ih_o}"
        for f in ("x", "z", "u"):
            a, b = G.get(f), O.get(f)
            assert np.array_equal(a, b), f"step {s}, {f}: {np.count_nonzero(a != b)} of {a.size} entries differ"
    assert G.stats()["bfgs_iters"] == O.bfgs_iters()
    G.close()


# ---------------------------------------------------------------- (b) x-update forms
def _state(name, mon, steps, iters, expect=None):
    G = engine(name, mon)
    if expect:
        opts = G.options()
        assert {k: opts[k] for k in expect} == expect
    ih = [G.step(iters, -1.0)[0] for _ in range(steps)]
    out = {f: G.get(f) for f in ("x", "xPrev", "xBar", "z", "u")}
    st = G.stats()
    out["ih"] = np.array(ih)
    out["primal"] = np.array([st["last_primal"], st["last_dual"]])
    out["bfgs"] = np.array([st["bfgs_iters"]])
    G.close()
    return out


CSR = {"MMX_XUP_REC": "0", "MMX_XUP_SWEEP": "0"}


def _xup_variants(dim):
    """One factor at a time around the default (the records; 2D: two sweep workgroups per CU, 3D:
    one and the slab order) and around the CSR walk, one node per lane.  The defaults themselves
    are the other value of each 0/1 switch: early 1, slot terms 1, XCD map 1, sweep residual 1,
    chunk 8; DEFAULTS asserts that."""
    flip = "1" if dim == 2 else "0"  # the node order that is not the dimension's default
    v = [("default", {}),
         ("rec-sweep0", {"MMX_XUP_SWEEP": "0"}), ("rec-sweep1", {"MMX_XUP_SWEEP": "1"}), ("rec-sweep2", {"MMX_XUP_SWEEP": "2"}),
         ("rec-early0", {"MMX_XUP_EARLY": "0"}), ("rec-tslot0", {"MMX_TSLOT": "0"}),
         ("rec-order" + flip, {"MMX_XUP_ORDER": flip}),  # 2D: the slab order together with the sweep
         ("rec-xcd0", {"MMX_XCD_MAP": "0"}), ("rec-resid0", {"MMX_XUP_SWEEP_RESID": "0"}),
         ("csr-sweep1", {"MMX_XUP_REC": "0", "MMX_XUP_SWEEP": "1"}), ("csr-sweep2", {"MMX_XUP_REC": "0", "MMX_XUP_SWEEP": "2"}),
         ("csr-tslot0", dict(CSR, MMX_TSLOT="0")), ("csr-order" + flip, dict(CSR, MMX_XUP_ORDER=flip)),
         ("csr-sweep1-order" + flip, {"MMX_XUP_REC": "0", "MMX_XUP_SWEEP": "1", "MMX_XUP_ORDER": flip}),
         ("csr-xcd0", dict(CSR, MMX_XCD_MAP="0")),
         ("csr-sweep1-resid0", {"MMX_XUP_REC": "0", "MMX_XUP_SWEEP": "1", "MMX_XUP_SWEEP_RESID": "0"})]
    if dim == 3:
        v += [("rec-ch16", {"MMX_XUP_CH": "16"}), ("rec-ch24", {"MMX_XUP_CH": "24"}),
              ("csr-sweep1-ch16", {"MMX_XUP_REC": "0", "MMX_XUP_SWEEP": "1", "MMX_XUP_CH": "16"}),
              ("csr-sweep1-ch24", {"MMX_XUP_REC": "0", "MMX_XUP_SWEEP": "1", "MMX_XUP_CH": "24"})]
    return v


DEFAULTS = {"MMX_XUP_REC": "1", "MMX_XUP_EARLY": "1", "MMX_TSLOT": "1", "MMX_XCD_MAP": "1", "MMX_XUP_SWEEP_RESID": "1",
            "MMX_XUP_CH": "8"}
XUP_RUNS = [(n, m, vid, env) for n, m in hc.XUP for vid, env in _xup_variants(hc.mesh(n).dim)]
_csr_state = {}


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _csr_reference(name, mon):
    """MMX_XUP_REC=0, one node per lane: computed once per mesh"""
    if name not in _csr_state:
        with pytest.MonkeyPatch.context() as mp:
            _setenv(mp, CSR)
            _csr_state[name] = _state(name, mon, 2, 10, expect=CSR)
    return _csr_state[name]


@pytest.mark.parametrize("name,mon,vid,env", XUP_RUNS, ids=[f"{n}-{v}" for n, _, v, _ in XUP_RUNS])
def test_xupdate_forms_equal_csr_walk(monkeypatch, name, mon, vid, env):
    ref = _csr_reference(name, mon)
    _setenv(monkeypatch, env)
    dim = hc.mesh(name).dim
    expect = dict(DEFAULTS, MMX_XUP_ORDER=str(int(dim == 3)), MMX_XUP_SWEEP="2" if dim == 2 else "1") if not env else env
    got = _state(name, mon, 2, 10, expect=expect)
    for f in ("x", "xPrev", "xBar", "z", "u", "ih", "bfgs"):
        assert np.array_equal(got[f], ref[f]), f"{f}: differs from the CSR walk, one node per lane"
    assert got["bfgs"][0] > 0 and np.isfinite(got["primal"]).all()


@pytest.mark.parametrize("name,mon", hc.XUP, ids=[n for n, _ in hc.XUP])
def test_xupdate_csr_walk_equals_oracle(name, mon):
    """The form the others are compared with, against the oracle on the same calls."""
    ref = _csr_reference(name, mon)
    oracle_py.set_pow_mode(1)
    O = hc.oracle(name, mon)
    ih = [O.step(10, -1.0)[0] for _ in range(2)]
    for f in ("x", "xPrev", "xBar", "z", "u"):
        assert np.array_equal(ref[f], O.get(f)), f
    assert all(same_energy(a, b) for a, b in zip(ref["ih"], ih)) and ref["bfgs"][0] == O.bfgs_iters()


# ---------------------------------------------------------------- (c) prox forms on ragged sizes
def _prox_variants(dim):
    v = [("tie1", {"MMX_FORCE_TIE": "1"}), ("gradcache0", {"MMX_GRAD_CACHE": "0"})]
    if dim == 2:
        v += [("wave", {"MMX_PROX2D": "wave"})] + [(f"block{b}", {"MMX_PROX_BLOCK": str(b)}) for b in (64, 128, 256)]
    else:
        v += [("quad", {"MMX_PROX3D": "quad"})]
    return v


PROX_RUNS = [(n, m, vid, env) for n, m in hc.PROX for vid, env in _prox_variants(hc.mesh(n).dim)]
_prox_default = {}


@pytest.mark.parametrize("name,mon,vid,env", PROX_RUNS, ids=[f"{n}-{v}" for n, _, v, _ in PROX_RUNS])
def test_prox_forms_equal_default(monkeypatch, name, mon, vid, env):
    if name not in _prox_default:
        _prox_default[name] = _state(name, mon, 2, hc.PROX_ITERS)
    ref = _prox_default[name]
    _setenv(monkeypatch, env)
    got = _state(name, mon, 2, hc.PROX_ITERS, expect=env)
    for f in ("x", "z", "u", "ih", "bfgs"):
        assert np.array_equal(got[f], ref[f]), f"{f}: differs from the default prox"
    assert got["bfgs"][0] > 0


@pytest.mark.parametrize("name,mon", hc.PROX, ids=[n for n, _ in hc.PROX])
def test_prox_default_equals_oracle(name, mon):
    O, G = pair(name, mon)
    assert G.nF == hc.SIZES[name][1]
    for s in range(2):
        ih_o = O.step(hc.PROX_ITERS, -1.0)[0]
        ih_g = G.step(hc.PROX_ITERS, -1.0)[0]
        assert same_energy(ih_g, ih_o)
        for f in ("x", "z", "u"):
            assert np.array_equal(G.get(f), O.get(f)), f"step {s}, {f}"
    assert G.stats()["bfgs_iters"] == O.bfgs_iters()
    G.close()


# ---------------------------------------------------------------- (d) backward Euler
BE_ROWS = hc.BE + hc.BE_HARD
BE_IDS = [f"{n}-mon{m}" + ("-hard" if d else "") for n, m, d, r in BE_ROWS]


@pytest.mark.parametrize("name,mon,dt,rho", BE_ROWS, ids=BE_IDS)
def test_backward_euler_bitwise_against_oracle(name, mon, dt, rho):
    """The Jacobian after the first step -- its widest row has 64 / 65 / 101 / 43 / 87 column nodes,
    the number launch_jac_assemble chooses the kernel by: up to 64 the wavefront assembly, above it
    k_jac_assemble_s -- and three Newton steps, done() before the third."""
    O, G = pair(name, mon, dt, rho)
    dt = dt or hc.DT
    D = hc.mesh(name).dim
    for s in range(3):
        if s == 2:  # done() moves Vp: the next Jacobian is a new one
            O.done()
            G.done()
            np.testing.assert_array_equal(G.get("points"), O.get("points"))
        ih_o, n_o = O.backwards_euler_step(dt, 1e-3, tree=True)
        ih_g, n_g = G.backwards_euler_step(dt, 1e-3)
        assert n_o == n_g, f"Newton iterations differ at step {s}: {n_g}, oracle {n_o}"
        assert same_energy(ih_g, ih_o)
        np.testing.assert_array_equal(G.get("x"), O.get("x"), err_msg=f"x step {s}")
        if s in (0, 2):
            ia_o, ja_o, a_o = O.jacobian()
            ia_g, ja_g, a_g = G.jacobian()
            np.testing.assert_array_equal(ia_g, ia_o)
            np.testing.assert_array_equal(ja_g, ja_o)
            np.testing.assert_array_equal(a_g, a_o)
            assert not np.any((a_g == 0) & np.signbit(a_g)), "a -0.0 in the assembled values"
            assert np.diff(ia_g).max() // D == hc.BE_COLS[name]
    assert G.options()["MMX_JAC_ASSEMBLE"] == "auto"
    G.close()


@pytest.mark.parametrize("name", list(hc.BE_COLS))
def test_jacobian_assembly_forms_agree(name, monkeypatch):
    """The default (the wavefront assembly or, past 64 column nodes, k_jac_assemble_s, after the fast
    FD pass) against the entry-outer assembly after the one-pass exact FD kernel."""
    m = hc.mesh(name)

    def run(expect):
        E = engine(name, 7)
        opts = E.options()
        assert (opts["MMX_JAC_ASSEMBLE"], opts["MMX_FDJ_FAST"]) == expect
        E.backwards_euler_step(hc.DT)
        ia, _, a = E.jacobian()
        jac = a.copy()
        E.backwards_euler_step(hc.DT)
        x = E.get("x").copy()
        E.close()
        return np.diff(ia).max() // m.dim, jac, x

    cols, jac, x = run(("auto", "1"))
    monkeypatch.setenv("MMX_FDJ_FAST", "0")
    monkeypatch.setenv("MMX_JAC_ASSEMBLE", "entry")
    cols0, jac0, x0 = run(("entry", "0"))
    assert cols == cols0 == hc.BE_COLS[name]
    np.testing.assert_array_equal(jac, jac0)
    np.testing.assert_array_equal(x, x0)


SOLVER_FORMS = [{"MMX_SWEEP": "level"}, {"MMX_FACTOR": "level"}, {"MMX_FACTOR": "global"}, {"MMX_FACTOR": "wave"}]
_be_default = {}


def _be_two_steps(name):
    E = engine(name, 7)
    n = [E.backwards_euler_step(hc.DT)[1] for _ in range(2)]
    x = E.get("x").copy()
    E.close()
    return n, x


@pytest.mark.parametrize("env", SOLVER_FORMS, ids=["-".join(f"{k[4:].lower()}-{v}" for k, v in e.items()) for e in SOLVER_FORMS])
@pytest.mark.parametrize("name", hc.BE_SOLVER)
def test_solver_forms_on_hub_rows(name, env, monkeypatch):
    if name not in _be_default:
        _be_default[name] = _be_two_steps(name)
    n0, x0 = _be_default[name]
    _setenv(monkeypatch, env)
    n, x = _be_two_steps(name)
    assert n == n0 and sum(n0) >= 2
    np.testing.assert_array_equal(x, x0)


# ---------------------------------------------------------------- (e) explicit Euler
@pytest.mark.parametrize("name,mon", hc.EULER, ids=[f"{n}-mon{m}" for n, m in hc.EULER])
def test_euler_steps_bitwise_against_oracle(name, mon):
    O, G = pair(name, mon)
    x0 = G.get("x").copy()
    for s in range(3):
        ih_o = O.euler_step()
        ih_g = G.euler_step()
        assert same_energy(ih_g, ih_o)
        np.testing.assert_array_equal(G.get("x"), O.get("x"), err_msg=f"x step {s}")
    assert mon == 1 or not np.array_equal(G.get("x"), x0), "the mesh was expected to move"
    G.close()


# ---------------------------------------------------------------- (g) partitions
def _run_parallel(fns):
    errs = []

    def wrap(f):
        try:
            f()
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=wrap, args=(f,)) for f in fns]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    if errs:
        raise errs[0]


@pytest.mark.parametrize("overlap", ["1", "0"])
@pytest.mark.parametrize("nranks", [2, 4])
@pytest.mark.parametrize("name,mon", hc.PARTITION, ids=[n for n, _ in hc.PARTITION])
def test_partition_equals_single(monkeypatch, name, mon, nranks, overlap):
    """The hub is a local node of every rank with slots of other ranks in its list (where the chunk
    tail's re-read of the last slot can meet a remote one); x equals one rank's."""
    monkeypatch.setenv("MMX_OVERLAP", overlap)
    m = hc.mesh(name)
    dim = m.dim
    last_remote = 0
    for r in range(nranks):
        plan = mx.partition_plan(dim, m.Xp, m.F, nranks, r)
        at = np.nonzero(plan["localNodes"] == 0)[0]
        assert at.size == 1, f"rank {r}: the hub is not a local node"
        src = plan["incSrc"][plan["incPtr"][at[0]]:plan["incPtr"][at[0] + 1]]
        assert src.size == hc.SIZES[name][2] and 0 < (src < 0).sum() < src.size
        last_remote += int(src[-1] < 0)
    assert last_remote >= 1, "on no rank is the hub's last slot a remote one"
    dt, rho = hc.params(name)
    M = mx.Mesh(m.Xp, m.F, m.mask, mx.BuiltinMonitor(dim, mon), rho=rho, tau=hc.TAU, device=0)
    ref = mx.Engine(M, dt)
    comm = mx.Comm.loopback(nranks)
    parts = [mx.Engine(M, dt, rank=r, nranks=nranks, comm=comm, partition="rcb") for r in range(nranks)]
    steps, iters = 5, 6  # the fused predictor from the fourth step on
    for _ in range(steps):
        ref.step(iters, -1.0)

    def run(r):
        def f():
            for _ in range(steps):
                parts[r].step(iters, -1.0)
        return f

    _run_parallel([run(r) for r in range(nranks)])
    xr = ref.get("x").reshape(-1, dim)
    assert not np.array_equal(xr, m.Xp), "the mesh was expected to move"
    covered = np.zeros(m.nP, bool)
    for r, e in enumerate(parts):
        ids = e.local_nodes()
        assert 0 in ids
        assert np.array_equal(e.get("x").reshape(-1, dim), xr[ids]), f"rank {r}: node positions differ from one rank"
        covered[ids] = True
        assert e.stats()["overlap"] == int(overlap)
    assert covered.all()
    for e in parts + [ref]:
        e.close()
    comm.close()


# ---------------------------------------------------------------- (h) the grid rebuilt at every step
@pytest.mark.parametrize("name,mon", hc.REGRID, ids=[n for n, _ in hc.REGRID])
def test_regrid_each_step_bitwise(name, mon):
    oracle_py.set_pow_mode(1)
    O = hc.oracle(name, mon, regrid=True)
    G = engine(name, mon)
    G.set_regrid(True)
    for s in range(4):
        ih_o = O.step(6, -1.0)[0]
        ih_g = G.step(6, -1.0)[0]
        np.testing.assert_array_equal(G.get("grid"), O.get("grid"), err_msg=f"grid step {s}")
        for f in ("x", "z", "u"):
            np.testing.assert_array_equal(G.get(f), O.get(f), err_msg=f"{f} step {s}")
        assert same_energy(ih_g, ih_o)
    assert G.stats()["regrids"] == 4
    G.close()


# ---------------------------------------------------------------- (i) the stationary fan
@pytest.mark.parametrize("name", list(hc.STATIONARY))
def test_failure_parity_at_a_stationary_mesh(name):
    """fan2d(N, 1) under the uniform monitor is stationary for N = 6 and 64: the prox gradient is ~0,
    (p . y)^2 underflows, the BFGS update divides by zero and x turns NaN.  The oracle reports an
    inverted element in step 2 (N = 6) or 1 (N = 64), where the reference would abort on
    assert(Edet > 0).  The engine agrees bit for bit up to that step and raises in it -- observed:
    NonFiniteEnergyError ("non-finite energy in prox without an inverted element") for both N, since
    the determinant of NaN positions is NaN and only a finite Edet <= 0 sets the inverted flag -- and
    it can be closed afterwards."""
    O, G = pair(name, 1)
    fails = hc.STATIONARY[name]
    for s in range(fails):
        ih_o, it_o = O.step(6, hc.TOLS[s])[:2]
        ih_g, it_g = G.step(6, hc.TOLS[s])
        assert it_o == it_g and same_energy(ih_g, ih_o)
        for f in ("x", "z", "u"):
            assert np.array_equal(G.get(f), O.get(f)), f"step {s}, {f}"
    with pytest.raises(RuntimeError, match="inverted element"):
        O.step(6, hc.TOLS[fails])
    with pytest.raises(mx.MMADMMError) as e:
        G.step(6, hc.TOLS[fails])
    print(name, "the engine raised", type(e.value).__name__, "-", e.value)
    assert isinstance(e.value, (mx.InvertedElementError, mx.NonFiniteEnergyError))
    G.close()
    assert G.h is None
