"""The x-update on node records in sweep order (mm-admm_amd/csrc/host/xup_records.h, DeviceMesh::xrec):
the record, invdiag and the first chunk of slot offsets come by position of the node order, so a
lane reaches its z/u gathers in two dependent load phases; MMX_XUP_REC=0 keeps the CSR walk.  The
sums keep their order, so everything here is bit for bit:

* against the oracle (x, z, u) over five steps whose tolerances (-1, 1e-3, -1, -1, -1) run the
  every-iteration residual (step 2) and the fused-predictor first x-update (steps after the third),
  on a hexagonal disc (valence <= 6), 2D square grids (valence 8: the tail past the chunk of 6), a
  3D grid (valence 24), a Shoulder mesh (nodes no simplex references) and two hub meshes (valence
  64 and 80);
* MMX_XUP_REC=0 against the default for the one-node-per-lane form and the sweep (MMX_XUP_SWEEP = 0,
  1, 2), with and without the next node's early request, for both MMX_TSLOT values;
* a 2-rank loopback partition (interior / interface launches by position, remote slots) against
  one rank, overlap on and off;
* the last prox of a step without its gradient-cache store (MMX_GC_SKIP) against with it."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(__file__)), "mm-admm_amd", "python"))

import hub_meshes  # noqa: E402
import mmadmm_amd as mx  # noqa: E402
import oracle_py  # noqa: E402

pytestmark = pytest.mark.gpu

TOLS = (-1.0, 1e-3, -1.0, -1.0, -1.0)


@pytest.fixture(autouse=True)
def _pow_mode_reset():
    yield
    oracle_py.set_pow_mode(0)


ORACLE_CASES = [
    ("hexdisc12", lambda: mx.MeshData.hexdisc(12, 0.5, 0.5, 0.5), 1, 50.0, 0.055),
    ("rect2d_6", lambda: mx.MeshData.rect(2, 6), 3, 1000.0, 0.025),
    ("rect3d_4", lambda: mx.MeshData.rect(3, 4), 6, 2000.0, 0.025),
    ("shoulder2d_8", lambda: mx.MeshData.shoulder(2, 8), 1, 50.0, 0.025),
    # one node of 64 / 80 slots (tests/hub_meshes.py; the other hub rows: tests/test_gpu_hub_meshes.py)
    ("fan2d_64_2", lambda: hub_meshes.fan2d(64, 2), 7, 1000.0, 0.0025),
    ("hub3d_8_6_2", lambda: hub_meshes.hub3d(8, 6, 2), 7, 2000.0, 0.0025),
]


@pytest.mark.parametrize("name,gen,mon,rho,dt", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_records_bitwise_against_oracle(name, gen, mon, rho, dt):
    m = gen()
    if name.startswith("shoulder"):  # the mesh must hold a node no simplex references
        assert np.setdiff1d(np.arange(m.nP), np.unique(m.F)).size > 0
    oracle_py.set_pow_mode(1)
    om = oracle_py.Mesh(m.dim, m.Xp, m.F, m.mask)
    O = oracle_py.Integrator(om, mon, dt, 0.5, rho, cgMode=1)
    G = mx.Engine(mx.Mesh(m.Xp, m.F, m.mask, mx.BuiltinMonitor(m.dim, mon), rho=rho, tau=0.5), dt)
    for s, tol in enumerate(TOLS):
        it_o = O.step(6, tol)[1]
        it_g = G.step(6, tol)[1]
        assert it_o == it_g, f"step {s}: ADMM iterations {it_g}, oracle {it_o}"
        for f in ("x", "z", "u"):
            a, b = G.get(f), O.get(f)
            assert np.array_equal(a, b), f"step {s}, {f}: {np.count_nonzero(a != b)} of {a.size} entries differ"
    G.close()


def _state(mesh, mon, rho, dt, steps, iters):
    G = mx.Engine(mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(mesh.dim, mon), rho=rho, tau=0.5), dt)
    ih = [G.step(iters, -1.0)[0] for _ in range(steps)]
    out = {f: G.get(f) for f in ("x", "xPrev", "xBar", "z", "u")}
    st = G.stats()
    out["ih"] = np.array(ih)
    out["primal"] = np.array([st["last_primal"], st["last_dual"]])
    out["bfgs"] = np.array([st["bfgs_iters"]])
    G.close()
    return out


AB_MESHES = {
    "hexdisc60": (lambda: mx.MeshData.hexdisc(60, 0.5, 0.5, 0.5), 1, 50.0, 0.055),
    "rect3d_12": (lambda: mx.MeshData.rect(3, 12), 6, 2000.0, 0.025),
}
_csr_state = {}


def _csr_reference(monkeypatch, mesh_id, tslot):
    """MMX_XUP_REC=0, one node per lane: computed once per mesh and slot-term setting."""
    key = (mesh_id, tslot)
    if key not in _csr_state:
        gen, mon, rho, dt = AB_MESHES[mesh_id]
        monkeypatch.setenv("MMX_XUP_REC", "0")
        monkeypatch.setenv("MMX_XUP_SWEEP", "0")
        monkeypatch.setenv("MMX_TSLOT", tslot)
        _csr_state[key] = _state(gen(), mon, rho, dt, 2, 10)
    return _csr_state[key]


# (workgroups per CU of the sweep, the next node's early request): 0 = one node per lane
FORMS = [("0", "0"), ("1", "0"), ("1", "1"), ("2", "0"), ("2", "1")]


@pytest.mark.parametrize("sweep,early", FORMS, ids=[f"sweep{s}_early{e}" for s, e in FORMS])
@pytest.mark.parametrize("tslot", ["0", "1"])
@pytest.mark.parametrize("mesh_id", list(AB_MESHES))
def test_records_equal_csr_path(monkeypatch, mesh_id, tslot, sweep, early):
    ref = _csr_reference(monkeypatch, mesh_id, tslot)
    gen, mon, rho, dt = AB_MESHES[mesh_id]
    monkeypatch.setenv("MMX_TSLOT", tslot)
    monkeypatch.setenv("MMX_XUP_SWEEP", sweep)
    monkeypatch.setenv("MMX_XUP_EARLY", early)
    got = {}
    for rec in ("0", "1"):
        monkeypatch.setenv("MMX_XUP_REC", rec)
        got[rec] = _state(gen(), mon, rho, dt, 2, 10)
    for f in ("x", "xPrev", "xBar", "z", "u", "ih", "bfgs"):
        assert np.array_equal(got["1"][f], got["0"][f]), f"{f}: the records differ from the CSR walk in the same form"
        assert np.array_equal(got["1"][f], ref[f]), f"{f}: differs from the CSR walk, one node per lane"
    # the residual's grouping belongs to the form (sweep: per workgroup of the fixed grid), not to the layout
    assert np.array_equal(got["1"]["primal"], got["0"]["primal"])


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
@pytest.mark.parametrize("dim,n,mon,rho,dt", [(2, 16, 3, 1000.0, 0.025), (3, 6, 6, 2000.0, 0.025)])
def test_records_partition_equals_single(monkeypatch, dim, n, mon, rho, dt, overlap):
    monkeypatch.setenv("MMX_OVERLAP", overlap)
    mesh = mx.MeshData.rect(dim, n)
    M = mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(dim, mon), rho=rho, tau=0.5, device=0)
    ref = mx.Engine(M, dt)
    nranks = 2
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
    covered = np.zeros(mesh.nP, bool)
    for r, e in enumerate(parts):
        ids = e.local_nodes()
        assert np.array_equal(e.get("x").reshape(-1, dim), xr[ids]), f"rank {r}: node positions differ from one rank"
        covered[ids] = True
        st = e.stats()
        assert st["overlap"] == int(overlap)
        if overlap == "1":
            assert 0 < st["interior_nodes"] < e.nP
    assert covered.all()
    for e in parts + [ref]:
        e.close()
    comm.close()


def test_last_prox_without_cache_store(monkeypatch):
    """A step resets z, so the gradient cache its last prox would leave is never read: with the store
    skipped (the default) and written (MMX_GC_SKIP=0) three steps give the same BFGS totals, x, z, u
    and reported energies."""
    mesh = mx.MeshData.hexdisc(40, 0.5, 0.5, 0.5)
    got = {}
    for skip in ("1", "0"):
        monkeypatch.setenv("MMX_GC_SKIP", skip)
        got[skip] = _state(mesh, 1, 50.0, 0.055, 3, 10)
    for f in ("bfgs", "x", "z", "u", "ih", "primal"):
        assert np.array_equal(got["1"][f], got["0"][f]), f
    assert got["1"]["bfgs"][0] > 0


def test_xupdate_bytes_count_the_records(monkeypatch):
    """stats()["xupdate_bytes"] on the records: record, invdiag and the chunk of the slot table by
    position, the CSR only for the slots past a node's first chunk."""
    mesh = mx.MeshData.rect(2, 12)  # valence 8 at the nodes where four diagonals meet
    val = np.bincount(mesh.F.reshape(-1), minlength=mesh.nP)
    assert val.max() == 8
    monkeypatch.setenv("MMX_TSLOT", "0")
    G = mx.Engine(mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(2, 3), rho=1000.0, tau=0.5), 0.025)
    nP, nF, K, D, CH = mesh.nP, mesh.nF, 6, 2, 6
    want = nP * (12 + 8 + 4 * CH) + 4 * int(np.maximum(val - CH, 0).sum()) + 16 * K * nF + 8 * D * nP * 2
    assert G.stats()["xupdate_bytes"] == want
    G.close()
