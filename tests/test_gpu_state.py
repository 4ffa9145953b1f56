"""Engine state save and restore on the device: Engine.save_state / load_state / save /
load and state_info.  Everything is compared bit for bit: the eight `get` arrays after a round trip,
and points, Ih and ADMM iteration counts of every step of a run that was saved, destroyed, created
again, loaded and continued, against the uninterrupted run.

Shapes: fan2d(63 / 64 / 65, 1) are one 64-simplex Bkinv block partial, full and spilling; rect2_14 (392
triangles) crosses the 256-simplex chunk; rect3_4 is 384 tets = 6 blocks; hub3d_8_6_2 (320 tets) has a
3D tail block and hub rows; one triangle and one tetrahedron (nF = 1) are saved and loaded only."""
import os
import threading

import numpy as np
import pytest
import torch  # before the library is loaded: libmmadmm then binds to the HIP runtime torch brought

import hub_cases as hc
import mmadmm_amd as mx
from field_monitor_cases import field, make_mesh, static_monitor, step_params
from slide_cases import case as slide_case

pytestmark = pytest.mark.gpu


def _run_parallel(fns):
    """one thread per rank engine of a loopback communicator, as tests/test_gpu_partition.py"""
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

GETS = ("x", "xPrev", "xBar", "z", "u", "points", "hess", "grid")
MESHES = ["fan2d_63_1", "fan2d_64_1", "fan2d_65_1", "rect2_14", "rect3_4", "hub3d_8_6_2"]
ITERS = 6
RHO_FREE = 10.0  # as tests/test_gpu_slide.py: BOUNDARY_FREE meshes invert at the usual rho


def monitor_of(name, dim):
    # the one-ring fans are stationary under the uniform monitor (hub_cases.STATIONARY): the bump at t = 0
    return 7 if name.startswith("fan2d") and name.endswith("_1") else static_monitor(name, dim)


def engine(name, mon=None, grad_use=False, dt=None, env=None, monkeypatch=None, **kw):
    mesh, _ = make_mesh(name)
    d, rho = step_params(name)
    M = mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(mesh.dim, mon or monitor_of(name, mesh.dim)), rho=rho,
                tau=0.5, gradUse=grad_use, device=0)
    if env:  # the environment only around the constructor: an engine reads its switches once, there
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            return mx.Engine(M, dt or d, **kw)
    return mx.Engine(M, dt or d, **kw)


def slide_engine(name, slide):
    c = slide_case(name)
    dt, _ = step_params(name)
    E = mx.Engine(mx.Mesh(c.X0, c.mesh.F, c.mask, mx.BuiltinMonitor(c.dim, 1), rho=RHO_FREE, tau=0.5, device=0), dt)
    if slide:
        E.set_boundary_slide(True)
    return E


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def gets(E):
    return {k: E.get(k) for k in GETS}


def assert_same_gets(A, B, what=""):
    for k in GETS:
        assert same(A[k], B[k]), f"{what}: get('{k}') differs"


def steps(E, tols, iters=ITERS):
    """[(Ih, ADMM iterations, points)] of one step per tolerance"""
    out = []
    for tol in tols:
        ih, it = E.step(iters, tol)
        out.append((ih, it, E.get("points")))
    return out


def assert_same_steps(got, want, what=""):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[1] == w[1], f"{what}: ADMM iterations of step {k}: {g[1]} != {w[1]}"
        assert same(np.array([g[0]]), np.array([w[0]])), f"{what}: Ih of step {k}: {g[0]!r} != {w[0]!r}"
        assert same(g[2], w[2]), f"{what}: points after step {k} differ"


# ---------------------------------------------------------------- 1. round trip
@pytest.mark.parametrize("name", MESHES)
def test_round_trip(name):
    A = engine(name)
    done = 0
    for s in (0, 1, 3):
        steps(A, hc.TOLS[done:s])
        done = s
        blob = A.save_state()
        assert blob.dtype == np.uint8 and blob.size == A.state_bytes()
        want = gets(A)
        B = engine(name)
        B.load_state(blob)
        assert_same_gets(gets(B), want, f"{name} after {s} steps")
        info = mx.state_info(blob)
        assert (info["steps_taken"], info["hess_computed"], info["step_taken"]) == (s, s > 0, s > 0)
        assert (info["dim"], info["nP"], info["nF"], info["nranks"], info["rank"]) == (A.dim, A.nP, A.nF, 1, 0)
        assert info["grid_rows"] == A.gridRows and not info["regrid_each_step"] and not info["slide_frozen"]
        assert info["sections"]["hess"][1] == 8 * A.nF * A.K * A.K
        assert info["payload_bytes"] + mx.STATE_HEADER_BYTES == blob.size
        assert mx.state_checksum(blob[mx.STATE_HEADER_BYTES:]) == info["checksum"]
        # what B saves is the blob it loaded
        assert np.array_equal(B.save_state(), blob)
        B.close()
    A.close()


@pytest.mark.parametrize("name", ["tri", "tet"])
def test_single_simplex_round_trip(name):
    """nF = 1: one lane of one block; saved, loaded and read only"""
    A, B = slide_engine(name, False), slide_engine(name, False)
    blob = A.save_state(device=True)
    assert blob.is_cuda and blob.dtype == torch.uint8 and blob.numel() == A.state_bytes()
    B.load_state(blob)
    assert_same_gets(gets(B), gets(A), name)
    assert np.array_equal(A.save_state(), blob.cpu().numpy())
    assert mx.state_info(blob)["nF"] == 1
    A.close()
    B.close()


# ---------------------------------------------------------------- 2. continuation
@pytest.mark.parametrize("name,grad_use", [(n, False) for n in MESHES] + [("fan2d_64_1", True)])
def test_continuation(name, grad_use):
    """five steps under hub_cases.TOLS (one early-exit step among the fixed-count ones); saved after s
    steps, s = 0 (no Hessian yet) .. 3 (the predictor has switched to xPrev), the engine destroyed, a
    new one loaded and run to the end"""
    A = engine(name, grad_use=grad_use)
    want = steps(A, hc.TOLS)
    A.close()
    B = engine(name, grad_use=grad_use)
    blobs, got = [], []
    for s in range(4):
        blobs.append(B.save_state())
        got += steps(B, hc.TOLS[s:s + 1])
    B.close()
    assert_same_steps(got, want[:4], f"{name}: the saving run")
    for s, blob in enumerate(blobs):
        C = engine(name, grad_use=grad_use)
        C.load_state(blob)
        assert_same_steps(steps(C, hc.TOLS[s:]), want[s:], f"{name}: continued after {s} steps")
        C.close()


# ---------------------------------------------------------------- 3. three routes, one blob
@pytest.mark.parametrize("name", ["rect2_14", "rect3_4"])
def test_three_routes_one_blob(name, tmp_path):
    A = engine(name)
    steps(A, hc.TOLS[:2])
    path = os.path.join(tmp_path, "state.mmx")
    host = A.save_state()
    dev = A.save_state(device=True)
    A.save(path)
    with open(path, "rb") as f:
        filed = f.read()
    assert np.array_equal(host, dev.cpu().numpy()), "the device blob differs from the host blob"
    assert host.tobytes() == filed, "the file differs from the host blob"
    assert mx.state_info(path) == mx.state_info(host[:mx.STATE_HEADER_BYTES]) == mx.state_info(dev)
    # `out` given: the blob in the caller's buffers
    out = torch.empty(host.size + 64, dtype=torch.uint8, device=dev.device)
    assert np.array_equal(A.save_state(out=out).cpu().numpy(), host)
    assert np.array_equal(A.save_state(out=np.zeros(host.size, dtype=np.uint8)), host)
    want = steps(A, hc.TOLS[2:4])
    A.close()
    for how, arg in (("host", host), ("bytes", filed), ("device", dev), ("file", path)):
        B = engine(name)
        if how == "file":
            B.load(arg)
        else:
            B.load_state(arg)
        assert_same_steps(steps(B, hc.TOLS[2:4]), want, f"{name}: loaded from {how}")
        B.close()


# ---------------------------------------------------------------- 4. rollback
@pytest.mark.parametrize("name", ["rect2_14", "hub3d_8_6_2"])
def test_rollback_after_failed_step(name):
    """a device snapshot, a step that fails on a NaN monitor (an error return: nothing faults), the
    snapshot loaded into the same engine: the following steps are those of the undisturbed run"""
    R = engine(name)
    want = steps(R, hc.TOLS[:4])
    R.close()
    A = engine(name)
    steps(A, hc.TOLS[:2])
    snap = A.save_state(device=True)
    A.regrid_values(torch.full((A.nP, A.dim, A.dim), float("nan"), dtype=torch.float64, device=snap.device))
    with pytest.raises(mx.NonFiniteEnergyError):
        A.step(ITERS, hc.TOLS[2])
    A.load_state(snap)
    assert_same_steps(steps(A, hc.TOLS[2:4]), want[2:4], f"{name}: after the rollback")
    A.close()


# ---------------------------------------------------------------- 5. time-varying monitor
@pytest.mark.parametrize("name,mon", hc.REGRID)
def test_time_varying_monitor_continues(name, mon):
    """set_regrid(True) with the moving bump: t = steps taken * dt and the flag come back with the blob"""
    A = engine(name, mon=mon)
    A.set_regrid(True)
    steps(A, [-1.0] * 2)
    blob = A.save_state()
    want = steps(A, [-1.0] * 2)
    A.close()
    info = mx.state_info(blob)
    assert info["regrid_each_step"] and info["steps_taken"] == 2
    B = engine(name, mon=mon)  # (set_regrid is not called: the blob carries it)
    B.load_state(blob)
    assert_same_steps(steps(B, [-1.0] * 2), want, name)
    assert B.stats()["regrids"] == 2
    B.close()


# ---------------------------------------------------------------- 6. field grid
def test_field_grid_travels_with_the_blob():
    name = "rect2_8"
    A = engine(name)
    steps(A, [-1.0])  # the rebuilt grid's box is then that of the moved points, not of the mesh
    u = field(A.get("points").reshape(-1, 2))
    A.regrid_field(u, 1.0)
    assert A.quality("last")[1]["invalid"] == 0
    blob = A.save_state()
    grid = A.get("grid")
    want = steps(A, [-1.0] * 2)
    A.close()
    B = engine(name)  # never saw u
    assert not same(B.get("grid"), grid)
    B.load_state(blob)
    assert same(B.get("grid"), grid)
    with pytest.raises(mx.MMADMMError, match="MMADMM_QUALITY_LAST before any rebuild"):
        B.quality("last")
    assert_same_steps(steps(B, [-1.0] * 2), want, name)
    B.regrid_field(field(B.get("points").reshape(-1, 2)), 1.0)
    assert B.quality("last")[1]["invalid"] == 0
    B.close()


# ---------------------------------------------------------------- 7. sliding
@pytest.mark.parametrize("name", ["rect2_8", "hexdisc6", "rect3_3"])  # the meshes tests/test_gpu_slide.py steps
def test_sliding_surface_travels_with_the_blob(name):
    A = slide_engine(name, False)
    A.step(5, -1.0)  # the surface is frozen after a step: X0 is not the mesh's points
    A.set_boundary_slide(True)
    steps(A, [-1.0] * 2, 5)
    blob = A.save_state()
    fa = A.boundary()
    want = steps(A, [-1.0] * 2, 5)
    A.close()
    info = mx.state_info(blob)
    assert info["slide_on"] and info["slide_frozen"] and info["n_sliding"] == len(fa[1]) > 0
    B = slide_engine(name, False)  # sliding never enabled here
    B.load_state(blob)
    fb = B.boundary()
    for a, b in zip(fa, fb):
        assert np.array_equal(a, b)
    assert_same_steps(steps(B, [-1.0] * 2, 5), want, name)
    assert sum(B.slide_counts()[k] for k in ("star", "hopped")) > 0  # (the projection did run)
    # a blob saved without a surface turns it off again, on the same engine
    C = slide_engine(name, False)
    B.load_state(C.save_state())
    with pytest.raises(mx.MMADMMError, match="no frozen boundary"):
        B.boundary()
    B.close()
    C.close()


# ---------------------------------------------------------------- 8. partition
@pytest.mark.parametrize("name,mon", hc.PARTITION)
def test_partition_each_rank_its_own_blob(name, mon):
    nranks = 2
    ref = engine(name, mon=mon)
    want = steps(ref, [-1.0] * 5)
    comm = mx.Comm.loopback(nranks)

    def run(parts, n, out):
        def f(r):
            return lambda: out.__setitem__(r, steps(parts[r], [-1.0] * n))
        _run_parallel([f(r) for r in range(nranks)])

    parts = [engine(name, mon=mon, rank=r, nranks=nranks, comm=comm) for r in range(nranks)]
    run(parts, 2, [None] * nranks)
    blobs = [e.save_state() for e in parts]
    for e in parts:
        e.close()
    for r, b in enumerate(blobs):
        info = mx.state_info(b)
        assert (info["rank"], info["nranks"], info["steps_taken"]) == (r, nranks, 2)
    parts = [engine(name, mon=mon, rank=r, nranks=nranks, comm=comm) for r in range(nranks)]
    with pytest.raises(mx.MMADMMError, match="rank"):
        parts[1].load_state(blobs[0])
    with pytest.raises(mx.MMADMMError, match="nranks"):
        ref.load_state(blobs[0])
    for e, b in zip(parts, blobs):
        e.load_state(b)
    got = [None] * nranks
    run(parts, 3, got)
    for r, e in enumerate(parts):
        ids = e.local_nodes()
        for k in range(3):
            assert got[r][k][1] == want[2 + k][1]
            xr = want[2 + k][2].reshape(-1, e.dim)[ids]
            assert same(got[r][k][2].reshape(-1, e.dim), xr), f"{name}: rank {r}, step {2 + k}"
        e.close()
    # the refusals left the one-rank engine as it was: its sixth step equals a fresh run's
    ref2 = engine(name, mon=mon)
    steps(ref2, [-1.0] * 5)
    assert_same_steps(steps(ref, [-1.0]), steps(ref2, [-1.0]), name)
    ref.close()
    ref2.close()
    comm.close()


# ---------------------------------------------------------------- 9. other switches
# DESIGN.md §11, each documented bit-identical: another prox kernel (2D: k_prox_wave<2> with Bkinv
# double-buffered; 3D: k_prox_quad), another x-update (the CSR walk from z and u, no slot terms)
SWITCHES = [("rect2_14", {"MMX_PROX2D": "wave"}), ("rect2_14", {"MMX_XUP_REC": "0", "MMX_TSLOT": "0", "MMX_ZX": "0"}),
            ("fan2d_65_1", {"MMX_PROX2D": "wave", "MMX_ISO": "0"}), ("rect3_4", {"MMX_PROX3D": "quad"}),
            ("hub3d_8_6_2", {"MMX_TSLOT": "0", "MMX_XUP_REC": "0"})]


@pytest.mark.parametrize("name,env", SWITCHES, ids=[f"{n}-{'-'.join(e)}" for n, e in SWITCHES])
def test_blob_loads_under_other_switches(name, env, monkeypatch):
    A = engine(name)
    steps(A, hc.TOLS[:2])
    blob = A.save_state()
    want = steps(A, hc.TOLS[2:5])
    A.close()
    # Ih is a sum over workgroup partials, which another prox kernel groups differently (the project
    # compares it to 1e-12 across prox kernels, tests/test_gpu_parity.py): its bits are checked against
    # the uninterrupted run under the same switches, the state's bits against the default run too
    U = engine(name, env=env, monkeypatch=monkeypatch)
    want_u = steps(U, hc.TOLS)[2:5]
    U.close()
    for (_, it_u, x_u), (_, it_w, x_w) in zip(want_u, want):
        assert it_u == it_w and same(x_u, x_w)
    B = engine(name, env=env, monkeypatch=monkeypatch)
    opts = B.options()
    assert all(opts[k] == v for k, v in env.items()), opts
    B.load_state(blob)
    assert_same_steps(steps(B, hc.TOLS[2:5]), want_u, f"{name} under {env}")
    # and back: what the other engine saves loads into a default one
    blob2 = B.save_state()
    want2 = steps(B, [-1.0])
    B.close()
    C = engine(name)
    C.load_state(blob2)
    (ih, it, x), (ih2, it2, x2) = steps(C, [-1.0])[0], want2[0]
    assert it == it2 and same(x, x2) and abs(ih - ih2) <= 1e-12 * abs(ih2), f"{name} from {env}"
    C.close()


# ---------------------------------------------------------------- 10. refusals
def test_refusals_leave_the_engine_untouched(tmp_path):
    name = "rect2_8"
    T, R = engine(name), engine(name)  # T sees every refused call, R none
    for e in (T, R):
        e.step(5, -1.0)
    good = T.save_state()
    H = mx.STATE_HEADER_BYTES
    other_mesh = engine("rect2_5")
    other_dt = engine(name, dt=0.0125)
    other_dt.step(5, -1.0)

    def edited(at, value):
        b = good.copy()
        b[at] = value
        return b

    version = int(np.frombuffer(good[8:12].tobytes(), dtype="<u4")[0])
    newer = good.copy()
    newer[8:12] = np.frombuffer(np.uint32(version + 1).astype("<u4").tobytes(), dtype=np.uint8)
    bad = [("another mesh", other_mesh.save_state(), "nP ="),
           ("another dt", other_dt.save_state(), "fingerprint"),
           ("truncated", good[:-8], "too short"),
           ("too long", np.concatenate([good, np.zeros(8, np.uint8)]), "too long"),
           ("payload byte", edited(H + good.size // 2, good[H + good.size // 2] ^ 1), "checksum"),
           ("magic", edited(0, ord("X")), "magic"),
           ("version", newer, "version")]
    path = os.path.join(tmp_path, "bad.mmx")
    for what, blob, msg in bad:
        for route in ("host", "device", "file"):
            with pytest.raises(mx.MMADMMError, match=msg) as e:
                if route == "host":
                    T.load_state(blob)
                elif route == "device":
                    T.load_state(torch.from_numpy(blob.copy()).cuda())
                else:
                    with open(path, "wb") as f:
                        f.write(blob.tobytes())
                    T.load(path)
            assert e.value.code == 1, (what, route)  # MMADMM_ERR_INVALID
        assert_same_steps(steps(T, [-1.0], 5), steps(R, [-1.0], 5), f"after the refusal of {what}")
        assert_same_gets(gets(T), gets(R), what)
    # cap one byte short, on both save routes; a missing file; NULL arguments
    n = T.state_bytes()
    with pytest.raises(mx.MMADMMError, match="cap"):
        T.save_state(out=np.zeros(n - 1, dtype=np.uint8))
    with pytest.raises(mx.MMADMMError, match="cap"):
        T.save_state(out=torch.zeros(n - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(mx.MMADMMError) as e:
        T.load(os.path.join(tmp_path, "missing.mmx"))
    assert e.value.code == 4  # MMADMM_ERR_IO
    L = mx.lib()
    for rc in (L.mmadmm_state_bytes(T.h, None), L.mmadmm_state_save(T.h, None, n), L.mmadmm_state_load(T.h, None, n),
               L.mmadmm_state_save_device(T.h, None, n, None), L.mmadmm_state_load_device(T.h, None, n, None),
               L.mmadmm_state_write_file(T.h, None), L.mmadmm_state_read_file(T.h, None)):
        assert rc == 1
    assert_same_steps(steps(T, [-1.0], 5), steps(R, [-1.0], 5), "after the refused saves")
    for e in (T, R, other_mesh, other_dt):
        e.close()
