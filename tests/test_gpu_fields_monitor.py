"""The monitor from several components on the device (mmadmm_field_hessians(_device),
mmadmm_regrid_fields(_huang)(_device); Engine.field_hessians, Engine.regrid_fields): the Hessians and the
metric against the host function (mmadmm_fields_monitor) bit for bit on a moved mesh; the rebuild
against the values path fed with the host function's monitor, plain and normalised, alpha given and
solved, over three rounds; the producer-stream ordering; quality("last"); the adaptive loop on tensors
against the same loop through the host calls; the refusals."""
import ctypes

import numpy as np
import pytest
import torch  # before the library is loaded: libmmadmm then binds to the HIP runtime torch brought

import mmadmm_amd as mx
from fields_cases import COUNTS, HUB_MESHES, fields, make_mesh, static_monitor, step_params, weights

pytestmark = pytest.mark.gpu

MESHES = ["rect2_8", "rect3_4", "hexdisc6", "shoulder2_8", "rect2_20", "fan2d_7_2", "fan2d_13_2", "hub3d_8_6_2"]
CASES = [(n, i) for n in MESHES for i in range(4)]  # i: index into COUNTS[dim]
ITERS = 5
HUB_FIELD_DT = 0.1  # as tests/test_gpu_field_monitor.py: the hub meshes' slivers under a field monitor
FINE_DT = 4.0       # as tests/test_gpu_field_huang.py: rect(2, 256) under a field monitor
BATCH = 64


def engine(mesh, mon, name="", dt_scale=1.0):
    dt, rho = step_params(name)
    M = mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(mesh.dim, mon), rho=rho, tau=0.5, device=0)
    return mx.Engine(M, dt * dt_scale)


def field_scale(name):
    return HUB_FIELD_DT if name in HUB_MESHES else FINE_DT if name == "rect2_256" else 1.0


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def same_state(A, B, what=("grid", "x", "z", "u")):
    for w in what:
        assert np.array_equal(A.get(w), B.get(w)), f"'{w}' differs"
    assert A.stats()["monitor_iso"] == B.stats()["monitor_iso"]


@pytest.mark.parametrize("name,i", CASES)
def test_field_hessians_equal_host_function(name, i):
    mesh, _ = make_mesh(name)
    D, C = mesh.dim, COUNTS[mesh.dim][i]
    E = engine(mesh, static_monitor(name, D), name)
    E.step(ITERS, -1.0)
    E.step(ITERS, -1.0)
    X = E.get("points").reshape(-1, D)
    assert not np.array_equal(X, mesh.Xp), "the mesh was expected to move"
    U, w = fields(X, C), weights(C)
    Hh, Ah, _, _ = mx.fields_monitor(X, E.simplices(), U, w, 1.0)
    Ht, At = E.field_hessians(cuda(U), w)
    assert Ht.is_cuda and tuple(Ht.shape) == (mesh.nP, C, D, D) and tuple(At.shape) == (mesh.nP, D, D)
    Ha, Aa = E.field_hessians(U, w)
    for got, want, what in ((Ht.cpu().numpy(), Hh, "H tensor"), (At.cpu().numpy(), Ah, "A tensor"),
                            (Ha, Hh, "H array"), (Aa, Ah, "A array")):
        assert np.array_equal(got, want), f"{what}: differs at {int((got != want).sum())} entries"
    # each component is the scalar call of that column, whatever the batching
    for c in {0, C - 1}:
        assert np.array_equal(Ha[:, c], E.field_hessian(U[:, c].copy()))
    if C == 1:  # a 1-D U is one component; weights None are all 1
        H1, A1 = E.field_hessians(cuda(U[:, 0].copy()))
        assert np.array_equal(H1.cpu().numpy(), Hh) and tuple(H1.shape) == (mesh.nP, 1, D, D)
    # either output alone through the C call
    L, one = mx.lib(), np.zeros_like(Ah)
    assert L.mmadmm_field_hessians(E.h, C, mx._dp(U), mx._dp(w), None, mx._dp(one)) == 0 and np.array_equal(one, Ah)
    one = np.zeros_like(Hh)
    assert L.mmadmm_field_hessians(E.h, C, mx._dp(U), mx._dp(w), mx._dp(one), None) == 0 and np.array_equal(one, Hh)


@pytest.mark.parametrize("normalise", [False, True], ids=["plain", "huang"])
@pytest.mark.parametrize("name,i", [(n, k % 4) for k, n in enumerate(MESHES)] + [("rect2_8", 1), ("rect3_4", 3)])
def test_regrid_fields_equals_values_path(name, i, normalise):
    mesh, _ = make_mesh(name)
    D, C = mesh.dim, COUNTS[mesh.dim][i]
    mon = static_monitor(name, D)
    A, B = engine(mesh, mon, name, field_scale(name)), engine(mesh, mon, name, field_scale(name))
    F, w = A.simplices(), weights(C)
    alpha = None
    for k in range(3):
        X = A.get("points").reshape(-1, D)
        assert np.array_equal(X, B.get("points").reshape(-1, D))
        U = fields(X, C)
        # normalised: rounds 0 and 2 solve, round 1 is given the last alpha; plain: the host function's
        # default in rounds 0 and 2 (the mean Frobenius norm of A), the last alpha in round 1
        given = alpha if k == 1 else None
        _, _, Mh, ah = mx.fields_monitor(X, F, U, w, given, normalise)
        if normalise:
            alpha = A.regrid_fields(cuda(U), w, given, normalise=True)
            passes, syncs = A.field_solve_info()
            if given is None:
                print(name, "C", C, "round", k, "alpha", alpha, "passes", passes, "read-backs", syncs)
                assert passes >= 52 and syncs == -(-passes // BATCH)
            else:
                assert (passes, syncs) == (0, 0)
        else:
            alpha = A.regrid_fields(cuda(U), w, ah)
        assert alpha == ah, (k, alpha, ah)
        B.regrid_values(cuda(Mh))
        same_state(A, B, what=("grid",))
        if k < 2:
            A.step(ITERS, -1.0)
            B.step(ITERS, -1.0)
            same_state(A, B)
    assert A.stats()["regrids"] == B.stats()["regrids"] == 3
    assert not np.array_equal(A.get("points").reshape(-1, D), mesh.Xp), "the mesh was expected to move"


def test_two_components_259_partials():
    mesh, _ = make_mesh("rect2_256")
    A, B = engine(mesh, 1, "rect2_256", FINE_DT), engine(mesh, 1, "rect2_256", FINE_DT)
    X = A.get("points").reshape(-1, 2)
    U, w = fields(X, 2), weights(2)
    a = A.regrid_fields(cuda(U), w, normalise=True)
    _, _, Mh, ah = mx.fields_monitor(X, A.simplices(), U, w, None, normalise=True)
    assert a == ah
    B.regrid_values(cuda(Mh))
    same_state(A, B, what=("grid",))


@pytest.mark.parametrize("normalise", [False, True], ids=["plain", "huang"])
def test_host_array_equals_tensor(normalise):
    mesh, _ = make_mesh("rect3_4")
    A, B, C3 = engine(mesh, 3), engine(mesh, 3), engine(mesh, 3)
    U, w = fields(A.get("points").reshape(-1, 3), 4), weights(4)
    a = A.regrid_fields(cuda(U), w, None if normalise else 2.5, normalise=normalise)
    assert B.regrid_fields(U, w, None if normalise else 2.5, normalise=normalise) == a
    same_state(A, B, what=("grid",))
    if not normalise:  # the wrapper's default alpha, arrays: numpy on both sides
        a = B.regrid_fields(U, w)
        assert a == mx.fields_monitor(mesh.Xp, B.simplices(), U, w)[3]
        assert A.regrid_fields(cuda(U), w) == pytest.approx(a, rel=1e-12)
    # one component, no weights: the scalar call, bit for bit in the plain form
    u = np.ascontiguousarray(U[:, 0])
    A.regrid_fields(cuda(u), None, 2.5, normalise=normalise)
    C3.regrid_field(cuda(u), 2.5, normalise=normalise)
    if not normalise:
        same_state(A, C3, what=("grid",))
    else:
        ga, gc = A.get("grid"), C3.get("grid")
        assert np.abs(ga - gc).max() <= 1e-12 * np.abs(gc).max()


def test_producer_stream_is_waited_for():
    mesh, _ = make_mesh("rect2_14")
    A, B = engine(mesh, 1), engine(mesh, 1)
    Uh = fields(A.get("points").reshape(-1, 2), 3) * 1.5
    w = weights(3)
    a = A.regrid_fields(cuda(Uh), w, normalise=True)  # the tensor is complete: .to() has finished
    Ha, Aa = A.field_hessians(cuda(Uh), w)
    torch.cuda.synchronize()
    base = cuda(Uh)
    big = torch.ones((2048, 2048), device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        for _ in range(20):  # work queued ahead of the producer on its stream
            big = (big @ big) * (1.0 / 2048)
        U = base * 1.0  # produced on s immediately before the calls; nobody synchronises
        Hb, Ab = B.field_hessians(U, w)
        b = B.regrid_fields(U, w, normalise=True)
    assert a == b
    same_state(A, B, what=("grid",))
    torch.cuda.synchronize()
    assert torch.equal(Ha, Hb) and torch.equal(Aa, Ab)


def test_c_call_with_null_stream():
    mesh, _ = make_mesh("rect2_8")
    A, B = engine(mesh, 1), engine(mesh, 1)
    U, w = fields(mesh.Xp, 3), weights(3)
    d_U = cuda(U)
    torch.cuda.synchronize()  # NULL stream: the data are ready
    L, used = mx.lib(), ctypes.c_double(0.0)
    assert L.mmadmm_regrid_fields_huang_device(A.h, 3, d_U.data_ptr(), mx._dp(w), 0.0, None, ctypes.byref(used)) == 0
    assert B.regrid_fields(U, w, normalise=True) == used.value
    same_state(A, B, what=("grid",))
    assert L.mmadmm_regrid_fields_device(A.h, 3, d_U.data_ptr(), None, 2.5, None) == 0
    B.regrid_fields(U, None, 2.5)
    same_state(A, B, what=("grid",))
    H = torch.zeros((mesh.nP, 3, 2, 2), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    assert L.mmadmm_field_hessians_device(A.h, 3, d_U.data_ptr(), None, H.data_ptr(), None, None) == 0  # waits
    assert np.array_equal(H.cpu().numpy(), mx.fields_monitor(mesh.Xp, A.simplices(), U, None, 1.0)[0])
    assert L.mmadmm_regrid_fields_huang(A.h, 3, mx._dp(U), None, 0.0, None) == 0  # alpha_used may be NULL


@pytest.mark.parametrize("name,normalise", [("rect2_14", True), ("rect3_4", False)])
def test_quality_last(name, normalise):
    mesh, _ = make_mesh(name)
    D = mesh.dim
    E = engine(mesh, static_monitor(name, D))
    C = COUNTS[D][2]
    U, w = fields(mesh.Xp, C), weights(C)
    a = E.regrid_fields(cuda(U), w, None if normalise else 2.5, normalise=normalise)
    _, _, Mh, _ = mx.fields_monitor(mesh.Xp, E.simplices(), U, w, a, normalise)
    q1, s1 = E.quality("last")
    q2, s2 = E.quality(Mh)
    assert np.array_equal(q1, q2) and s1 == s2


def test_adaptive_loop_tensors_equal_host_calls():
    mesh, _ = make_mesh("rect2_14")
    A, B = engine(mesh, 1), engine(mesh, 1)
    w = weights(2)
    Ua = fields(mesh.Xp, 2)
    Ub = cuda(Ua)
    for k in range(3):
        aa = A.regrid_fields(Ua, w, normalise=True)
        ab = B.regrid_fields(Ub, w, normalise=True)
        assert aa == ab
        same_state(A, B, what=("grid",))
        qa, sa = A.quality("last")
        qb, sb = B.quality("last")
        assert sa == sb and np.array_equal(qa, qb)
        Xa, Xb = A.get("points").reshape(-1, 2), B.get_tensor("points")
        A.step(ITERS, -1.0)
        B.step(ITERS, -1.0)
        same_state(A, B)
        Ua, ia = A.transfer(Ua, Xa)
        Ub, ib = B.transfer(Ub, Xb)
        assert {k2: ia[k2] for k2 in mx.TRANSFER_COUNTS} == {k2: ib[k2] for k2 in mx.TRANSFER_COUNTS}
        assert np.array_equal(Ua, Ub.cpu().numpy()), f"round {k}: U differs"
    assert not np.array_equal(A.get("points").reshape(-1, 2), mesh.Xp), "the mesh was expected to move"


def test_field_solve_info():
    mesh, _ = make_mesh("rect2_8")
    E = engine(mesh, 1)
    U, w = fields(mesh.Xp, 2), weights(2)
    a = E.regrid_fields(cuda(U), w, normalise=True)
    passes, syncs = E.field_solve_info()
    assert passes >= 52 and syncs == -(-passes // BATCH)
    assert E.regrid_fields(cuda(U), w, a, normalise=True) == a and E.field_solve_info() == (0, 0)
    # constant components: the sum of omega and the largest l, nothing to search
    assert E.regrid_fields(cuda(np.full((mesh.nP, 2), 0.75)), w, normalise=True) == 1.0
    assert E.field_solve_info() == (1, 1)
    I = engine(mesh, 1)
    I.regrid_values(cuda(np.broadcast_to(np.eye(2), (mesh.nP, 2, 2))))
    same_state(E, I, what=("grid",))


def test_refusals():
    mesh, _ = make_mesh("rect2_8")
    E = engine(mesh, 1)
    U, w = fields(mesh.Xp, 3), weights(3)
    for bad in (cuda(U).float(), torch.from_numpy(U), cuda(U)[:-1], cuda(np.concatenate([U, U]))):
        for call in (lambda: E.regrid_fields(bad, None, 1.0), lambda: E.regrid_fields(bad, None, normalise=True),
                     lambda: E.field_hessians(bad)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        E.regrid_fields(cuda(U), w[:2], 1.0)
    for alpha in (-2.0, float("nan"), float("inf")):
        for Ux in (cuda(U), U):
            with pytest.raises(mx.MMADMMError, match="alpha"):
                E.regrid_fields(Ux, w, alpha)
            with pytest.raises(mx.MMADMMError, match="alpha"):
                E.regrid_fields(Ux, w, alpha, normalise=True)
    with pytest.raises(mx.MMADMMError, match="alpha"):
        E.regrid_fields(U, w, 0.0)
    for badw in (0.0, -1.0, float("nan"), float("inf")):
        wb = w.copy()
        wb[2] = badw
        for call in (lambda: E.regrid_fields(cuda(U), wb, 1.0), lambda: E.regrid_fields(U, wb, normalise=True),
                     lambda: E.field_hessians(cuda(U), wb), lambda: E.field_hessians(U, wb)):
            with pytest.raises(mx.MMADMMError, match="weight"):
                call()
    L, dU = mx.lib(), cuda(U)
    H = np.zeros((mesh.nP, 3, 2, 2))
    torch.cuda.synchronize()
    for rc in (L.mmadmm_regrid_fields(E.h, 3, None, None, 1.0), L.mmadmm_regrid_fields_device(E.h, 3, None, None, 1.0, None),
               L.mmadmm_regrid_fields_huang(E.h, 3, None, None, 0.0, None),
               L.mmadmm_regrid_fields_huang_device(E.h, 3, None, None, 0.0, None, None),
               L.mmadmm_field_hessians(E.h, 3, None, None, mx._dp(H), None),
               L.mmadmm_field_hessians(E.h, 3, mx._dp(U), None, None, None),
               L.mmadmm_field_hessians_device(E.h, 3, dU.data_ptr(), None, None, None, None),
               L.mmadmm_regrid_fields(E.h, 0, mx._dp(U), None, 1.0), L.mmadmm_regrid_fields(E.h, 33, mx._dp(U), None, 1.0),
               L.mmadmm_regrid_fields_huang_device(E.h, 33, dU.data_ptr(), None, 0.0, None, None),
               L.mmadmm_field_hessians(E.h, 0, mx._dp(U), None, mx._dp(H), None)):
        assert rc == 1  # MMADMM_ERR_INVALID
    assert E.stats()["regrids"] == 0


def test_partitioned_engine_refuses():
    mesh, _ = make_mesh("rect2_5")
    M = mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(2, 1), rho=1000.0, tau=0.5, device=0)
    comm = mx.Comm.loopback(2)
    parts = [mx.Engine(M, 0.025, rank=r, nranks=2, comm=comm) for r in range(2)]
    for e in parts:
        U = np.zeros((e.nP, 2))
        for c in (lambda: e.regrid_fields(U, None, 1.0), lambda: e.regrid_fields(cuda(U), None, 1.0),
                  lambda: e.regrid_fields(U, normalise=True), lambda: e.regrid_fields(cuda(U), normalise=True),
                  lambda: e.field_hessians(U), lambda: e.field_hessians(cuda(U))):
            with pytest.raises(mx.MMADMMError, match="single rank only"):
                c()
