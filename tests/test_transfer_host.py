"""mmadmm_transfer_field (host only, no GPU): nodal fields carried from the old node positions to the
new ones against the Python-float restatement (tests/transfer_py.py), bit for bit,
and the properties of the transfer: constants and linear fields reproduced, unmoved nodes copied,
contained nodes within the range of their simplex, a node moved across several simplices walked to,
a node moved out of the mesh flagged and extrapolated; the face-neighbour table; the refusals.

The project's rect meshes carry cell centres: rect(2, 17) has 613 nodes and rect(3, 6) 559, so both
span more than two 256-node blocks with a partial one.  The hub meshes (tests/hub_meshes.py) put 6 to 168
simplices at one node: their patch search runs whole chunks of 4 with every remainder, and their own
move "hubwalk" starts walks at that node and beside it."""
import functools

import numpy as np
import pytest

import mmadmm_amd as mx
import transfer_py
from transfer_cases import (ALL_MESHES, CASES, HUB_MESHES, MESHES, centre_node, fields, hubwalk_nodes, linear, make_mesh,
                            moved, unreferenced)

KEYS = mx.TRANSFER_COUNTS


@functools.lru_cache(maxsize=None)
def host(name, move, C):
    mesh, h, F = make_mesh(name)
    Xn = moved(name, move)
    u = fields(mesh.Xp, C)
    un, info = mx.transfer_field(mesh.Xp, F, Xn, u)
    return Xn, u, un, info


def counts(info):
    return [info[k] for k in KEYS]


def brute_force(X, F, p):
    """the simplices of (X, F) that contain p to 1e-12, by numpy.linalg.solve over all of them"""
    D = X.shape[1]
    A = np.swapaxes(X[F[:, 1:]] - X[F[:, :1]], 1, 2)  # columns e_j
    lam = np.linalg.solve(A, np.broadcast_to((p - X[F[:, 0]])[:, :, None], (F.shape[0], D, 1)))[:, :, 0]
    lam0 = 1.0 - lam.sum(axis=1)
    return np.nonzero(np.minimum(lam.min(axis=1), lam0) >= -1e-12)[0]


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name,move", CASES)
def test_host_equals_restatement(name, move, C):
    mesh, h, F = make_mesh(name)
    Xn, u, un, info = host(name, move, C)
    r_u, r_where, r_counts = transfer_py.transfer(mesh.Xp.tolist(), F.tolist(), Xn.tolist(), u.tolist())
    assert np.array_equal(np.array(r_u), un)
    assert np.array_equal(np.array(r_where, dtype=np.int32), info["where"])
    assert r_counts == counts(info)
    assert sum(counts(info)) == mesh.nP


@pytest.mark.parametrize("name,move", CASES)
def test_components_are_independent(name, move):
    mesh, h, F = make_mesh(name)
    Xn, u, un, info = host(name, move, 3)
    for c in range(3):
        u1, i1 = mx.transfer_field(mesh.Xp, F, Xn, u[:, c])
        assert u1.shape == (mesh.nP,)
        assert np.array_equal(u1, un[:, c])
        assert np.array_equal(i1["where"], info["where"]) and counts(i1) == counts(info)


@pytest.mark.parametrize("name,move", CASES)
def test_constant_and_linear_fields(name, move):
    mesh, h, F = make_mesh(name)
    Xn = moved(name, move)
    const = np.full(mesh.nP, 0.1 + 2.0 / 3.0)
    uc, _ = mx.transfer_field(mesh.Xp, F, Xn, const)
    assert np.array_equal(uc, const)
    lin = linear(mesh.Xp)
    ul, _ = mx.transfer_field(mesh.Xp, F, Xn, lin)
    lone = unreferenced(mesh.nP, F)  # copied, and not moved by any of the displacements
    assert np.array_equal(Xn[lone], mesh.Xp[lone])
    err = np.abs(ul - linear(Xn)).max()
    print(f"{name} {move}: linear field error {err:.3e}, max|u| {np.abs(lin).max():.3f}")
    assert err <= 1e-13 * np.abs(lin).max()


@pytest.mark.parametrize("name,move", CASES)
def test_unmoved_nodes_are_copied(name, move):
    mesh, h, F = make_mesh(name)
    Xn, u, un, info = host(name, move, 3)
    same = (Xn.view(np.int64) == np.ascontiguousarray(mesh.Xp).view(np.int64)).all(axis=1)
    lone = np.zeros(mesh.nP, dtype=bool)
    lone[unreferenced(mesh.nP, F)] = True
    copied = same | lone
    assert np.array_equal(info["where"] == -1, copied)
    assert np.array_equal(un[copied], u[copied])
    assert info["copied"] == int(copied.sum())
    if name.startswith("shoulder"):
        assert lone.any()


@pytest.mark.parametrize("name,move", CASES)
def test_contained_nodes_stay_in_range(name, move):
    mesh, h, F = make_mesh(name)
    Xn, u, un, info = host(name, move, 3)
    w = info["where"]
    inside = np.nonzero(w >= 0)[0]
    assert inside.size == info["patch"] + info["walked"]
    corner = u[F[w[inside]]]  # n x (D + 1) x C
    lo, hi = corner.min(axis=1), corner.max(axis=1)
    pad = 1e-12 * (hi - lo)
    assert (un[inside] >= lo - pad).all() and (un[inside] <= hi + pad).all()


@pytest.mark.parametrize("name", ALL_MESHES)
@pytest.mark.parametrize("move", ["a0.1", "a0.45"])
def test_small_moves_stay_in_the_patch(name, move):
    # a = 0.1 is inside the star of every interior node (inradius >= h / sqrt(3)); at a = 0.45 the
    # host function found every node of these meshes in its patch as well.  A hub mesh's h is its
    # smallest altitude, and a node moved by less than that stays in its star.
    mesh, h, F = make_mesh(name)
    Xn, _, _, info = host(name, move, 1)
    assert info["patch"] > 0
    assert info["walked"] == 0 and info["outside"] == 0
    if name in HUB_MESHES:  # the hub itself moved, and an independent search finds it in one of its own simplices
        assert (Xn[0] != mesh.Xp[0]).any()
        assert info["patch"] == int((mesh.mask == mx.INTERIOR).sum())
        assert all((F[s] == 0).any() for s in brute_force(np.asarray(mesh.Xp), F, Xn[0]))


@pytest.mark.parametrize("name", HUB_MESHES)
def test_hub_walk(name):
    """The hub moved out of its patch of 6 .. 168 simplices, and every third node of the first ring /
    shell into a hub simplex it is no vertex of: each is walked to, lands in a simplex an independent
    search over all simplices finds too, and the counts are that search's."""
    mesh, h, F = make_mesh(name)
    Xn, u, un, info = host(name, "hubwalk", 1)
    hub, movers, n_fan = hubwalk_nodes(mesh)
    assert n_fan == np.bincount(F.reshape(-1))[hub] and len(movers) >= 2
    X = np.asarray(mesh.Xp)
    want = dict.fromkeys(KEYS, 0)
    for v in range(mesh.nP):
        w = int(info["where"][v])
        if (Xn[v] == X[v]).all():
            want["copied"] += 1
            assert w == -1
            continue
        assert v == hub or v in movers
        holders = brute_force(X, F, Xn[v])
        assert holders.size == 1, "the targets lie inside one simplex, off its faces"
        assert not (F[holders[0]] == v).any(), "the target is outside the node's patch"
        want["walked"] += 1
        assert w == holders[0]
    assert info["where"][hub] >= n_fan, "the hub leaves the simplices at the hub"
    assert counts(info) == [want[k] for k in KEYS] == [mesh.nP - 1 - len(movers), 0, 1 + len(movers), 0]


@pytest.mark.parametrize("name", MESHES)
def test_big_move_is_walked(name):
    """The moved node's target lies several simplices away.  Where an independent search over all
    simplices finds it inside the mesh, it must be walked to; the shoulder mesh's target lies in
    the removed quadrant -- inside the box but in no simplex -- and must be flagged outside."""
    mesh, h, F = make_mesh(name)
    Xn, u, un, info = host(name, "big", 1)
    v = centre_node(mesh)
    holders = brute_force(np.asarray(mesh.Xp), F, Xn[v])
    w = int(info["where"][v])
    if holders.size:
        assert counts(info) == [mesh.nP - 1, 0, 1, 0]
        assert w >= 0 and v not in F[w]
        assert w in holders
    else:
        assert name.startswith("shoulder")
        assert counts(info) == [mesh.nP - 1, 0, 0, 1] and w <= -2


def test_big_move_is_inside_the_mesh_on_convex_domains():
    for name in MESHES:
        mesh, h, F = make_mesh(name)
        holders = brute_force(np.asarray(mesh.Xp), F, moved(name, "big")[centre_node(mesh)])
        assert bool(holders.size) == (not name.startswith("shoulder")), name


@pytest.mark.parametrize("name", MESHES)
def test_outside_move_is_flagged_and_extrapolated(name):
    mesh, h, F = make_mesh(name)
    Xn, u, un, info = host(name, "outside", 1)
    v = centre_node(mesh)
    w = int(info["where"][v])
    assert w <= -2 and info["outside"] == 1 and counts(info) == [mesh.nP - 1, 0, 0, 1]
    assert brute_force(np.asarray(mesh.Xp), F, Xn[v]).size == 0
    # the linear extrapolation from the simplex -2 - w, by an independent solve
    f = F[-2 - w]
    X = np.asarray(mesh.Xp)
    lam = np.linalg.solve((X[f[1:]] - X[f[0]]).T, Xn[v] - X[f[0]])
    want = u[f[0], 0] + lam @ (u[f[1:], 0] - u[f[0], 0])
    assert abs(un[v, 0] - want) <= 1e-12 * max(1.0, np.abs(u).max()) * max(1.0, np.abs(lam).max())


@pytest.mark.parametrize("name", ALL_MESHES)
def test_face_neighbour_table(name):
    mesh, h, F = make_mesh(name)
    nbr = mx.face_neighbours(F, mesh.nP)
    assert nbr.shape == F.shape
    assert np.array_equal(nbr, np.array(transfer_py.face_neighbours(F.tolist()), dtype=np.int32))
    for s in range(F.shape[0]):
        for j in range(F.shape[1]):
            t = nbr[s, j]
            if t >= 0:
                assert s in nbr[t]
                shared = set(F[s]) & set(F[t])
                assert len(shared) == mesh.dim and F[s, j] not in shared
    # boundary faces: those that occur once among all faces, counted in numpy
    faces = np.concatenate([np.sort(np.delete(F, j, axis=1), axis=1) for j in range(F.shape[1])])
    _, occ = np.unique(faces, axis=0, return_counts=True)
    assert occ.max() <= 2
    assert int((nbr == -1).sum()) == int((occ == 1).sum())


def test_stand_alone_driver():
    """tests/cpp/transfer_host_main.cpp with csrc/host/transfer.cpp as one program (no device, no
    libmmadmm.so): the driver that host-sanitizer builds of the transfer use, kept compiling and
    passing here in a plain build."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    build = os.path.join(root, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "transfer_host_main")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-D__HIP_PLATFORM_AMD__",
           "-isystem", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
           os.path.join(root, "tests", "cpp", "transfer_host_main.cpp"),
           os.path.join(root, "mm-admm_amd", "csrc", "host", "transfer.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 16 and all(ln.endswith(" ok") for ln in lines), r.stdout


def test_refusals():
    mesh, h, F = make_mesh("rect2_5")
    X = np.ascontiguousarray(mesh.Xp)
    u = fields(X, 1)
    out = np.zeros_like(u)
    L = mx.lib()
    dp, ip = mx._dp, mx._ip
    nP, nF = mesh.nP, F.shape[0]
    Fc = np.ascontiguousarray(F)

    def refused(rc, word):
        assert rc == 1  # MMADMM_ERR_INVALID
        assert word in L.mmadmm_last_error().decode()

    refused(L.mmadmm_transfer_field(2, nP, dp(X), nF, ip(Fc), dp(X), 0, dp(u), dp(out), None, None), "C must be")
    refused(L.mmadmm_transfer_field(2, nP, None, nF, ip(Fc), dp(X), 1, dp(u), dp(out), None, None), "NULL")
    refused(L.mmadmm_transfer_field(2, nP, dp(X), nF, ip(Fc), None, 1, dp(u), dp(out), None, None), "NULL")
    refused(L.mmadmm_transfer_field(2, nP, dp(X), nF, ip(Fc), dp(X), 1, None, dp(out), None, None), "NULL")
    refused(L.mmadmm_transfer_field(2, nP, dp(X), nF, ip(Fc), dp(X), 1, dp(u), None, None, None), "NULL")
    refused(L.mmadmm_transfer_field(2, nP, dp(X), nF, None, dp(X), 1, dp(u), dp(out), None, None), "NULL")
    refused(L.mmadmm_transfer_field(2, nP, dp(X), nF, ip(Fc), dp(X), 1, dp(u), dp(u), None, None), "unew must not be uold")
    refused(L.mmadmm_transfer_field(4, nP, dp(X), nF, ip(Fc), dp(X), 1, dp(u), dp(out), None, None), "bad dim")
    bad = Fc.copy()
    bad[3, 1] = nP
    refused(L.mmadmm_transfer_field(2, nP, dp(X), nF, ip(bad), dp(X), 1, dp(u), dp(out), None, None), "out of range")
    refused(L.mmadmm_face_neighbours(2, nP, nF, ip(bad), ip(np.zeros_like(bad))), "out of range")
    with pytest.raises(ValueError):
        mx.transfer_field(X, Fc, X, np.zeros((nP, 0)))
    with pytest.raises(ValueError):
        mx.transfer_field(X, Fc, X[:-1], u)
    # where and counts are optional
    assert L.mmadmm_transfer_field(2, nP, dp(X), nF, ip(Fc), dp(X), 1, dp(u), dp(out), None, None) == 0
    assert np.array_equal(out, u)
