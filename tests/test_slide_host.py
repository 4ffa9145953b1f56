"""mmadmm_boundary_project_field and mmadmm_boundary_faces (host only, no GPU): the sliding boundary's
projection against the Python-float restatement (tests/slide_py.py), bit for bit, and
its properties: the closest point over all boundary faces within the ranges the hop rule was checked
in, untouched nodes, exact coordinates on straight sides, the polygon's annulus, idempotence, the pin
and the hop limit, a NaN; the frozen faces against the face-neighbour table; the refusals.

Decided here: a position with a NaN finds no face (a NaN never compares smaller), so the node keeps
its bits and its anchor and is counted unmoved; every other node's result is what it is without the
NaN.  The move "far" can exhaust the eight hops only where no pinned vertex stops the search first:
on hexdisc(6) (a 36-gon without pins, 12 edges on) it is asserted; on hexdisc(3) the other way round
is 6 edges, on the square a side has 7 free vertices between two pins."""
import functools

import numpy as np
import pytest

import mmadmm_amd as mx
import slide_py
from slide_cases import BRUTE_MOVES, CASES, MESHES, MOVES, NOFREE, PINNED, brute_force, case, far_target_hops, moved, \
    special_node

KEYS = mx.SLIDE_COUNTS


@functools.lru_cache(maxsize=None)
def host(name, move):
    c = case(name)
    X = moved(name, move)
    Xn, an, info = mx.boundary_project(c.X0, c.F, c.mask, X)
    for a in (X, Xn, an):
        a.setflags(write=False)
    return X, Xn, an, info


def counts(info):
    return [info[k] for k in KEYS]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("name,move", CASES)
def test_host_equals_restatement(name, move):
    c = case(name)
    X, Xn, an, info = host(name, move)
    rX, ra, rc, rmax = slide_py.project(c.X0.tolist(), c.F.tolist(), c.mask.tolist(), X.tolist())
    assert same_bits(np.array(rX), Xn)
    assert np.array_equal(np.array(ra, dtype=np.int32), an)
    assert rc == counts(info)
    assert rmax == info["max_d2"]
    assert sum(rc[:4]) == len(c.sliding)


@pytest.mark.parametrize("name,move", CASES)
def test_only_sliding_nodes_are_touched(name, move):
    c = case(name)
    X, Xn, an, info = host(name, move)
    rest = np.ones(c.nP, dtype=bool)
    rest[c.sliding] = False
    assert same_bits(Xn[rest], X[rest])
    assert np.array_equal(an[rest], np.arange(c.nP)[rest])
    if name == "shoulder2_8":  # its mask has BOUNDARY_FREE nodes on no boundary face
        assert int((c.mask == mx.BOUNDARY_FREE).sum()) > len(c.sliding)
    if name == NOFREE:
        assert len(c.sliding) == 0 and counts(info) == [0] * 5 and info["max_d2"] == 0.0


@pytest.mark.parametrize("move", BRUTE_MOVES)
@pytest.mark.parametrize("name", MESHES)
def test_equals_closest_point_over_all_faces(name, move):
    c = case(name)
    X, Xn, an, info = host(name, move)
    want = brute_force(c, X)
    tol = 1e-13 * c.diam
    for v in c.sliding:
        assert np.abs(Xn[v] - want[int(v)]).max() <= tol, (name, move, int(v), Xn[v], want[int(v)])


@pytest.mark.parametrize("move", MOVES + ["corner"])
@pytest.mark.parametrize("name", PINNED)
def test_straight_sides_are_kept_exactly(name, move):
    """on the square every slid node has its edge coordinate exactly 0.0 or 1.0, on the cube its face
    coordinate; the Shoulder's sides lie at 0.0, 0.5 and 1.0"""
    c = case(name)
    X, Xn, an, info = host(name, move)
    sides = (0.0, 0.5, 1.0) if name.startswith("shoulder") else (0.0, 1.0)
    for v in c.sliding:
        if np.isnan(X[v]).any():
            continue
        on = [(k, s) for k in range(c.dim) for s in sides if c.X0[v, k] == s]
        assert on, "a sliding node of these meshes starts on a side"
        assert any(Xn[v, k] == s for k in range(c.dim) for s in sides), (int(v), Xn[v])
        if move in ("a0.2", "a0.45", "on", "nan"):  # the node cannot have left its own side
            assert any(Xn[v, k] == s for k, s in on)


@pytest.mark.parametrize("move", MOVES)
@pytest.mark.parametrize("name", ["hexdisc3", "hexdisc6"])
def test_polygon_results_lie_in_its_annulus(name, move):
    c = case(name)
    X, Xn, an, info = host(name, move)
    ctr = np.array([0.5, 0.5])
    V = c.X0[c.faces]  # nFaces x 2 x 2
    circ = float(np.linalg.norm(c.X0[np.unique(c.faces)] - ctr, axis=1).max())
    inr = float(np.linalg.norm(V.mean(axis=1) - ctr, axis=1).min())
    eps = 1e-13 * c.diam
    for v in c.sliding:
        if np.isnan(X[v]).any():
            continue
        r = float(np.linalg.norm(Xn[v] - ctr))
        assert inr - eps <= r <= circ + eps


@pytest.mark.parametrize("name,move", CASES)
def test_second_projection_moves_nothing(name, move):
    c = case(name)
    X, Xn, an, info = host(name, move)
    X2, a2, i2 = mx.boundary_project(c.X0, c.F, c.mask, Xn, anchor=an)
    ok = ~np.isnan(X).any(axis=1)
    assert np.abs(X2[ok] - Xn[ok]).max(initial=0.0) <= 1e-13 * c.diam
    if info["exhausted"] == 0:
        assert np.array_equal(a2, an)
    else:
        # a node whose search the hop limit ended is, by the hop rule itself, not at rest: its point
        # lies at the far end of its anchor's star and the second search hops on from there.  Every
        # other anchor is unchanged
        assert int((a2 != an).sum()) <= info["exhausted"]
    assert i2["max_d2"] <= (1e-13 * c.diam) ** 2
    assert i2["exhausted"] == 0


@pytest.mark.parametrize("name", ["rect2_4", "rect2_8"])
def test_along_ends_at_the_exact_foot(name):
    c = case(name)
    X, Xn, an, info = host(name, "along")
    v, w = special_node(c)
    e = (c.X0[w] - c.X0[v]) / c.h
    foot = c.X0[v] + 2.5 * c.h * e
    assert np.abs(Xn[v] - foot).max() <= 1e-13 * c.diam
    assert info["hopped"] == 1 and info["exhausted"] == 0
    assert info["max_d2"] == pytest.approx((0.3 * c.h) ** 2, rel=1e-12)
    # the anchor ended at a vertex of the segment the foot lies on, two or three vertices on
    d = np.linalg.norm(c.X0[an[v]] - c.X0[v]) / c.h
    assert round(d) in (2, 3) and abs(d - round(d)) < 1e-12


@pytest.mark.parametrize("name", ["rect2_4", "rect2_8", "shoulder2_8"])
def test_corner_is_counted_at_pin(name):
    c = case(name)
    X, Xn, an, info = host(name, "corner")
    v, w = c.pinned_pair()
    assert same_bits(Xn[v], c.X0[w])
    assert info["at_pin"] == 1 and an[v] == v
    # the unconstrained closest point rounds the corner
    assert np.abs(brute_force(c, X)[v] - c.X0[w]).max() > 0.1 * c.h


@pytest.mark.parametrize("name,move", CASES)
def test_at_pin_counts_results_on_pinned_vertices(name, move):
    c = case(name)
    X, Xn, an, info = host(name, move)
    pins = {c.X0[w].tobytes() for w in range(c.nP) if c.mask[w] == mx.BOUNDARY_FIXED}
    assert info["at_pin"] == sum(Xn[v].tobytes() in pins for v in c.sliding)


def test_far_exhausts_the_hops():
    assert far_target_hops("hexdisc6") == 12
    X, Xn, an, info = host("hexdisc6", "far")
    assert info["exhausted"] == 1
    c = case("hexdisc6")
    v, w = special_node(c)
    # eight hops on: the anchor is eight edges from the node
    ring = [v, w]
    for _ in range(7):
        ring.append([u for u in c.neighbours(ring[-1]) if u != ring[-2]][0])
    assert an[v] == ring[8]
    for name in ("hexdisc3", "rect2_4", "rect2_8", "shoulder2_8", "tri"):
        k = far_target_hops(name)
        assert k is None or k <= 8
        assert host(name, "far")[3]["exhausted"] == 0


@pytest.mark.parametrize("name", MESHES)
def test_nan_stays_and_affects_nothing_else(name):
    c = case(name)
    X, Xn, an, info = host(name, "nan")
    v = int(c.sliding[-1])
    assert same_bits(Xn[v], X[v]) and an[v] == v
    Xa, Xna, ana, ia = host(name, "a0.2")
    others = np.arange(c.nP) != v
    assert same_bits(Xn[others], Xna[others])
    assert np.array_equal(an[others], ana[others])


@pytest.mark.parametrize("name", MESHES + [NOFREE])
def test_boundary_faces(name):
    c = case(name)
    faces = mx.boundary_faces(c.F, c.nP)
    assert faces.dtype == np.int32 and np.array_equal(faces, c.faces)
    nbr = mx.face_neighbours(c.F, c.nP)
    assert len(faces) == int((nbr == -1).sum())
    k = 0
    for s in range(c.F.shape[0]):
        for j in range(c.dim + 1):
            if nbr[s, j] == -1:
                assert np.array_equal(faces[k], np.delete(c.F[s], j))
                k += 1
    assert k == len(faces)
    if name not in ("hub3d_40_3_1",):  # (its mask is the test's own)
        assert (c.mask[faces] != mx.INTERIOR).all()


def test_stand_alone_driver():
    """tests/cpp/slide_host_main.cpp with csrc/host/slide.cpp and transfer.cpp as one program (no
    device, no libmmadmm.so): the driver that host-sanitizer builds of the projection use, kept
    compiling and passing here in a plain build."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    build = os.path.join(root, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "slide_host_main")
    host_dir = os.path.join(root, "mm-admm_amd", "csrc", "host")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-D__HIP_PLATFORM_AMD__",
           "-isystem", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
           os.path.join(root, "tests", "cpp", "slide_host_main.cpp"), os.path.join(host_dir, "slide.cpp"),
           os.path.join(host_dir, "transfer.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 21 and all(ln.endswith(" ok") for ln in lines), r.stdout


def test_refusals():
    c = case("rect2_4")
    L = mx.lib()
    dp, ip = mx._dp, mx._ip
    X0, F, mask = np.array(c.X0), np.array(c.F), np.array(c.mask)
    nP, nF = c.nP, F.shape[0]
    X = X0.copy()
    a = np.arange(nP, dtype=np.int32)
    cnt = np.zeros(5, dtype=np.int32)

    def refused(rc, word):
        assert rc == 1  # MMADMM_ERR_INVALID
        assert word in L.mmadmm_last_error().decode()

    ok = (2, nP, dp(X0), nF, ip(F), ip(mask), ip(a), dp(X), ip(cnt), None)
    assert L.mmadmm_boundary_project_field(*ok) == 0
    for k in (2, 4, 5, 6, 7):
        bad = list(ok)
        bad[k] = None
        refused(L.mmadmm_boundary_project_field(*bad), "NULL")
    refused(L.mmadmm_boundary_project_field(4, *ok[1:]), "bad dim")
    refused(L.mmadmm_boundary_project_field(2, nP, dp(X0), nF, ip(F), ip(mask), ip(a), dp(X0), None, None), "must not be X0")
    Fb = F.copy()
    Fb[3, 1] = nP
    refused(L.mmadmm_boundary_project_field(2, nP, dp(X0), nF, ip(Fb), ip(mask), ip(a), dp(X), None, None), "out of range")
    v = int(c.sliding[0])
    for wrong in (-1, nP, int(np.nonzero(c.mask == mx.INTERIOR)[0][0])):
        ab = a.copy()
        ab[v] = wrong
        refused(L.mmadmm_boundary_project_field(2, nP, dp(X0), nF, ip(F), ip(mask), ip(ab), dp(X), None, None), "anchor")
    n = np.zeros(1, dtype=np.int32)
    refused(L.mmadmm_boundary_faces(2, nP, nF, ip(F), None, None), "NULL")
    refused(L.mmadmm_boundary_faces(2, nP, nF, ip(Fb), ip(n), None), "out of range")
    with pytest.raises(ValueError):
        mx.boundary_project(X0, F, mask, X[:-1])
    with pytest.raises(ValueError):
        mx.boundary_project(X0, F, mask[:-1], X)
    with pytest.raises(ValueError):
        mx.boundary_project(X0, F, mask, X, anchor=a[:-1])
