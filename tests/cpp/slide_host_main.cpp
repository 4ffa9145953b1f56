// slide_host_main.cpp -- a stand-alone driver of the host-only sliding boundary (csrc/host/slide.cpp:
// mmadmm_boundary_project_field and mmadmm_boundary_faces, with transfer.cpp's face-neighbour table),
// for builds under host sanitizers (-fsanitize=address,undefined): no device, no libmmadmm.so.
// Three meshes: the Kuhn-split unit square (corners pinned) and cube (its twelve edges pinned), and a
// ball of tetrahedra from a hub node to a lat-long sphere of M = 40 meridians (no pin; the poles' stars
// are 40 triangles).  Every node displaced, one node sent far along the boundary, one given a NaN.
// Prints one "<name> ok|FAIL" line per check.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mmadmm.h"

namespace mmx {
static std::string g_err;
void set_last_error(const std::string& msg) { g_err = msg; }
}  // namespace mmx

static int fails = 0;
static void report(const std::string& name, bool ok) {
  printf("%s %s\n", name.c_str(), ok ? "ok" : "FAIL");
  if (!ok) fails++;
}

struct TestMesh {
  int D = 2;
  std::vector<double> X;
  std::vector<int32_t> F, mask;
  long long expectFaces = 0;
  double h = 0;
};

static TestMesh grid(int D, int n) {
  TestMesh t;
  t.D = D;
  t.h = 1.0 / n;
  const int m = n + 1, nz = D == 3 ? m : 1;
  for (int k = 0; k < nz; ++k)
    for (int j = 0; j < m; ++j)
      for (int i = 0; i < m; ++i) {
        t.X.push_back((double)i / n);
        t.X.push_back((double)j / n);
        if (D == 3) t.X.push_back((double)k / n);
        int onSide = (i == 0 || i == n) + (j == 0 || j == n) + (D == 3 && (k == 0 || k == n));
        t.mask.push_back(onSide == 0 ? MMADMM_INTERIOR : onSide == 1 ? MMADMM_BOUNDARY_FREE : MMADMM_BOUNDARY_FIXED);
      }
  auto id = [&](int i, int j, int k) { return (k * m + j) * m + i; };
  static const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  for (int k = 0; k < (D == 3 ? n : 1); ++k)
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i) {
        if (D == 2) {
          const int a = id(i, j, 0), b = id(i + 1, j, 0), c = id(i + 1, j + 1, 0), d = id(i, j + 1, 0);
          for (int v : {a, b, c, a, c, d}) t.F.push_back(v);
        } else {
          for (const auto& p : perm) {  // Kuhn: the paths from (i, j, k) to the opposite corner
            int c[3] = {i, j, k};
            t.F.push_back(id(c[0], c[1], c[2]));
            for (int s = 0; s < 3; ++s) {
              c[p[s]]++;
              t.F.push_back(id(c[0], c[1], c[2]));
            }
          }
        }
      }
  t.expectFaces = D == 2 ? 4LL * n : 12LL * n * n;
  return t;
}

// node 0 at the centre, then a lat-long sphere of radius 0.45: north pole, R - 1 rings of M, south pole
static TestMesh hub(int M, int R) {
  TestMesh t;
  t.D = 3;
  const double pi = std::acos(-1.0), rad = 0.45;
  auto push = [&](double x, double y, double z, int type) {
    t.X.push_back(0.5 + rad * x);
    t.X.push_back(0.5 + rad * y);
    t.X.push_back(0.5 + rad * z);
    t.mask.push_back(type);
  };
  t.X = {0.5, 0.5, 0.5};
  t.mask = {MMADMM_INTERIOR};
  push(0, 0, 1, MMADMM_BOUNDARY_FREE);
  for (int r = 1; r < R; ++r)
    for (int i = 0; i < M; ++i) {
      const double th = pi * r / R, ph = 2.0 * pi * i / M;
      push(std::sin(th) * std::cos(ph), std::sin(th) * std::sin(ph), std::cos(th), MMADMM_BOUNDARY_FREE);
    }
  push(0, 0, -1, MMADMM_BOUNDARY_FREE);
  auto ring = [&](int r, int i) { return 2 + (r - 1) * M + (i % M); };
  const int north = 1, south = 2 + (R - 1) * M;
  auto tet = [&](int a, int b, int c) {
    for (int v : {0, a, b, c}) t.F.push_back(v);
  };
  for (int i = 0; i < M; ++i) {
    tet(north, ring(1, i), ring(1, i + 1));
    for (int r = 1; r < R - 1; ++r) {
      tet(ring(r, i), ring(r + 1, i), ring(r + 1, i + 1));
      tet(ring(r, i), ring(r + 1, i + 1), ring(r, i + 1));
    }
    tet(south, ring(R - 1, i + 1), ring(R - 1, i));
  }
  t.expectFaces = 2LL * M * (R - 1);
  t.h = rad * 2.0 * std::sin(pi / M) * std::sin(pi / R);  // the shortest edge: along the first ring
  return t;
}

static void run(const std::string& tag, const TestMesh& t, bool straight) {
  const int D = t.D, nP = (int)t.X.size() / D, nF = (int)t.F.size() / (D + 1);
  int nFaces = -1;
  report("faces_" + tag, mmadmm_boundary_faces(D, nP, nF, t.F.data(), &nFaces, nullptr) == MMADMM_OK &&
                             nFaces == t.expectFaces);
  std::vector<int32_t> faces((size_t)nFaces * D);
  mmadmm_boundary_faces(D, nP, nF, t.F.data(), nullptr, faces.data());
  std::vector<char> onFace(nP, 0);
  for (int32_t v : faces) onFace[v] = 1;
  int nSliding = 0;
  for (int v = 0; v < nP; ++v) nSliding += t.mask[v] == MMADMM_BOUNDARY_FREE && onFace[v];

  std::vector<double> X(t.X);
  unsigned seed = 2468u;
  auto rnd = [&] {  // [-1, 1)
    seed = seed * 1664525u + 1013904223u;
    return (double)(seed >> 8) / 8388608.0 - 1.0;
  };
  for (size_t i = 0; i < X.size(); ++i) X[i] += rnd() * 0.45 * t.h / std::sqrt((double)D);
  int vFar = -1, vNan = -1;
  for (int v = 0; v < nP; ++v)
    if (t.mask[v] == MMADMM_BOUNDARY_FREE && onFace[v]) {
      if (vFar < 0)
        vFar = v;
      else
        vNan = v;
    }
  // far: to the position of another sliding node well away, and off the surface
  for (int k = 0; k < D; ++k) X[(size_t)vFar * D + k] = t.X[(size_t)vNan * D + k] + 0.3 * t.h;
  X[(size_t)vNan * D] = std::nan("");
  const std::vector<double> Xin(X);
  std::vector<int32_t> anchor(nP);
  for (int v = 0; v < nP; ++v) anchor[v] = v;
  int counts[5] = {-1, -1, -1, -1, -1};
  double maxD2 = -1.0;
  report("project_" + tag, mmadmm_boundary_project_field(D, nP, t.X.data(), nF, t.F.data(), t.mask.data(), anchor.data(),
                                                         X.data(), counts, &maxD2) == MMADMM_OK);
  report("counts_" + tag, counts[0] + counts[1] + counts[2] + counts[3] == nSliding && counts[0] >= 1 && maxD2 > 0.0);
  bool untouched = true, invariant = true;
  for (int v = 0; v < nP; ++v) {
    const bool slides = t.mask[v] == MMADMM_BOUNDARY_FREE && onFace[v];
    if (!slides || v == vNan) {
      untouched &= std::memcmp(&X[(size_t)v * D], &Xin[(size_t)v * D], D * sizeof(double)) == 0 && anchor[v] == v;
      continue;
    }
    if (straight) {  // a coordinate exactly on a side
      bool on = false;
      for (int k = 0; k < D; ++k) on |= X[(size_t)v * D + k] == 0.0 || X[(size_t)v * D + k] == 1.0;
      invariant &= on;
    } else {  // between the inscribed and the circumscribed sphere
      double r2 = 0;
      for (int k = 0; k < D; ++k) r2 += (X[(size_t)v * D + k] - 0.5) * (X[(size_t)v * D + k] - 0.5);
      invariant &= std::sqrt(r2) <= 0.45 * (1.0 + 1e-13) && std::sqrt(r2) >= 0.45 * 0.5;
    }
  }
  report("untouched_" + tag, untouched);
  report("invariant_" + tag, invariant);
  std::vector<double> X2(X);
  std::vector<int32_t> anchor2(anchor);
  int c2[5];
  double m2 = -1.0;
  const int rc = mmadmm_boundary_project_field(D, nP, t.X.data(), nF, t.F.data(), t.mask.data(), anchor2.data(),
                                               X2.data(), c2, &m2);
  double moved = 0;
  for (size_t i = 0; i < X.size(); ++i)
    if (X[i] == X[i]) moved = std::fmax(moved, std::fabs(X2[i] - X[i]));
  // (a node whose search the hop limit ended carries on from its anchor: only then may anchors differ)
  report("idempotent_" + tag,
         rc == MMADMM_OK && moved <= 1e-13 * 2.0 && (counts[3] > 0 || anchor2 == anchor) && c2[3] == 0);
  int vIn = 0;  // the hub / an interior node: no vertex of the surface
  while (onFace[vIn]) ++vIn;
  anchor2[vFar] = vIn;
  report("bad_anchor_refused_" + tag,
         mmadmm_boundary_project_field(D, nP, t.X.data(), nF, t.F.data(), t.mask.data(), anchor2.data(), X2.data(), nullptr,
                                       nullptr) == MMADMM_ERR_INVALID);
}

int main() {
  run("square", grid(2, 8), true);
  run("cube", grid(3, 4), true);
  run("hub", hub(40, 3), false);
  return fails ? 1 : 0;
}
