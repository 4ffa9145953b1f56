// quality_host_main.cpp -- a stand-alone driver of the host-only mesh quality measures
// (csrc/host/quality.cpp: mmadmm_mesh_quality), for builds under host sanitizers
// (-fsanitize=address,undefined): no device, no libmmadmm.so.  Kuhn-split unit square / cube of n
// cells per side (a partial last block of 256 simplices in both); the identity map, a sheared copy
// under the constant monitor that makes it ideal, the constant reference simplex, a NaN node with an
// inverted simplex, and a refusal.  Prints one "<name> ok|FAIL" line per check.
#include <cmath>
#include <cstdint>
#include <cstdio>
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

static void grid(int D, int n, std::vector<double>& X, std::vector<int32_t>& F) {
  const int m = n + 1, nz = D == 3 ? m : 1;
  for (int k = 0; k < nz; ++k)
    for (int j = 0; j < m; ++j)
      for (int i = 0; i < m; ++i) {
        X.push_back((double)i / n);
        X.push_back((double)j / n);
        if (D == 3) X.push_back((double)k / n);
      }
  auto id = [&](int i, int j, int k) { return (k * m + j) * m + i; };
  static const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  for (int k = 0; k < (D == 3 ? n : 1); ++k)
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i) {
        if (D == 2) {
          const int a = id(i, j, 0), b = id(i + 1, j, 0), c = id(i + 1, j + 1, 0), d = id(i, j + 1, 0);
          for (int v : {a, b, c, a, c, d}) F.push_back(v);
        } else {
          for (const auto& p : perm) {  // Kuhn: the paths from (i, j, k) to the opposite corner
            int c[3] = {i, j, k};
            F.push_back(id(c[0], c[1], c[2]));
            for (int s = 0; s < 3; ++s) {
              c[p[s]]++;
              F.push_back(id(c[0], c[1], c[2]));
            }
          }
        }
      }
}

// positive orientation (the engine's re-orientation): swap local vertices 1 and 2 where det E < 0
static void orient(int D, const std::vector<double>& X, std::vector<int32_t>& F) {
  const int nF = (int)F.size() / (D + 1);
  for (int s = 0; s < nF; ++s) {
    int32_t* f = &F[(size_t)s * (D + 1)];
    double e[3][3] = {{0}};
    for (int j = 0; j < D; ++j)
      for (int k = 0; k < D; ++k) e[j][k] = X[(size_t)f[j + 1] * D + k] - X[(size_t)f[0] * D + k];
    const double det = D == 2 ? e[0][0] * e[1][1] - e[0][1] * e[1][0]
                              : e[0][0] * (e[1][1] * e[2][2] - e[1][2] * e[2][1]) -
                                    e[0][1] * (e[1][0] * e[2][2] - e[1][2] * e[2][0]) +
                                    e[0][2] * (e[1][0] * e[2][1] - e[1][1] * e[2][0]);
    if (det < 0) std::swap(f[1], f[2]);
  }
}

static void run(int D, int n) {
  const std::string tag = D == 2 ? "2d" : "3d";
  std::vector<double> Xc;
  std::vector<int32_t> F;
  grid(D, n, Xc, F);
  orient(D, Xc, F);
  const int nP = (int)Xc.size() / D, nF = (int)F.size() / (D + 1);
  std::vector<double> q((size_t)3 * nF, -1.0);
  double s[8];

  report("identity_map_" + tag,
         mmadmm_mesh_quality(D, nP, Xc.data(), Xc.data(), nF, F.data(), nullptr, nullptr, q.data(), s) == MMADMM_OK);
  double err = 0.0;
  for (int i = 0; i < 3 * nF; ++i) err = std::fmax(err, std::fabs(q[i] - 1.0));
  report("identity_values_" + tag, err <= 1e-14 && s[7] == 0.0 && std::fabs(s[6] - 1.0) <= 1e-12);

  // X = Xc B^T with B upper triangular, M = (B B^T)^-1 = B^-T B^-1 at every node
  const double B[3][3] = {{2.0, 0.5, 0.0}, {0.0, 1.0, 0.25}, {0.0, 0.0, 1.5}};
  double Bi[3][3] = {{0}};  // B^-1 by back substitution on the leading D x D block
  for (int c = 0; c < D; ++c)
    for (int r = D - 1; r >= 0; --r) {
      double v = r == c ? 1.0 : 0.0;
      for (int k = r + 1; k < D; ++k) v -= B[r][k] * Bi[k][c];
      Bi[r][c] = v / B[r][r];
    }
  std::vector<double> X((size_t)nP * D), M((size_t)nP * D * D);
  double detB = 1.0;
  for (int k = 0; k < D; ++k) detB *= B[k][k];
  for (int v = 0; v < nP; ++v) {
    for (int r = 0; r < D; ++r) {
      double a = 0.0;
      for (int k = 0; k < D; ++k) a += B[r][k] * Xc[(size_t)v * D + k];
      X[(size_t)v * D + r] = a;
    }
    for (int r = 0; r < D; ++r)
      for (int c = 0; c < D; ++c) {
        double a = 0.0;
        for (int k = 0; k < D; ++k) a += Bi[k][r] * Bi[k][c];
        M[(size_t)v * D * D + r * D + c] = a;
      }
  }
  report("affine_" + tag,
         mmadmm_mesh_quality(D, nP, X.data(), Xc.data(), nF, F.data(), nullptr, M.data(), q.data(), s) == MMADMM_OK);
  double ea = 0.0, eg = 0.0;
  for (int i = 0; i < nF; ++i) {
    ea = std::fmax(ea, std::fmax(std::fabs(q[(size_t)nF + i] - 1.0), std::fabs(q[(size_t)2 * nF + i] - 1.0)));
    eg = std::fmax(eg, std::fabs(q[i] - q[0]));
  }
  report("affine_values_" + tag, ea <= 1e-12 && eg <= 1e-12 * q[0] && q[0] > 1.0 && s[7] == 0.0 &&
                                     std::fabs(s[6] / detB - 1.0) <= 1e-12);

  // the constant reference simplex, the summary alone
  double Ehat[9] = {0};
  const double side = 1.0 / n;
  for (int k = 0; k < D; ++k) Ehat[k * D + k] = side;
  double s2[8];
  bool ok = mmadmm_mesh_quality(D, nP, X.data(), nullptr, nF, F.data(), Ehat, M.data(), nullptr, s2) == MMADMM_OK;
  report("constant_reference_" + tag, ok && s2[0] >= 1.0 - 1e-15 && s2[1] >= 1.0 - 1e-15 && s2[7] == 0.0 &&
                                          s2[5] == s[5] && s2[6] == s[6]);

  // a NaN node, and a node moved across the mesh: counted, +inf, and nothing else disturbed
  std::vector<double> Xb(X);
  Xb[0] = std::nan("");
  const int mid = (nP / 2);
  for (int k = 0; k < D; ++k) Xb[(size_t)mid * D + k] += 5.0;
  ok = mmadmm_mesh_quality(D, nP, Xb.data(), Xc.data(), nF, F.data(), nullptr, M.data(), q.data(), s) == MMADMM_OK;
  int ninf = 0;
  bool whole = true;
  for (int i = 0; i < nF; ++i) {
    const bool a = std::isinf(q[i]), b = std::isinf(q[(size_t)nF + i]), c = std::isinf(q[(size_t)2 * nF + i]);
    whole &= a == b && b == c;
    ninf += a;
  }
  report("invalid_" + tag, ok && whole && ninf > 0 && ninf < nF && s[7] == (double)ninf && std::isinf(s[0]) &&
                               std::isinf(s[3]) && std::isfinite(s[5]) && std::isfinite(s[6]) && s[5] > 0.0);
  report("both_null_refused_" + tag, mmadmm_mesh_quality(D, nP, X.data(), Xc.data(), nF, F.data(), nullptr, M.data(),
                                                         nullptr, nullptr) == MMADMM_ERR_INVALID);
}

int main() {
  run(2, 12);  // 288 triangles: one full block and a partial one
  run(3, 4);   // 384 tetrahedra
  return fails ? 1 : 0;
}
