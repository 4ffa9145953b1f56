// transfer_host_main.cpp -- a stand-alone driver of the host-only transfer (csrc/host/transfer.cpp:
// mmadmm_transfer_field and the face-neighbour table), for builds under host sanitizers
// (-fsanitize=address,undefined): no device, no libmmadmm.so.  Kuhn-split unit square / cube of
// n cells per side; every interior node displaced, one node moved several cells (walked), one moved
// out of the mesh (outside), C = 3 components.  Prints one "<name> ok|FAIL" line per check.
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

static void run(int D, int n) {
  const std::string tag = D == 2 ? "2d" : "3d";
  std::vector<double> X;
  std::vector<int32_t> F;
  grid(D, n, X, F);
  const int nP = (int)X.size() / D, nF = (int)F.size() / (D + 1), C = 3, m = n + 1;
  const double h = 1.0 / n;
  std::vector<int32_t> nbr(F.size());
  report("neighbours_" + tag, mmadmm_face_neighbours(D, nP, nF, F.data(), nbr.data()) == MMADMM_OK);
  long long boundary = 0;
  bool symmetric = true;
  for (int s = 0; s < nF; ++s)
    for (int j = 0; j < D + 1; ++j) {
      const int t = nbr[(size_t)s * (D + 1) + j];
      if (t < 0) {
        boundary++;
        continue;
      }
      bool back = false;
      for (int i = 0; i < D + 1; ++i) back |= nbr[(size_t)t * (D + 1) + i] == s;
      symmetric &= back;
    }
  report("neighbours_symmetric_" + tag, symmetric && boundary == (D == 2 ? 4LL * n : 12LL * n * n));

  std::vector<double> Xn(X), u((size_t)nP * C), out((size_t)nP * C, -1.0);
  unsigned seed = 12345u;
  auto rnd = [&] {  // [-1, 1)
    seed = seed * 1664525u + 1013904223u;
    return (double)(seed >> 8) / 8388608.0 - 1.0;
  };
  auto interior = [&](int v) {
    bool in = true;
    for (int k = 0; k < D; ++k) in &= X[(size_t)v * D + k] > 0.0 && X[(size_t)v * D + k] < 1.0;
    return in;
  };
  for (int v = 0; v < nP; ++v) {
    if (interior(v))
      for (int k = 0; k < D; ++k) Xn[(size_t)v * D + k] += rnd() * 0.3 * h / std::sqrt((double)D);
    for (int c = 0; c < C; ++c) u[(size_t)v * C + c] = 0.25 + (c + 1) * X[(size_t)v * D] - 2.0 * X[(size_t)v * D + D - 1];
  }
  const int mid = n / 2;
  const int vb = D == 2 ? mid * m + mid : (mid * m + mid) * m + mid;  // walked
  const int vo = vb + 1;                                                // outside
  const double big[3] = {2.3, 1.4, 0.6}, far[3] = {1.2, 0.4, 0.4};
  for (int k = 0; k < D; ++k) {
    Xn[(size_t)vb * D + k] = X[(size_t)vb * D + k] + big[k] * h;
    Xn[(size_t)vo * D + k] = far[k];
  }
  std::vector<int32_t> where(nP);
  int counts[4] = {0, 0, 0, 0};
  report("transfer_" + tag, mmadmm_transfer_field(D, nP, X.data(), nF, F.data(), Xn.data(), C, u.data(), out.data(),
                                                  where.data(), counts) == MMADMM_OK);
  report("walked_" + tag, where[vb] >= 0 && counts[2] >= 1);
  report("outside_" + tag, where[vo] <= -2 && counts[3] == 1);
  report("counts_" + tag, counts[0] + counts[1] + counts[2] + counts[3] == nP);
  double err = 0.0;  // the field is linear: reproduced everywhere, the outside node included
  for (int v = 0; v < nP; ++v)
    for (int c = 0; c < C; ++c)
      err = std::fmax(err, std::fabs(out[(size_t)v * C + c] -
                                     (0.25 + (c + 1) * Xn[(size_t)v * D] - 2.0 * Xn[(size_t)v * D + D - 1])));
  report("linear_" + tag, err <= 1e-13 * 4.0);
  report("alias_refused_" + tag, mmadmm_transfer_field(D, nP, X.data(), nF, F.data(), Xn.data(), C, u.data(), u.data(),
                                                       nullptr, nullptr) == MMADMM_ERR_INVALID);
}

int main() {
  run(2, 8);
  run(3, 5);
  return fails ? 1 : 0;
}
