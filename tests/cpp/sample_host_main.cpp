// sample_host_main.cpp -- a stand-alone driver of the host-only point locator and field sampling
// (csrc/host/locate.cpp: mmadmm_sample_field, mmadmm_locator_field_info), for builds under host
// sanitizers (-fsanitize=address,undefined): no device, no libmmadmm.so.  Kuhn-split unit square /
// cube of n cells per side, every interior node displaced; query points made inside known simplices,
// one outside the mesh, one with a NaN; automatic, single-cell, uneven and fine cells, C = 3
// components.  Prints one "<name> ok|FAIL" line per check.
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
  const int nP = (int)X.size() / D, nF = (int)F.size() / (D + 1), C = 3;
  const double h = 1.0 / n;
  unsigned seed = 24680u;
  auto rnd = [&] {  // [0, 1)
    seed = seed * 1664525u + 1013904223u;
    return (double)(seed >> 8) / 16777216.0;
  };
  std::vector<double> u((size_t)nP * C);
  for (int v = 0; v < nP; ++v) {
    bool in = true;
    for (int k = 0; k < D; ++k) in &= X[(size_t)v * D + k] > 0.0 && X[(size_t)v * D + k] < 1.0;
    if (in)
      for (int k = 0; k < D; ++k) X[(size_t)v * D + k] += (2.0 * rnd() - 1.0) * 0.3 * h / std::sqrt((double)D);
  }
  auto lin = [&](const double* x, int c) { return 0.25 + (c + 1) * x[0] - 2.0 * x[D - 1]; };
  for (int v = 0; v < nP; ++v)
    for (int c = 0; c < C; ++c) u[(size_t)v * C + c] = lin(&X[(size_t)v * D], c);

  // interior points of known simplices (every lambda >= 0.05), then one outside the mesh, one NaN
  const int nIn = 300, nQ = nIn + 2;
  std::vector<double> Q((size_t)nQ * D);
  std::vector<int32_t> src(nIn);
  for (int i = 0; i < nIn; ++i) {
    const int s = (int)(rnd() * nF) % nF;
    src[i] = s;
    double lam[4], sum = 0.0;
    for (int j = 0; j < D + 1; ++j) sum += lam[j] = rnd() + 0.01;
    for (int j = 0; j < D + 1; ++j) lam[j] = 0.05 + (1.0 - 0.05 * (D + 1)) * lam[j] / sum;
    for (int k = 0; k < D; ++k) {
      double x = 0.0;
      for (int j = 0; j < D + 1; ++j) x += lam[j] * X[(size_t)F[(size_t)s * (D + 1) + j] * D + k];
      Q[(size_t)i * D + k] = x;
    }
  }
  for (int k = 0; k < D; ++k) {
    Q[(size_t)nIn * D + k] = k == 0 ? 1.07 : 0.4;
    Q[(size_t)(nIn + 1) * D + k] = k == 0 ? std::nan("") : 0.5;
  }

  const int g4 = 4 * n;
  const int ones[3] = {1, 1, 1}, uneven[3] = {7, 3, D == 3 ? 2 : 1}, fine[3] = {g4, g4, D == 3 ? g4 : 1};
  const int* choices[4] = {nullptr, ones, uneven, fine};
  std::vector<double> out0((size_t)nQ * C), out((size_t)nQ * C);
  std::vector<int32_t> where0(nQ), where(nQ);
  int counts[3] = {0, 0, 0};
  report("sample_" + tag, mmadmm_sample_field(D, nP, X.data(), nF, F.data(), nullptr, nQ, Q.data(), C, u.data(),
                                              out0.data(), where0.data(), counts) == MMADMM_OK);
  bool found = true;
  for (int i = 0; i < nIn; ++i) found &= where0[i] == src[i];
  report("interior_" + tag, found);
  report("counts_" + tag, counts[0] == nIn && counts[0] + counts[1] + counts[2] == nQ && counts[2] >= 1);
  bool same = true;
  for (int c = 1; c < 4; ++c) {
    int cnt[3];
    same &= mmadmm_sample_field(D, nP, X.data(), nF, F.data(), choices[c], nQ, Q.data(), C, u.data(), out.data(),
                                where.data(), cnt) == MMADMM_OK;
    for (int i = 0; i < nIn; ++i) same &= where[i] == where0[i];
    same &= std::memcmp(out.data(), out0.data(), sizeof(double) * nIn * C) == 0;
  }
  report("cells_do_not_matter_" + tag, same);
  // the single cell lists every simplex: the outside point is extrapolated, not lost
  int cnt1[3];
  mmadmm_sample_field(D, nP, X.data(), nF, F.data(), ones, nQ, Q.data(), C, u.data(), out.data(), where.data(), cnt1);
  report("outside_" + tag, where[nIn] <= -2 && cnt1[1] == 1);
  bool nan = where[nIn + 1] == -1 && cnt1[2] == 1;
  for (int c = 0; c < C; ++c) {
    unsigned long long b;
    std::memcpy(&b, &out[(size_t)(nIn + 1) * C + c], 8);
    nan &= b == 0x7ff8000000000000ull;
  }
  report("none_is_nan_" + tag, nan);
  double err = 0.0;  // the field is linear: reproduced everywhere, the outside point included
  for (int i = 0; i < nIn + 1; ++i)
    for (int c = 0; c < C; ++c) err = std::fmax(err, std::fabs(out[(size_t)i * C + c] - lin(&Q[(size_t)i * D], c)));
  report("linear_" + tag, err <= 1e-13 * 4.0);
  int used[3];
  double box[6];
  long long pairs = 0;
  int longest = 0;
  bool info = mmadmm_locator_field_info(D, nP, X.data(), nF, F.data(), fine, used, box, &pairs, &longest) == MMADMM_OK;
  info &= used[0] == g4 && pairs >= nF && longest >= 1 && box[0] == 0.0 && box[D] == 1.0;
  report("info_" + tag, info);
  std::vector<double> flat(X);
  for (int v = 0; v < nP; ++v) flat[(size_t)v * D] = 0.5;
  report("flat_box_refused_" + tag, mmadmm_sample_field(D, nP, flat.data(), nF, F.data(), nullptr, nQ, Q.data(), C,
                                                        u.data(), out.data(), nullptr, nullptr) == MMADMM_ERR_INVALID);
  const int bad[3] = {4, 0, 1};
  report("bad_cells_refused_" + tag, mmadmm_sample_field(D, nP, X.data(), nF, F.data(), bad, nQ, Q.data(), C, u.data(),
                                                         out.data(), nullptr, nullptr) == MMADMM_ERR_INVALID);
}

int main() {
  run(2, 8);
  run(3, 5);
  return fails ? 1 : 0;
}
