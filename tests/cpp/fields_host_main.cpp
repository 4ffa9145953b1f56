// fields_host_main.cpp -- a stand-alone driver of the host-only monitor from several components
// (csrc/host/field_monitor.cpp: mmadmm_fields_monitor beside the scalar mmadmm_field_monitor(_huang)),
// for builds under host sanitizers (-fsanitize=address,undefined): no device, no libmmadmm.so.
// Kuhn-split unit square / cube of n cells per side, interior nodes displaced, C = 3 components of
// different shape and scale.  Prints one "<name> ok|FAIL" line per check.
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

static bool same(const double* a, const double* b, size_t n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }
static double rel(const std::vector<double>& a, const std::vector<double>& b) {
  double d = 0.0, s = 0.0;
  for (size_t i = 0; i < a.size(); ++i) {
    d = std::fmax(d, std::fabs(a[i] - b[i]));
    s = std::fmax(s, std::fabs(b[i]));
  }
  return s > 0.0 ? d / s : d;
}

static void run(int D, int n) {
  const std::string tag = D == 2 ? "2d" : "3d";
  std::vector<double> X;
  std::vector<int32_t> F;
  grid(D, n, X, F);
  const int nP = (int)X.size() / D, nF = (int)F.size() / (D + 1), C = 3, DD = D * D;
  const double h = 1.0 / n;
  unsigned seed = 12345u;
  auto rnd = [&] {  // [-1, 1)
    seed = seed * 1664525u + 1013904223u;
    return (double)(seed >> 8) / 8388608.0 - 1.0;
  };
  for (int v = 0; v < nP; ++v) {
    bool in = true;
    for (int k = 0; k < D; ++k) in &= X[(size_t)v * D + k] > 0.0 && X[(size_t)v * D + k] < 1.0;
    if (in)
      for (int k = 0; k < D; ++k) X[(size_t)v * D + k] += rnd() * 0.1 * h / std::sqrt((double)D);
  }
  std::vector<double> U((size_t)nP * C), u0(nP), UU((size_t)nP * 2);
  for (int v = 0; v < nP; ++v) {
    const double* x = &X[(size_t)v * D];
    double r2 = 0.0;
    for (int k = 0; k < D; ++k) r2 += (x[k] - 0.3) * (x[k] - 0.3);
    u0[v] = std::tanh(20.0 * (x[0] - 0.5 + 0.2 * x[1])) + x[D - 1] * x[D - 1];
    U[(size_t)v * C + 0] = u0[v];
    U[(size_t)v * C + 1] = 1e3 * std::exp(-50.0 * r2);
    U[(size_t)v * C + 2] = 3.0 * x[0] - 1.0;
    UU[(size_t)v * 2] = UU[(size_t)v * 2 + 1] = u0[v];
  }
  const double w[3] = {1.0, 1e-3, 1.0}, half[2] = {0.5, 0.5}, alpha = 3.7;
  const size_t nM = (size_t)nP * DD;
  std::vector<double> H(nM * C), A(nM), M(nM), Hs(nM), Ms(nM), A1(nM), A2(nM), M1(nM);
  double used = -1.0;

  report("plain_" + tag, mmadmm_fields_monitor(D, nP, X.data(), nF, F.data(), C, U.data(), w, alpha, 0, &used, H.data(),
                                               A.data(), M.data()) == MMADMM_OK && used == alpha);
  bool cols = true;
  std::vector<double> uc(nP);
  for (int c = 0; c < C; ++c) {
    for (int v = 0; v < nP; ++v) uc[v] = U[(size_t)v * C + c];
    cols &= mmadmm_field_monitor(D, nP, X.data(), nF, F.data(), uc.data(), 1.0, Hs.data(), nullptr) == MMADMM_OK;
    for (int v = 0; v < nP; ++v) cols &= same(&H[((size_t)v * C + c) * DD], &Hs[(size_t)v * DD], DD);
  }
  report("components_equal_scalar_" + tag, cols);
  bool sym = true;
  for (int v = 0; v < nP; ++v)
    for (int i = 0; i < D; ++i)
      for (int j = 0; j < D; ++j) {
        sym &= same(&A[(size_t)v * DD + i * D + j], &A[(size_t)v * DD + j * D + i], 1);
        sym &= same(&M[(size_t)v * DD + i * D + j], &M[(size_t)v * DD + j * D + i], 1);
      }
  report("symmetric_" + tag, sym);

  bool one = mmadmm_field_monitor(D, nP, X.data(), nF, F.data(), u0.data(), alpha, nullptr, Ms.data()) == MMADMM_OK &&
             mmadmm_fields_monitor(D, nP, X.data(), nF, F.data(), 1, u0.data(), nullptr, alpha, 0, nullptr, nullptr,
                                   A1.data(), M1.data()) == MMADMM_OK;
  report("one_component_plain_bitwise_" + tag, one && same(M1.data(), Ms.data(), nM));

  double solved = -1.0;
  report("huang_solved_" + tag, mmadmm_fields_monitor(D, nP, X.data(), nF, F.data(), C, U.data(), w, 0.0, 1, &solved,
                                                      nullptr, nullptr, M.data()) == MMADMM_OK &&
                                    solved > 0.0 && std::isfinite(solved));
  double a1 = -1.0, as = -2.0;
  bool hu = mmadmm_fields_monitor(D, nP, X.data(), nF, F.data(), 1, u0.data(), nullptr, 0.0, 1, &a1, nullptr, nullptr,
                                  M1.data()) == MMADMM_OK &&
            mmadmm_field_monitor_huang(D, nP, X.data(), nF, F.data(), u0.data(), 0.0, &as, nullptr, Ms.data()) ==
                MMADMM_OK;
  report("one_component_huang_close_" + tag, hu && std::fabs(a1 - as) <= 1e-12 * as && rel(M1, Ms) <= 1e-12);

  bool split = mmadmm_fields_monitor(D, nP, X.data(), nF, F.data(), 2, UU.data(), half, 1.0, 0, nullptr, nullptr,
                                     A2.data(), nullptr) == MMADMM_OK;
  report("split_weights_bitwise_" + tag, split && same(A2.data(), A1.data(), nM));

  std::vector<double> K((size_t)nP * C, 0.75);
  bool flat = mmadmm_fields_monitor(D, nP, X.data(), nF, F.data(), C, K.data(), w, 0.0, 1, &used, nullptr, A.data(),
                                    M.data()) == MMADMM_OK && used == 1.0;
  for (int v = 0; v < nP && flat; ++v)
    for (int i = 0; i < DD; ++i) flat &= A[(size_t)v * DD + i] == 0.0 && M[(size_t)v * DD + i] == (i / D == i % D ? 1.0 : 0.0);
  report("constant_components_" + tag, flat);

  const double bad[3] = {1.0, 0.0, 1.0};
  report("zero_weight_refused_" + tag, mmadmm_fields_monitor(D, nP, X.data(), nF, F.data(), C, U.data(), bad, alpha, 0,
                                                             nullptr, nullptr, A.data(), nullptr) == MMADMM_ERR_INVALID);
  report("count_refused_" + tag, mmadmm_fields_monitor(D, nP, X.data(), nF, F.data(), 33, U.data(), nullptr, alpha, 0,
                                                       nullptr, nullptr, A.data(), nullptr) == MMADMM_ERR_INVALID);
}

int main() {
  run(2, 8);
  run(3, 4);
  return fails ? 1 : 0;
}
