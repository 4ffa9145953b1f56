// field_monitor.cpp -- mmadmm_field_monitor: the Hessian-recovered monitor of a nodal scalar field
// on the host (no device needed), compiled from the very text the device kernels run
// (kernels/field_math.h; DESIGN.md §Monitor from a nodal field): bit-identical to
// mmadmm_field_hessian / mmadmm_regrid_field at the same positions and simplices.
#include <cmath>
#include <vector>

#include "../kernels/field_math.h"
#include "common.h"

namespace mmx {
namespace {

template <int D>
void field_monitor_host(int nP, const double* X, int nF, const int32_t* F, const double* u, double alpha, double* H,
                        double* M) {
  constexpr int K = D * (D + 1), DD = D * D;
  // node -> incident slot offsets s K + n D in ascending simplex id (the engine's incidence CSR)
  std::vector<int> ptr((size_t)nP + 1, 0), off((size_t)nF * (D + 1));
  for (size_t i = 0; i < (size_t)nF * (D + 1); ++i) ptr[F[i] + 1]++;
  for (int v = 0; v < nP; ++v) ptr[v + 1] += ptr[v];
  std::vector<int> fill(ptr.begin(), ptr.end() - 1);
  for (int s = 0; s < nF; ++s)
    for (int n = 0; n < D + 1; ++n) off[fill[F[(size_t)s * (D + 1) + n]]++] = s * K + n * D;
  std::vector<double> ebuf((size_t)nF * (1 + DD)), grad((size_t)nP * D);
  for (int s = 0; s < nF; ++s) {
    int f[D + 1];
    for (int n = 0; n < D + 1; ++n) f[n] = F[(size_t)s * (D + 1) + n];
    field_element<D, 1>(X, u, f, &ebuf[(size_t)s * (1 + D)]);
  }
  for (int v = 0; v < nP; ++v) field_node<D, 1>(off.data() + ptr[v], ptr[v + 1] - ptr[v], ebuf.data(), &grad[(size_t)v * D]);
  for (int s = 0; s < nF; ++s) {
    int f[D + 1];
    for (int n = 0; n < D + 1; ++n) f[n] = F[(size_t)s * (D + 1) + n];
    field_element<D, D>(X, grad.data(), f, &ebuf[(size_t)s * (1 + DD)]);
  }
  for (int v = 0; v < nP; ++v) {
    double G[DD];
    field_node<D, D>(off.data() + ptr[v], ptr[v + 1] - ptr[v], ebuf.data(), G);
    field_epilogue<D>(G, alpha, H ? H + (size_t)v * DD : nullptr, M ? M + (size_t)v * DD : nullptr);
  }
}

}  // namespace
}  // namespace mmx

extern "C" int mmadmm_field_monitor(int dim, int nP, const double* Xp, int nF, const int32_t* F, const double* u,
                                    double alpha, double* H, double* M) {
  return mmx::guarded([&] {
    if ((dim != 2 && dim != 3) || nP < 1 || nF < 0)
      throw mmx::Error(MMADMM_ERR_INVALID, "mmadmm_field_monitor: bad dim / sizes");
    if (!Xp || !u || (nF > 0 && !F)) throw mmx::Error(MMADMM_ERR_INVALID, "mmadmm_field_monitor: NULL array");
    if (M && !(std::isfinite(alpha) && alpha > 0))
      throw mmx::Error(MMADMM_ERR_INVALID, "mmadmm_field_monitor: alpha must be finite and > 0");
    for (long long i = 0; i < (long long)nF * (dim + 1); ++i)
      if (F[i] < 0 || F[i] >= nP) throw mmx::Error(MMADMM_ERR_INVALID, "simplex vertex id out of range");
    if (dim == 2)
      mmx::field_monitor_host<2>(nP, Xp, nF, F, u, alpha, H, M);
    else
      mmx::field_monitor_host<3>(nP, Xp, nF, F, u, alpha, H, M);
  });
}
