// field_monitor.cpp -- mmadmm_field_monitor and mmadmm_field_monitor_huang: the Hessian-recovered
// monitor of a nodal scalar field on the host (no device needed), compiled from the very text the
// device kernels run (kernels/field_math.h; DESIGN.md §Monitor from a nodal field): bit-identical to
// mmadmm_field_hessian / mmadmm_regrid_field / mmadmm_regrid_field_huang at the same positions and
// simplices.  mmadmm_fields_monitor is the same for several components: the twin of
// mmadmm_field_hessians / mmadmm_regrid_fields / mmadmm_regrid_fields_huang.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../kernels/field_math.h"
#include "common.h"

namespace mmx {
namespace {

// the two recoveries; node(v, G, sw) receives the second one (G, D x D) and the node's sum of
// simplex weights, v ascending
template <int D, class NodeFn>
void field_recover_host(int nP, const double* X, int nF, const int32_t* F, const double* u, NodeFn node) {
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
    double G[DD], sw;
    field_node<D, D>(off.data() + ptr[v], ptr[v + 1] - ptr[v], ebuf.data(), G, &sw);
    node(v, G, sw);
  }
}

template <int D>
void field_monitor_host(int nP, const double* X, int nF, const int32_t* F, const double* u, double alpha, double* H,
                        double* M) {
  constexpr int DD = D * D;
  field_recover_host<D>(nP, X, nF, F, u, [&](int v, const double* G, double) {
    field_epilogue<D>(G, alpha, H ? H + (size_t)v * DD : nullptr, M ? M + (size_t)v * DD : nullptr);
  });
}

// the device's fixed-shape sum (kernels/block_reduce.h) on the host: block_sum's tree over 256 lanes,
// and fin_sum over the per-block partials
constexpr int kRB = 256;
double tree_sum(double* red) {
  for (int w = kRB / 2; w > 0; w >>= 1)
    for (int t = 0; t < w; ++t) red[t] = red[t] + red[t + w];
  return red[0];
}
double fin_sum_host(const std::vector<double>& part) {
  double red[kRB];
  for (int t = 0; t < kRB; ++t) {
    double v = 0.0;
    for (size_t b = t; b < part.size(); b += kRB) v += part[b];
    red[t] = v;
  }
  return tree_sum(red);
}
// R(value(v)) over the node ids: each block 256 consecutive ids, missing lanes 0.0
template <class ValueFn>
double field_sum_host(int nP, ValueFn value) {
  std::vector<double> part((size_t)(nP + kRB - 1) / kRB);
  for (size_t b = 0; b < part.size(); ++b) {
    double red[kRB];
    for (int t = 0; t < kRB; ++t) {
      const long long v = (long long)b * kRB + t;
      red[t] = v < nP ? value((int)v) : 0.0;
    }
    part[b] = tree_sum(red);
  }
  return fin_sum_host(part);
}

// the device's search (field_math.h: field_solve_*) over l (nP x D) and om (nP), sum by sum
template <int D>
double field_solve_host(int nP, const std::vector<double>& l, const std::vector<double>& om) {
  double Lambda = 0.0;
  for (size_t i = 0; i < l.size(); ++i) Lambda = l[i] > Lambda ? l[i] : Lambda;
  FieldSolve st{};
  field_solve_begin(&st, field_sum_host(nP, [&](int v) { return om[v]; }), Lambda);
  while (st.phase != kFieldDone)
    field_solve_advance(&st, field_sum_host(nP, [&](int v) {
                          return om[v] * field_huang_rho<D>(&l[(size_t)v * D], st.trial, nullptr);
                        }));
  return st.alpha;
}

template <int D>
double field_monitor_huang_host(int nP, const double* X, int nF, const int32_t* F, const double* u, double alpha,
                                double* H, double* M) {
  constexpr int DD = D * D;
  std::vector<double> A((size_t)nP * DD), l((size_t)nP * D), om(nP);
  field_recover_host<D>(nP, X, nF, F, u, [&](int v, const double* G, double sw) {
    field_huang_node<D>(G, sw, H ? H + (size_t)v * DD : nullptr, &A[(size_t)v * DD], &l[(size_t)v * D], &om[v]);
  });
  if (!(alpha > 0.0)) alpha = field_solve_host<D>(nP, l, om);
  if (M)
    for (int v = 0; v < nP; ++v) field_huang_monitor<D>(&A[(size_t)v * DD], &l[(size_t)v * D], alpha, M + (size_t)v * DD);
  return alpha;
}

// the metric of C components: field_recover_host per column, the kernels' accumulation
// text; H nP x C x D*D, A and M nP x D*D, each may be null.  Returns the alpha M was (or would be) built with
template <int D>
double fields_monitor_host(int nP, const double* X, int nF, const int32_t* F, int C, const double* U, const double* w,
                           double alpha, bool normalise, double* H, double* Aout, double* M) {
  constexpr int DD = D * D;
  std::vector<double> A((size_t)nP * DD), om(nP), uc(nP);
  for (int c = 0; c < C; ++c) {
    for (int v = 0; v < nP; ++v) uc[v] = U[(size_t)v * C + c];
    field_recover_host<D>(nP, X, nF, F, uc.data(), [&](int v, const double* G, double sw) {
      double h[DD], ab[DD];
      field_symmetrise<D>(G, h);
      if (H)
        for (int i = 0; i < DD; ++i) H[((size_t)v * C + c) * DD + i] = h[i];
      field_abs_sym<D>(h, ab);
      double* Av = &A[(size_t)v * DD];
      field_accumulate<D>(ab, w ? w[c] : 1.0, c == 0, Av, Av);
      om[v] = sw / (double)(D + 1);
    });
  }
  if (Aout) std::copy(A.begin(), A.end(), Aout);
  if (!normalise) {
    if (M)
      for (int v = 0; v < nP; ++v) field_plain_monitor<D>(&A[(size_t)v * DD], alpha, M + (size_t)v * DD);
    return alpha;
  }
  std::vector<double> l((size_t)nP * D);
  for (int v = 0; v < nP; ++v) field_metric_diag<D>(&A[(size_t)v * DD], &l[(size_t)v * D]);
  if (!(alpha > 0.0)) alpha = field_solve_host<D>(nP, l, om);
  if (M)
    for (int v = 0; v < nP; ++v) field_huang_monitor<D>(&A[(size_t)v * DD], &l[(size_t)v * D], alpha, M + (size_t)v * DD);
  return alpha;
}

void check_field_arrays(const char* who, int dim, int nP, const double* Xp, int nF, const int32_t* F, const double* u) {
  if ((dim != 2 && dim != 3) || nP < 1 || nF < 0) throw Error(MMADMM_ERR_INVALID, std::string(who) + ": bad dim / sizes");
  if (!Xp || !u || (nF > 0 && !F)) throw Error(MMADMM_ERR_INVALID, std::string(who) + ": NULL array");
}

}  // namespace
}  // namespace mmx

extern "C" int mmadmm_field_monitor(int dim, int nP, const double* Xp, int nF, const int32_t* F, const double* u,
                                    double alpha, double* H, double* M) {
  return mmx::guarded([&] {
    mmx::check_field_arrays("mmadmm_field_monitor", dim, nP, Xp, nF, F, u);
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

extern "C" int mmadmm_field_monitor_huang(int dim, int nP, const double* Xp, int nF, const int32_t* F,
                                          const double* u, double alpha, double* alpha_used, double* H, double* M) {
  return mmx::guarded([&] {
    mmx::check_field_arrays("mmadmm_field_monitor_huang", dim, nP, Xp, nF, F, u);
    if (!(std::isfinite(alpha) && alpha >= 0))
      throw mmx::Error(MMADMM_ERR_INVALID, "mmadmm_field_monitor_huang: alpha must be finite and > 0, or 0 (solved)");
    for (long long i = 0; i < (long long)nF * (dim + 1); ++i)
      if (F[i] < 0 || F[i] >= nP) throw mmx::Error(MMADMM_ERR_INVALID, "simplex vertex id out of range");
    const double a = dim == 2 ? mmx::field_monitor_huang_host<2>(nP, Xp, nF, F, u, alpha, H, M)
                              : mmx::field_monitor_huang_host<3>(nP, Xp, nF, F, u, alpha, H, M);
    if (alpha_used) *alpha_used = a;
  });
}

extern "C" int mmadmm_fields_monitor(int dim, int nP, const double* Xp, int nF, const int32_t* F, int C,
                                     const double* U, const double* w, double alpha, int normalise,
                                     double* alpha_used, double* H, double* A, double* M) {
  return mmx::guarded([&] {
    const char* who = "mmadmm_fields_monitor";
    if (C < 1 || C > 32) throw mmx::Error(MMADMM_ERR_INVALID, std::string(who) + ": C must be 1 .. 32");
    mmx::check_field_arrays(who, dim, nP, Xp, nF, F, U);
    for (int c = 0; w && c < C; ++c)
      if (!(std::isfinite(w[c]) && w[c] > 0))
        throw mmx::Error(MMADMM_ERR_INVALID, std::string(who) + ": every weight must be finite and > 0");
    if (M && normalise && !(std::isfinite(alpha) && alpha >= 0))
      throw mmx::Error(MMADMM_ERR_INVALID, std::string(who) + ": alpha must be finite and > 0, or 0 (solved)");
    if (M && !normalise && !(std::isfinite(alpha) && alpha > 0))
      throw mmx::Error(MMADMM_ERR_INVALID, std::string(who) + ": alpha must be finite and > 0");
    for (long long i = 0; i < (long long)nF * (dim + 1); ++i)
      if (F[i] < 0 || F[i] >= nP) throw mmx::Error(MMADMM_ERR_INVALID, "simplex vertex id out of range");
    const double a = dim == 2 ? mmx::fields_monitor_host<2>(nP, Xp, nF, F, C, U, w, alpha, normalise != 0, H, A, M)
                              : mmx::fields_monitor_host<3>(nP, Xp, nF, F, C, U, w, alpha, normalise != 0, H, A, M);
    if (alpha_used) *alpha_used = a;
  });
}

extern "C" int mmadmm_field_root(int n, int count, const double* d, double* out) {
  return mmx::guarded([&] {
    if ((n != 3 && n != 7) || count < 0 || (count > 0 && (!d || !out)))
      throw mmx::Error(MMADMM_ERR_INVALID, "mmadmm_field_root: n is 3 or 7, d and out hold count values");
    for (int i = 0; i < count; ++i) out[i] = n == 3 ? mmx::field_root<3>(d[i]) : mmx::field_root<7>(d[i]);
  });
}
