// quality.cpp -- mmadmm_mesh_quality: Huang's alignment, geometry and equidistribution measures of a
// mesh on the host (no device needed), compiled from the very text the device kernels run
// (kernels/quality_math.h), with the device's fixed-shape sums restated here:
// bit-identical to mmadmm_quality / mmadmm_quality_device at the same positions, simplices and
// tensors.
#include <vector>

#include "../kernels/quality_math.h"
#include "common.h"

namespace mmx {
namespace {

// the device's fixed-shape sum R (kernels/block_reduce.h) on the host: block_sum's tree over 256
// lanes per block of 256 consecutive simplex ids (missing lanes 0.0), fin_sum over the partials
constexpr int kRB = 256;
double tree_sum(double* red) {
  for (int w = kRB / 2; w > 0; w >>= 1)
    for (int t = 0; t < w; ++t) red[t] = red[t] + red[t + w];
  return red[0];
}
double quality_sum_host(const std::vector<double>& val) {
  const size_t n = val.size();
  std::vector<double> part((n + kRB - 1) / kRB);
  double red[kRB];
  for (size_t b = 0; b < part.size(); ++b) {
    for (int t = 0; t < kRB; ++t) red[t] = b * kRB + t < n ? val[b * kRB + t] : 0.0;
    part[b] = tree_sum(red);
  }
  for (int t = 0; t < kRB; ++t) {
    double v = 0.0;
    for (size_t b = t; b < part.size(); b += kRB) v += part[b];
    red[t] = v;
  }
  return tree_sum(red);
}

template <int D>
void mesh_quality_host(const double* X, const double* Xc, int nF, const int32_t* F, const double* Ehat, const double* M,
                       double* q, double* summary) {
  constexpr int DD = D * D;
  std::vector<double> geo(nF), ali(nF), e(nF), c(nF), term[kQualitySums];
  for (auto& t : term) t.resize(nF);
  double mg = 0.0, ma = 0.0, me = 0.0;
  for (int s = 0; s < nF; ++s) {
    const int32_t* f = F + (size_t)s * (D + 1);
    double x[D + 1][D], eh[D][D], m[(D + 1) * DD];
    for (int n = 0; n < D + 1; ++n)
      for (int k = 0; k < D; ++k) x[n][k] = X[(size_t)f[n] * D + k];
    if (Xc) {
      for (int j = 0; j < D; ++j)
        for (int k = 0; k < D; ++k) eh[j][k] = Xc[(size_t)f[j + 1] * D + k] - Xc[(size_t)f[0] * D + k];
    } else {
      quality_ref_edges<D>(Ehat, eh);
    }
    if (M)
      for (int n = 0; n < D + 1; ++n)
        for (int i = 0; i < DD; ++i) m[n * DD + i] = M[(size_t)f[n] * DD + i];
    const QualityElem r = quality_element<D>(x, eh, M ? m : nullptr);
    geo[s] = r.geo;
    ali[s] = r.ali;
    e[s] = r.e;
    c[s] = r.c;
    term[0][s] = r.valid ? r.e : 0.0;
    term[1][s] = r.vol;
    term[2][s] = quality_c_term(r.c);
    term[3][s] = r.geo;
    term[4][s] = r.ali;
    term[5][s] = r.valid ? 0.0 : 1.0;
    mg = quality_max(mg, r.geo);
    ma = quality_max(ma, r.ali);
  }
  double sum[kQualitySums];
  for (int k = 0; k < kQualitySums; ++k) sum[k] = quality_sum_host(term[k]);
  for (int s = 0; s < nF; ++s) {
    e[s] = quality_eq(e[s], c[s], sum[0], sum[2]);
    me = quality_max(me, e[s]);
  }
  if (q)
    for (int s = 0; s < nF; ++s) {
      q[s] = geo[s];
      q[(size_t)nF + s] = ali[s];
      q[(size_t)2 * nF + s] = e[s];
    }
  if (summary) {
    summary[0] = mg;
    summary[1] = ma;
    summary[2] = me;
    summary[3] = sum[3] / (double)nF;
    summary[4] = sum[4] / (double)nF;
    summary[5] = sum[0];
    summary[6] = sum[1];
    summary[7] = sum[5];
  }
}

}  // namespace
}  // namespace mmx

extern "C" int mmadmm_mesh_quality(int dim, int nP, const double* Xp, const double* Xc, int nF, const int32_t* F,
                                   const double* Ehat, const double* M, double* q, double* summary) {
  return mmx::guarded([&] {
    const std::string who = "mmadmm_mesh_quality";
    if ((dim != 2 && dim != 3) || nP < 1 || nF < 1) throw mmx::Error(MMADMM_ERR_INVALID, who + ": bad dim / sizes");
    if (!Xp || !F) throw mmx::Error(MMADMM_ERR_INVALID, who + ": NULL array");
    if (!Xc && !Ehat) throw mmx::Error(MMADMM_ERR_INVALID, who + ": Ehat is required when Xc is NULL");
    if (!q && !summary) throw mmx::Error(MMADMM_ERR_INVALID, who + ": q and summary are both NULL");
    for (long long i = 0; i < (long long)nF * (dim + 1); ++i)
      if (F[i] < 0 || F[i] >= nP) throw mmx::Error(MMADMM_ERR_INVALID, who + ": simplex vertex id out of range");
    if (dim == 2)
      mmx::mesh_quality_host<2>(Xp, Xc, nF, F, Ehat, M, q, summary);
    else
      mmx::mesh_quality_host<3>(Xp, Xc, nF, F, Ehat, M, q, summary);
  });
}
