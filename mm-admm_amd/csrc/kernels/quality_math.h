// quality_math.h -- the arithmetic of Huang's element-wise mesh quality measures, one
// text for the device kernels (quality_kernels.hip) and the host-only mmadmm_mesh_quality
// (csrc/host/quality.cpp).  Only + - * / sqrt and comparisons, every operation order fixed and every
// product rounded before it is added (-ffp-contract=off), so a restatement on IEEE doubles
// (tests/quality_py.py) reproduces both bit for bit.
//
//   edges     e_j = X[v_{j+1}] - X[v0] (the rows of e; E has them as columns), eh_j the same from Xc,
//             or column j of the engine's constant Ehat
//   det       2D: a00 a11 - a01 a10; 3D: (a0[0] c[0] + a0[1] c[1]) + a0[2] c[2], c = a1 x a2
//   M_K       ((M_v0 + M_v1) + M_v2 [+ M_v3]) / (D + 1), component by component; no tensors: I
//   valid     det E > 0, det Ehat < 0 or > 0, det M_K > 0 (a NaN fails each); decided before
//             anything is divided or rooted
//   J         J_ik = (sum_j e_j[i] cr_j[k]) / det Ehat, cr_j the columns of Ehat's adjugate (3D:
//             eh_{j+1} x eh_{j+2}; 2D: (eh_1[1], -eh_1[0]), (-eh_0[1], eh_0[0])), sums left to right
//   traces    T = M_K J (T_ik = sum_j M_ij J_jk); trA = sum_ik J_ik T_ik, trG = sum_ik J_ik J_ik,
//             both over (i, k) row-major, left to right
//   dets      r = det E / det Ehat; detG = r r; detA = detG det M_K
//   Q         t = tr / D; q = (t t [t]) / det; 2D: sqrt(q), 3D: sqrt(sqrt(q))
//   e_K       vol_K rho_K, vol_K = det E / D!, rho_K = sqrt(det M_K); c_K = |det Ehat| / D!
//   Q_eq      (e_K / sigma) / (c_K / Vhat), sigma = R(e_K), Vhat = R(c_K)
// An invalid simplex has all three measures +inf, adds 0.0 to sigma and |Omega| and its c_K to Vhat
// (0.0 when that c_K is not finite).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MMX_QHD __host__ __device__ __forceinline__
#else
#define MMX_QHD inline
#endif

namespace mmx {

constexpr double kQualityMaxDouble = 1.7976931348623157e308;
// the monitor sources (include/mmadmm.h: MMADMM_QUALITY_*)
enum QualitySource { kQualityIdentity = 0, kQualityValues = 1, kQualityLast = 2 };
// the sums of a pass, in the order of their partials: sigma, |Omega|, Vhat, sum Q_geo, sum Q_ali,
// the invalid count (0.0 / 1.0 per simplex: exact); then the two maxima
constexpr int kQualitySums = 6;
constexpr int kQualityPartials = 8;
// the record the finalisers write: the 8 doubles of the summary, then Vhat
constexpr int kQualityRecord = 9;
constexpr int kQualityVhat = 8;

MMX_QHD double quality_inf() { return __builtin_huge_val(); }
MMX_QHD double quality_abs(double x) { return x < 0.0 ? -x : x; }

// what one simplex contributes
struct QualityElem {
  double geo, ali, e, vol, c;
  bool valid;
};

// the columns of the adjugate of a (rows a_j) into cr, and det a
template <int D>
MMX_QHD double quality_adjugate(const double (*a)[D], double (*cr)[D]) {
  if (D == 2) {
    cr[0][0] = a[1][1];
    cr[0][1] = -a[1][0];
    cr[1][0] = -a[0][1];
    cr[1][1] = a[0][0];
    return a[0][0] * a[1][1] - a[0][1] * a[1][0];
  }
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const double* p = a[(j + 1) % D];
    const double* q = a[(j + 2) % D];
    cr[j][0] = p[1] * q[2 % D] - p[2 % D] * q[1];
    cr[j][1] = p[2 % D] * q[0] - p[0] * q[2 % D];
    cr[j][2 % D] = p[0] * q[1] - p[1] * q[0];
  }
  return (a[0][0] * cr[0][0] + a[0][1] * cr[0][1]) + a[0][2 % D] * cr[0][2 % D];
}

// Q from a trace and a determinant
template <int D>
MMX_QHD double quality_q(double tr, double det) {
  const double t = tr / (double)D;
  if (D == 2) return __builtin_sqrt((t * t) / det);
  return __builtin_sqrt(__builtin_sqrt(((t * t) * t) / det));
}

// one simplex: x its D + 1 vertex positions, eh the D edges of its reference simplex (rows), m the
// D + 1 vertex tensors (row-major, one after the other) or null for the identity
template <int D>
MMX_QHD QualityElem quality_element(const double (*x)[D], const double (*eh)[D], const double* m) {
  constexpr int DD = D * D;
  constexpr double fact = D == 2 ? 2.0 : 6.0;
  double e[D][D], cr[D][D], ce[D][D];
#pragma unroll
  for (int j = 0; j < D; ++j)
#pragma unroll
    for (int k = 0; k < D; ++k) e[j][k] = x[j + 1][k] - x[0][k];
  const double dE = quality_adjugate<D>(e, ce);
  const double dh = quality_adjugate<D>(eh, cr);
  double mk[D][D];
  double dM = 1.0;
  if (m) {
#pragma unroll
    for (int i = 0; i < DD; ++i) {
      double s = m[i] + m[DD + i];
#pragma unroll
      for (int n = 2; n < D + 1; ++n) s = s + m[n * DD + i];
      mk[i / D][i % D] = s / (double)(D + 1);
    }
    double cm[D][D];
    dM = quality_adjugate<D>(mk, cm);
  }
  QualityElem r;
  r.c = quality_abs(dh) / fact;
  r.valid = dE > 0.0 && (dh > 0.0 || dh < 0.0) && dM > 0.0;
  if (!r.valid) {
    r.geo = r.ali = r.e = quality_inf();
    r.vol = 0.0;
    return r;
  }
  double J[D][D];
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int k = 0; k < D; ++k) {
      double s = e[0][i] * cr[0][k];
#pragma unroll
      for (int j = 1; j < D; ++j) s = s + e[j][i] * cr[j][k];
      J[i][k] = s / dh;
    }
  const double rr = dE / dh;
  const double detG = rr * rr;
  double trG = J[0][0] * J[0][0];
#pragma unroll
  for (int i = 1; i < DD; ++i) trG = trG + J[i / D][i % D] * J[i / D][i % D];
  r.geo = quality_q<D>(trG, detG);
  r.vol = dE / fact;
  if (!m) {
    r.ali = r.geo;
    r.e = r.vol;
    return r;
  }
  double trA = 0.0;
#pragma unroll
  for (int i = 0; i < DD; ++i) {
    double t = mk[i / D][0] * J[0][i % D];
#pragma unroll
    for (int j = 1; j < D; ++j) t = t + mk[i / D][j] * J[j][i % D];
    trA = i == 0 ? J[0][0] * t : trA + J[i / D][i % D] * t;
  }
  r.ali = quality_q<D>(trA, detG * dM);
  r.e = r.vol * __builtin_sqrt(dM);
  return r;
}

// what an invalid simplex still adds to Vhat
MMX_QHD double quality_c_term(double c) { return c <= kQualityMaxDouble ? c : 0.0; }

// Q_eq of one simplex from its stored e_K (+inf: invalid)
MMX_QHD double quality_eq(double e, double c, double sigma, double vhat) {
  if (!(e <= kQualityMaxDouble)) return quality_inf();
  return (e / sigma) / (c / vhat);
}

// a maximum that starts from 0.0 and never takes a NaN
MMX_QHD double quality_max(double a, double b) { return b > a ? b : a; }

// row j of eh = column j of the engine's Ehat (D x D row-major)
template <int D>
MMX_QHD void quality_ref_edges(const double* Ehat, double (*eh)[D]) {
#pragma unroll
  for (int j = 0; j < D; ++j)
#pragma unroll
    for (int k = 0; k < D; ++k) eh[j][k] = Ehat[k * D + j];
}

}  // namespace mmx
