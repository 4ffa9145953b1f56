// field_math.h -- the arithmetic of the Hessian-recovered monitor (DESIGN.md §Monitor from a
// nodal field), one text for the device kernels (field_kernels.hip) and the host-only
// mmadmm_field_monitor (csrc/host/field_monitor.cpp).  Only + - * / sqrt and comparisons, every
// operation order fixed and every product rounded before it is added (-ffp-contract=off), so a
// restatement on IEEE doubles (tests/field_monitor_py.py) reproduces both bit for bit.
//
//   element   e_j = X[v_{j+1}] - X[v0], du_j = val[v_{j+1}] - val[v0]; g solves E^T g = du by the
//             adjugate divided by det; weight w = |det| / D!
//   node      r_v = (sum_s w_s g_s) / (sum_s w_s) over the incident simplices in ascending id,
//             both sums from 0.0; a node no simplex references (sum w = 0) gets 0
//   Hessian   g = r(u); G_ij = d_j g_i = r(g_i)_j; H_ij = 0.5 (G_ij + G_ji)
//   |H|       cyclic Jacobi with Rutishauser's rotation (2D: one; 3D: kFieldSweeps sweeps over
//             (0,1), (0,2), (1,2)), |H|_ij = sum_k (V_ik |lambda_k|) V_jk left to right, j >= i, mirrored
//   monitor   M_ij = delta_ij + |H|_ij / alpha
//   Huang     the normalised form (Huang's metric): l_k = |a_kk| the Jacobi diagonal,
//             d = ((1 + l_0 / alpha) (1 + l_1 / alpha)) [(1 + l_2 / alpha)]; 2D: c = root3(d), rho = c,
//             t = sqrt(c); 3D: s = root7(d), rho = s s, t = s; M_ij = (delta_ij + |H|_ij / alpha) / t, so
//             sqrt(det M) = rho; omega_v = (sum_s w_s) / (D + 1); alpha given, or solved from
//             sum_v omega_v rho_v(alpha) = 2 sum_v omega_v (field_solve_*)
//   several   components: A = w_0 |H_0| + w_1 |H_1| + ... in ascending order from the
//             first product, in the place of |H| above; Huang's l is the Jacobi diagonal of A
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MMX_FHD __host__ __device__ __forceinline__
#else
#define MMX_FHD inline
#endif

namespace mmx {

constexpr int kFieldSweeps = 6;  // 3D Jacobi sweeps (four converged on every test input)

// doubles per simplex of the element buffer for C value components: {w, g[c * D + d]}
template <int D>
constexpr int field_elem_stride(int C) {
  return 1 + C * D;
}

MMX_FHD double field_abs(double x) { return x < 0.0 ? -x : x; }

// one simplex: f = its D + 1 vertex ids, X positions (n x D), val values (C components per vertex,
// vertex v's at val[v ld .. v ld + C): ld >= C, so a batch of C columns of a wider array can be read
// in place); out = {w, g[C][D]}
template <int D, int C>
MMX_FHD void field_element_ld(const double* X, const double* val, int ld, const int* f, double* out) {
  double e[D][D], du[D][C];
#pragma unroll
  for (int j = 0; j < D; ++j) {
#pragma unroll
    for (int k = 0; k < D; ++k) e[j][k] = X[(size_t)f[j + 1] * D + k] - X[(size_t)f[0] * D + k];
#pragma unroll
    for (int c = 0; c < C; ++c) du[j][c] = val[(size_t)f[j + 1] * ld + c] - val[(size_t)f[0] * ld + c];
  }
  if (D == 2) {
    const double det = e[0][0] * e[1][1] - e[0][1] * e[1][0];
    out[0] = field_abs(det) / 2.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      out[1 + c * D + 0] = (e[1][1] * du[0][c] - e[0][1] * du[1][c]) / det;
      out[1 + c * D + 1] = (e[0][0] * du[1][c] - e[1][0] * du[0][c]) / det;
    }
  } else {
    // the adjugate's columns: c0 = e1 x e2, c1 = e2 x e0, c2 = e0 x e1; det = e0 . c0
    double cr[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double* a = e[(j + 1) % 3];
      const double* b = e[(j + 2) % 3];
      cr[j][0] = a[1] * b[2] - a[2] * b[1];
      cr[j][1] = a[2] * b[0] - a[0] * b[2];
      cr[j][2] = a[0] * b[1] - a[1] * b[0];
    }
    const double det = (e[0][0] * cr[0][0] + e[0][1] * cr[0][1]) + e[0][2] * cr[0][2];
    out[0] = field_abs(det) / 6.0;
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int k = 0; k < 3; ++k)
        out[1 + c * D + k] = ((du[0][c] * cr[0][k] + du[1][c] * cr[1][k]) + du[2][c] * cr[2][k]) / det;
  }
}

// val n x C: C components per vertex, nothing between them
template <int D, int C>
MMX_FHD void field_element(const double* X, const double* val, const int* f, double* out) {
  field_element_ld<D, C>(X, val, C, f, out);
}

// one node: off[0 .. cnt) its incident slot offsets s K + n D in ascending simplex id (the
// x-update's incidence list), ebuf the element buffer; r = the recovered gradient (C x D)
// (the rows of kFieldChunk incident simplices are loaded before any is added -- that many gathers
// in flight per lane -- and then added one by one in list order: the sums are those of a plain loop)
constexpr int kFieldChunk = 4;

// one row of the element buffer into registers; rows of an even number of doubles (3D: 4, 10) are
// 16-byte aligned in a 16-byte aligned buffer and go as 16-byte loads on the device
template <int S>
MMX_FHD void field_load_row(const double* eb, double* row) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (S % 2 == 0) {
    const double2* p = reinterpret_cast<const double2*>(eb);
#pragma unroll
    for (int i = 0; i < S / 2; ++i) {
      const double2 q = p[i];
      row[2 * i] = q.x;
      row[2 * i + 1] = q.y;
    }
    return;
  }
#endif
#pragma unroll
  for (int i = 0; i < S; ++i) row[i] = eb[i];
}
template <int S>
MMX_FHD void field_store_row(const double* row, double* eb) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (S % 2 == 0) {
    double2* p = reinterpret_cast<double2*>(eb);
#pragma unroll
    for (int i = 0; i < S / 2; ++i) p[i] = make_double2(row[2 * i], row[2 * i + 1]);
    return;
  }
#endif
#pragma unroll
  for (int i = 0; i < S; ++i) eb[i] = row[i];
}

template <int D, int C>
MMX_FHD void field_node(const int* off, int cnt, const double* ebuf, double* r, double* swOut = nullptr) {
  constexpr int K = D * (D + 1), S = 1 + C * D;
  double sw = 0.0;
#pragma unroll
  for (int i = 0; i < C * D; ++i) r[i] = 0.0;
  int t = 0;
  for (; t + kFieldChunk <= cnt; t += kFieldChunk) {
    int s[kFieldChunk];
    double row[kFieldChunk][S];
#pragma unroll
    for (int j = 0; j < kFieldChunk; ++j) s[j] = off[t + j] / K;
#pragma unroll
    for (int j = 0; j < kFieldChunk; ++j) field_load_row<S>(ebuf + (size_t)s[j] * S, row[j]);
#pragma unroll
    for (int j = 0; j < kFieldChunk; ++j) {
      sw = sw + row[j][0];
#pragma unroll
      for (int i = 0; i < C * D; ++i) r[i] = r[i] + row[j][0] * row[j][1 + i];
    }
  }
  for (; t < cnt; ++t) {
    double row[S];
    field_load_row<S>(ebuf + (size_t)(off[t] / K) * S, row);
    sw = sw + row[0];
#pragma unroll
    for (int i = 0; i < C * D; ++i) r[i] = r[i] + row[0] * row[1 + i];
  }
#pragma unroll
  for (int i = 0; i < C * D; ++i) r[i] = (sw == 0.0) ? 0.0 : r[i] / sw;
  if (swOut) *swOut = sw;
}

// H_ij = 0.5 (G_ij + G_ji), G row-major (G_ij = d_j g_i)
template <int D>
MMX_FHD void field_symmetrise(const double* G, double* H) {
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) H[i * D + j] = 0.5 * (G[i * D + j] + G[j * D + i]);
}

// one Jacobi rotation of the pair (p, q) on the symmetric a (both triangles kept), v <- v R
template <int D>
MMX_FHD void field_rotate(double* a, double* v, int p, int q) {
  const double apq = a[p * D + q];
  if (apq == 0.0) return;
  const double theta = (a[q * D + q] - a[p * D + p]) / (2.0 * apq);
  const double at = field_abs(theta);
  const double tm = 1.0 / (at + __builtin_sqrt(theta * theta + 1.0));
  const double t = theta < 0.0 ? -tm : tm;
  const double c = 1.0 / __builtin_sqrt(t * t + 1.0);
  const double s = t * c;
  a[p * D + p] = a[p * D + p] - t * apq;
  a[q * D + q] = a[q * D + q] + t * apq;
  a[p * D + q] = 0.0;
  a[q * D + p] = 0.0;
#pragma unroll
  for (int r = 0; r < D; ++r) {
    if (r != p && r != q) {
      const double arp = a[r * D + p], arq = a[r * D + q];
      const double np = c * arp - s * arq, nq = s * arp + c * arq;
      a[r * D + p] = np;
      a[p * D + r] = np;
      a[r * D + q] = nq;
      a[q * D + r] = nq;
    }
    const double vrp = v[r * D + p], vrq = v[r * D + q];
    v[r * D + p] = c * vrp - s * vrq;
    v[r * D + q] = s * vrp + c * vrq;
  }
}

// |H| of the symmetric H; l (may be null): |a_kk|, the absolute Jacobi diagonal it is assembled from
template <int D>
MMX_FHD void field_abs_sym(const double* H, double* A, double* l = nullptr) {
  double a[D * D], v[D * D];
#pragma unroll
  for (int i = 0; i < D * D; ++i) {
    a[i] = H[i];
    v[i] = (i / D == i % D) ? 1.0 : 0.0;
  }
  if (D == 2) {
    field_rotate<D>(a, v, 0, 1);
  } else {
    for (int sweep = 0; sweep < kFieldSweeps; ++sweep) {
      field_rotate<D>(a, v, 0, 1);
      field_rotate<D>(a, v, 0, 2);
      field_rotate<D>(a, v, 1, 2);
    }
  }
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = i; j < D; ++j) {
      double s = (v[i * D + 0] * field_abs(a[0])) * v[j * D + 0];
#pragma unroll
      for (int k = 1; k < D; ++k) s = s + (v[i * D + k] * field_abs(a[k * D + k])) * v[j * D + k];
      A[i * D + j] = s;
      A[j * D + i] = s;
    }
  if (l) {
#pragma unroll
    for (int k = 0; k < D; ++k) l[k] = field_abs(a[k * D + k]);
  }
}

// the node epilogue: G (the second recovery, D x D) -> H and/or M = I + |H| / alpha (either may be null)
template <int D>
MMX_FHD void field_epilogue(const double* G, double alpha, double* H, double* M) {
  double h[D * D], ab[D * D];
  field_symmetrise<D>(G, h);
  if (H) {
#pragma unroll
    for (int i = 0; i < D * D; ++i) H[i] = h[i];
  }
  if (M) {
    field_abs_sym<D>(h, ab);
#pragma unroll
    for (int i = 0; i < D * D; ++i) M[i] = ((i / D == i % D) ? 1.0 : 0.0) + ab[i] / alpha;
  }
}

// ---- several components ------------------------------------------------------------
// the combined metric A = w_0 |H_0| + w_1 |H_1| + ..., one component per call in ascending c: the sum
// starts from its first product (first: Ain is not read), every product rounded before it is added
template <int D>
MMX_FHD void field_accumulate(const double* absH, double w, bool first, const double* Ain, double* Aout) {
#pragma unroll
  for (int i = 0; i < D * D; ++i) Aout[i] = first ? w * absH[i] : Ain[i] + w * absH[i];
}
// M = I + A / alpha
template <int D>
MMX_FHD void field_plain_monitor(const double* A, double alpha, double* M) {
#pragma unroll
  for (int i = 0; i < D * D; ++i) M[i] = ((i / D == i % D) ? 1.0 : 0.0) + A[i] / alpha;
}
// l_k = |a_kk| of the Jacobi on the combined metric A (field_abs_sym's l; its re-assembly is not used)
template <int D>
MMX_FHD void field_metric_diag(const double* A, double* l) {
  double re[D * D];
  field_abs_sym<D>(A, re, l);
}

// ---- Huang's normalised monitor ----------------------------------------------------------------

constexpr double kFieldMaxDouble = 1.7976931348623157e308;
constexpr double kFieldMinNormal = 2.2250738585072014e-308;

// exact scaling by powers of two: d = m 2^e with m in [1, 2) (d finite, normal, > 0), and 2^q for
// -1022 <= q <= 1023
MMX_FHD double field_split(double d, int* e) {
  unsigned long long b;
  __builtin_memcpy(&b, &d, 8);
  *e = (int)((b >> 52) & 0x7ffULL) - 1023;
  b = (b & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL;
  double m;
  __builtin_memcpy(&m, &b, 8);
  return m;
}
MMX_FHD double field_pow2(int q) {
  const unsigned long long b = (unsigned long long)(1023 + q) << 52;
  double p;
  __builtin_memcpy(&p, &b, 8);
  return p;
}

// the N-th root (N = 3, 7) of a finite d >= 1, within 1 ulp on every argument tried (the bound the
// tests hold it to is 4); 1.0 -> 1.0 exactly, inf / NaN -> themselves.  d = m 2^e, e = q N + r with
// 0 <= r < N, x = m 2^r in [1, 2^N): root(d) = root(x) 2^q.  Start y = ((c2 m + c1) m + c0) 2^(r/N)
// (a quadratic for m^(1/N) on [1, 2), relative error < 7.2e-4, times a tabulated constant), then
// three Newton steps y <- y + (x / y^(N-1) - y) (1/N), y^2 = y y, y^6 = (y^2 y)(y^2 y): one
// division each.  A fixed count: the error goes 7.2e-4 -> 1.6e-6 -> 8e-12 -> rounding for N = 7.
template <int N>
MMX_FHD double field_root(double d) {
  static_assert(N == 3 || N == 7, "root3 and root7 only");
  if (d == 1.0 || !(d <= kFieldMaxDouble)) return d;
  int e;
  const double m = field_split(d, &e);
  const int q = e / N, r = e - q * N;
  const double x = m * field_pow2(r);
  double y;
  if (N == 3) {
    const double tab[3] = {1.0, 1.2599210498948732, 1.5874010519681994};
    y = ((-0.05965740676787307 * m + 0.4374729459679123) * m + 0.6228944233278514) * tab[r];
  } else {
    const double tab[7] = {1.0,
                           1.1040895136738123,
                           1.2190136542044754,
                           1.3459001926323562,
                           1.4859942891369484,
                           1.640670712015276,
                           1.8114473285278132};
    y = ((-0.030509945641418488 * m + 0.19480296734660044) * m + 0.8361453064203973) * tab[r];
  }
  constexpr double inv = 1.0 / N;
#pragma unroll
  for (int it = 0; it < 3; ++it) {
    double p = y * y;
    if (N == 7) {
      const double y3 = p * y;
      p = y3 * y3;
    }
    y = y + (x / p - y) * inv;
  }
  return y * field_pow2(q);
}

// rho_v = sqrt(det M_v) of the normalised monitor from the Jacobi diagonal l (D values); t (may be
// null): the divisor of M
template <int D>
MMX_FHD double field_huang_rho(const double* l, double alpha, double* t) {
  double d = (1.0 + l[0] / alpha) * (1.0 + l[1] / alpha);
  if (D == 3) d = d * (1.0 + l[2] / alpha);
  if (D == 2) {
    const double c = field_root<3>(d);
    if (t) *t = __builtin_sqrt(c);
    return c;
  }
  const double s = field_root<7>(d);
  if (t) *t = s;
  return s * s;
}

// the second recovery of one node (G, D x D, and sw its sum of simplex weights) -> H (may be
// null), |H|, l and omega
template <int D>
MMX_FHD void field_huang_node(const double* G, double sw, double* H, double* A, double* l, double* omega) {
  double h[D * D];
  field_symmetrise<D>(G, h);
  if (H) {
#pragma unroll
    for (int i = 0; i < D * D; ++i) H[i] = h[i];
  }
  field_abs_sym<D>(h, A, l);
  *omega = sw / (double)(D + 1);
}

// M = (I + |H| / alpha) / t
template <int D>
MMX_FHD void field_huang_monitor(const double* A, const double* l, double alpha, double* M) {
  double t;
  field_huang_rho<D>(l, alpha, &t);
#pragma unroll
  for (int i = 0; i < D * D; ++i) M[i] = (((i / D == i % D) ? 1.0 : 0.0) + A[i] / alpha) / t;
}

// the solve of sigma(alpha) = sum_v omega_v rho_v(alpha) = 2 Omega, a state record advanced once
// per evaluated sum (on the device by the one-workgroup update kernel, on the host by a loop):
//   kFieldInit    the pass that sums Omega and takes Lambda = max l is pending
//   kFieldHalve   trial = hi / 2 is being evaluated (lo == hi: the last trial with sigma <= 2 Omega)
//   kFieldBisect  trial = lo + (hi - lo) / 2 is being evaluated
//   kFieldDone    alpha holds the result
enum FieldPhase { kFieldInit = 0, kFieldHalve = 1, kFieldBisect = 2, kFieldDone = 3 };
struct FieldSolve {
  double lo, hi, trial, twoOmega, lambda, alpha;
  int phase, passes;  // passes: sums evaluated, the Omega pass included
};

MMX_FHD void field_solve_bisect(FieldSolve* s) {
  const double mid = s->lo + (s->hi - s->lo) / 2.0;
  if (mid == s->lo || mid == s->hi) {
    s->alpha = s->hi;
    s->phase = kFieldDone;
  } else {
    s->trial = mid;
    s->phase = kFieldBisect;
  }
}
MMX_FHD void field_solve_halve(FieldSolve* s) {
  const double cand = s->hi * 0.5;
  if (cand < kFieldMinNormal) {  // would underflow: lo == hi, the bisection ends at once
    field_solve_bisect(s);
  } else {
    s->trial = cand;
    s->phase = kFieldHalve;
  }
}
// after the first pass: Omega and Lambda.  No root (nothing curved, no volume, or a non-finite
// input): alpha = 1.0
MMX_FHD void field_solve_begin(FieldSolve* s, double Omega, double Lambda) {
  s->passes = 1;
  s->twoOmega = 2.0 * Omega;
  s->lambda = Lambda;
  if (!(Lambda > 0.0 && Lambda <= kFieldMaxDouble && Omega > 0.0 && Omega <= kFieldMaxDouble)) {
    s->alpha = 1.0;
    s->phase = kFieldDone;
    return;
  }
  s->lo = Lambda;
  s->hi = Lambda;
  field_solve_halve(s);
}
// after a pass at s->trial: sigma its sum.  A sum that is not <= 2 Omega (inf and NaN included) is
// too large
MMX_FHD void field_solve_advance(FieldSolve* s, double sigma) {
  s->passes = s->passes + 1;
  const bool large = !(sigma <= s->twoOmega);
  if (s->phase == kFieldHalve) {
    s->lo = s->trial;
    if (large) {
      field_solve_bisect(s);
    } else {
      s->hi = s->trial;
      field_solve_halve(s);
    }
  } else {
    if (large)
      s->lo = s->trial;
    else
      s->hi = s->trial;
    field_solve_bisect(s);
  }
}

}  // namespace mmx
