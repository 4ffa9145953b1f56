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

// one simplex: f = its D + 1 vertex ids, X positions (n x D), val values (n x C, C components
// per vertex); out = {w, g[C][D]}
template <int D, int C>
MMX_FHD void field_element(const double* X, const double* val, const int* f, double* out) {
  double e[D][D], du[D][C];
#pragma unroll
  for (int j = 0; j < D; ++j) {
#pragma unroll
    for (int k = 0; k < D; ++k) e[j][k] = X[(size_t)f[j + 1] * D + k] - X[(size_t)f[0] * D + k];
#pragma unroll
    for (int c = 0; c < C; ++c) du[j][c] = val[(size_t)f[j + 1] * C + c] - val[(size_t)f[0] * C + c];
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
MMX_FHD void field_node(const int* off, int cnt, const double* ebuf, double* r) {
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

// |H| of the symmetric H
template <int D>
MMX_FHD void field_abs_sym(const double* H, double* A) {
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

}  // namespace mmx
