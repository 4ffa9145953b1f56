// transfer_math.h -- the arithmetic of the nodal-field transfer onto the moved mesh (DESIGN.md
// §7e), one text for the device kernels (transfer_kernels.hip) and the host-only
// mmadmm_transfer_field (csrc/host/transfer.cpp).  Only + - * / and comparisons, every operation
// order fixed and every product rounded before it is added (-ffp-contract=off), so a restatement
// on IEEE doubles (tests/transfer_py.py) reproduces both bit for bit.
//
//   copy      p = Xnew[v] equal to Xold[v] bit for bit, or no simplex references v: unew = uold
//   bary      e_j = Xold[v_{j+1}] - Xold[v0], d = p - Xold[v0]; lambda_{1..D} by the adjugate
//             divided by det (the form of field_math.h), lambda_0 = 1 - sum; m = min lambda
//   contains  m >= -kTransferTol
//   patch     the simplices incident to v in ascending id (the x-update's incidence list): the
//             first that contains p; else the one with the largest m (the first wins ties)
//   walk      from that simplex through the face opposite the smallest lambda (the first smallest)
//             to the face neighbour, until a simplex contains p (walked), the face has no neighbour
//             or kTransferMaxWalk moves are made (outside: the best simplex seen, extrapolated)
//   value     u0 + sum_j lambda_j (u_j - u0), left to right
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#ifndef MMX_FHD
#if defined(__HIPCC__)
#define MMX_FHD __host__ __device__ __forceinline__
#else
#define MMX_FHD inline
#endif
#endif

namespace mmx {

constexpr double kTransferTol = 1e-12;
constexpr int kTransferMaxWalk = 64;
// incident simplices whose rows are requested before any is tested (as kFieldChunk; 2 and 8 were
// both slower on the 3D cube and the 2D disc)
constexpr int kTransferChunk = 4;
// counts[] of a transfer
enum { kTransferCopied = 0, kTransferPatch = 1, kTransferWalked = 2, kTransferOutside = 3 };

// every component of p equal to q's bit for bit (-0.0 and 0.0 differ, a NaN equals itself)
template <int D>
MMX_FHD bool transfer_unmoved(const double* p, const double* q) {
  bool same = true;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    unsigned long long a, b;
    __builtin_memcpy(&a, &p[k], 8);
    __builtin_memcpy(&b, &q[k], 8);
    same = same && a == b;
  }
  return same;
}

// the D + 1 vertex ids of simplex s; a 3D row is one 16-byte load on the device
template <int D>
MMX_FHD void transfer_load_ids(const int* F, int s, int* f) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (D == 3) {
    const int4 q = reinterpret_cast<const int4*>(F)[s];
    f[0] = q.x;
    f[1] = q.y;
    f[2] = q.z;
    f[D] = q.w;
    return;
  }
#endif
#pragma unroll
  for (int n = 0; n < D + 1; ++n) f[n] = F[(size_t)s * (D + 1) + n];
}

// the position of node v; a 2D row is one 16-byte load on the device (X 16-byte aligned)
template <int D>
MMX_FHD void transfer_load_point(const double* X, int v, double* x) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (D == 2) {
    const double2 q = reinterpret_cast<const double2*>(X)[v];
    x[0] = q.x;
    x[1] = q.y;
    return;
  }
#endif
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = X[(size_t)v * D + k];
}

// barycentric coordinates lam[0 .. D] of p in the simplex with vertex positions xv; returns their
// minimum, taken left to right
template <int D>
MMX_FHD double transfer_bary(const double (*xv)[D], const double* p, double* lam) {
  double e[D][D], d[D];
#pragma unroll
  for (int j = 0; j < D; ++j)
#pragma unroll
    for (int k = 0; k < D; ++k) e[j][k] = xv[j + 1][k] - xv[0][k];
#pragma unroll
  for (int k = 0; k < D; ++k) d[k] = p[k] - xv[0][k];
  if constexpr (D == 2) {
    const double det = e[0][0] * e[1][1] - e[0][1] * e[1][0];
    lam[1] = (e[1][1] * d[0] - e[1][0] * d[1]) / det;
    lam[2] = (e[0][0] * d[1] - e[0][1] * d[0]) / det;
    lam[0] = 1.0 - (lam[1] + lam[2]);
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
#pragma unroll
    for (int j = 0; j < 3; ++j) lam[j + 1] = ((d[0] * cr[j][0] + d[1] * cr[j][1]) + d[2] * cr[j][2]) / det;
    lam[0] = 1.0 - ((lam[1] + lam[2]) + lam[3]);
  }
  double m = lam[0];
#pragma unroll
  for (int j = 1; j < D + 1; ++j) m = lam[j] < m ? lam[j] : m;
  return m;
}

MMX_FHD bool transfer_contains(double m) { return m >= -kTransferTol; }

// the vertex positions of a simplex from its ids
template <int D>
MMX_FHD void transfer_load_simplex(const double* X, const int* f, double (*xv)[D]) {
#pragma unroll
  for (int n = 0; n < D + 1; ++n) transfer_load_point<D>(X, f[n], xv[n]);
}

// the patch search of one node: off[0 .. cnt) its incident slot offsets s K + n D in ascending
// simplex id, cnt >= 1.  True: *sOut contains p; false: *sOut is the simplex with the largest m.
// lam: the coordinates in *sOut.  (The rows of kTransferChunk simplices are requested before any
// is tested; they are tested one by one in list order, as a plain loop would.)
template <int D>
MMX_FHD bool transfer_patch(const double* Xold, const int* F, const int* off, int cnt, const double* p, int* sOut,
                            double* lam) {
  constexpr int K = D * (D + 1);
  int bs = -1;
  double bm = 0.0, bl[D + 1];
  int t = 0;
  for (; t + kTransferChunk <= cnt; t += kTransferChunk) {
    int s[kTransferChunk], f[kTransferChunk][D + 1];
    double xv[kTransferChunk][D + 1][D];
#pragma unroll
    for (int j = 0; j < kTransferChunk; ++j) s[j] = off[t + j] / K;
#pragma unroll
    for (int j = 0; j < kTransferChunk; ++j) transfer_load_ids<D>(F, s[j], f[j]);
#pragma unroll
    for (int j = 0; j < kTransferChunk; ++j) transfer_load_simplex<D>(Xold, f[j], xv[j]);
#pragma unroll
    for (int j = 0; j < kTransferChunk; ++j) {
      double l[D + 1];
      const double m = transfer_bary<D>(xv[j], p, l);
      if (transfer_contains(m)) {
        *sOut = s[j];
#pragma unroll
        for (int i = 0; i < D + 1; ++i) lam[i] = l[i];
        return true;
      }
      if (bs < 0 || m > bm) {
        bs = s[j];
        bm = m;
#pragma unroll
        for (int i = 0; i < D + 1; ++i) bl[i] = l[i];
      }
    }
  }
  for (; t < cnt; ++t) {
    const int s = off[t] / K;
    int f[D + 1];
    double xv[D + 1][D], l[D + 1];
    transfer_load_ids<D>(F, s, f);
    transfer_load_simplex<D>(Xold, f, xv);
    const double m = transfer_bary<D>(xv, p, l);
    if (transfer_contains(m)) {
      *sOut = s;
#pragma unroll
      for (int i = 0; i < D + 1; ++i) lam[i] = l[i];
      return true;
    }
    if (bs < 0 || m > bm) {
      bs = s;
      bm = m;
#pragma unroll
      for (int i = 0; i < D + 1; ++i) bl[i] = l[i];
    }
  }
  *sOut = bs;
#pragma unroll
  for (int i = 0; i < D + 1; ++i) lam[i] = bl[i];
  return false;
}

// the walk from *s (the patch search's best simplex, which does not contain p) over the
// face-neighbour table nbr.  True: *s contains p; false: *s is the best simplex seen.  lam: the
// coordinates in *s.
template <int D>
MMX_FHD bool transfer_walk(const double* Xold, const int* F, const int* nbr, const double* p, int* s, double* lam) {
  int cur = *s, f[D + 1];
  double xv[D + 1][D], lc[D + 1];
  transfer_load_ids<D>(F, cur, f);
  transfer_load_simplex<D>(Xold, f, xv);
  double bm = transfer_bary<D>(xv, p, lc);
  int bs = cur;
  double bl[D + 1];
#pragma unroll
  for (int i = 0; i < D + 1; ++i) bl[i] = lc[i];
  for (int moves = 0; moves < kTransferMaxWalk; ++moves) {
    int jm = 0;
    double lm = lc[0];
#pragma unroll
    for (int j = 1; j < D + 1; ++j)
      if (lc[j] < lm) {
        lm = lc[j];
        jm = j;
      }
    const int nb = nbr[(size_t)cur * (D + 1) + jm];
    if (nb < 0) break;
    cur = nb;
    transfer_load_ids<D>(F, cur, f);
    transfer_load_simplex<D>(Xold, f, xv);
    const double m = transfer_bary<D>(xv, p, lc);
    if (m > bm) {
      bm = m;
      bs = cur;
#pragma unroll
      for (int i = 0; i < D + 1; ++i) bl[i] = lc[i];
    }
    if (transfer_contains(m)) {
      *s = cur;
#pragma unroll
      for (int i = 0; i < D + 1; ++i) lam[i] = lc[i];
      return true;
    }
  }
  *s = bs;
#pragma unroll
  for (int i = 0; i < D + 1; ++i) lam[i] = bl[i];
  return false;
}

// the C components of the field at the point with coordinates lam in simplex s
template <int D>
MMX_FHD void transfer_value(const int* F, int s, const double* lam, int C, const double* uold, double* out) {
  int f[D + 1];
  transfer_load_ids<D>(F, s, f);
  for (int c = 0; c < C; ++c) {
    const double u0 = uold[(size_t)f[0] * C + c];
    double r = u0;
#pragma unroll
    for (int j = 1; j < D + 1; ++j) r = r + lam[j] * (uold[(size_t)f[j] * C + c] - u0);
    out[c] = r;
  }
}

}  // namespace mmx
