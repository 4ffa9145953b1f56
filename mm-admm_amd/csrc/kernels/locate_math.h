// locate_math.h -- the arithmetic of the point locator and of the field sampled at arbitrary points
// (DESIGN.md §7j), one text for the device kernels (locate_kernels.hip) and the host-only
// mmadmm_sample_field (csrc/host/locate.cpp).  The barycentric coordinates, the containment test and
// the interpolation are transfer_math.h's, unchanged; what is added is integer cell arithmetic and
// comparisons, so a restatement on IEEE doubles (tests/sample_py.py) reproduces both bit for bit
// (-ffp-contract=off).
//
//   box       lo_k / hi_k = min / max of X[:, k] over all nodes (exact, order-independent)
//   cells     n_k per axis (n_2 = 1 in 2D), given or automatic: n_k = g, g the largest integer with
//             g^D <= max(1, nF / kLocateFill[D]) and g^D <= 2^27 (locate_default_cells)
//   cell      inv_k = (double)n_k / (hi_k - lo_k); cell_k(x) = clamp((int)((x - lo_k) inv_k), 0,
//             n_k - 1), truncating; id = (c_2 n_1 + c_1) n_0 + c_0.  (The clamp is taken on the double
//             before the conversion, so a product beyond the int range clamps too.)
//   lists     simplex s is listed in every cell of cell_k(min_j X[v_j][k] - pad_k) ..
//             cell_k(max_j X[v_j][k] + pad_k), pad_k = kLocatePad (hi_k - lo_k): a point that
//             transfer_contains accepts through its 1e-12 tolerance lies, per axis, within
//             (D + 1) 1e-12 simplex extents of the simplex's extent, and the rounding of the cell
//             products moves a cell boundary by about 2^-52 of the box: both far inside the pad of
//             1e-9 of the box
//   query     a component of p not finite, or the clamped cell of p empty: none.  Else over the SET
//             of listed simplices: the lowest id among those that contain p (inside); if none does,
//             the largest m, the lowest id on ties (outside, extrapolated).  A NaN m (a simplex of zero
//             volume) ranks as -inf, so the order of the list never matters
#pragma once

#include <stddef.h>

#include "transfer_math.h"

namespace mmx {

// simplices per cell the automatic grid aims at, by dimension ([2], [3]): measured on one MI355X, the
// values with the lowest build + 1M-uniform-query time among {1, 2, 4, 8} and {1, 3, 6, 12}
// (3D: 3 and 6 are within 2% of each other, 3 holds 1.4x the memory)
constexpr int kLocateFill[4] = {0, 0, 2, 3};
constexpr double kLocatePad = 1e-9;
constexpr long long kLocateMaxCells = 1LL << 27;
// counts[] of a sample
enum { kSampleInside = 0, kSampleOutside = 1, kSampleNone = 2 };
// the value of a point that is not located: the quiet NaN 0x7ff8000000000000
constexpr unsigned long long kSampleNanBits = 0x7ff8000000000000ull;

struct LocateGrid {
  double lo[3], hi[3];
  double inv[3];  // cells per unit length
  double pad[3];  // kLocatePad (hi - lo)
  int n[3];       // cells per axis (n[2] = 1 in 2D)
};

// the automatic cells of nF simplices in `dim` dimensions; integers only
inline void locate_default_cells(int dim, int nF, int* cells) {
  long long target = (long long)nF / kLocateFill[dim];
  if (target < 1) target = 1;
  if (target > kLocateMaxCells) target = kLocateMaxCells;
  long long g = 1;
  for (;;) {
    const long long h = g + 1;
    const long long p = dim == 2 ? h * h : h * h * h;
    if (p > target) break;
    g = h;
  }
  cells[0] = cells[1] = (int)g;
  cells[2] = dim == 3 ? (int)g : 1;
}

// inv and pad from lo, hi and n
inline void locate_finish_grid(int dim, LocateGrid& g) {
  for (int k = 0; k < 3; ++k) {
    if (k >= dim) {
      g.lo[k] = g.hi[k] = g.inv[k] = g.pad[k] = 0.0;
      g.n[k] = 1;
      continue;
    }
    const double w = g.hi[k] - g.lo[k];
    g.inv[k] = (double)g.n[k] / w;
    g.pad[k] = kLocatePad * w;
  }
}

MMX_FHD bool locate_finite(double x) {
  unsigned long long b;
  __builtin_memcpy(&b, &x, 8);
  return ((b >> 52) & 0x7ffull) != 0x7ffull;
}

MMX_FHD int locate_cell_axis(const LocateGrid& g, int k, double x) {
  const double t = (x - g.lo[k]) * g.inv[k];
  if (!(t >= 0.0)) return 0;
  if (t >= (double)g.n[k]) return g.n[k] - 1;
  return (int)t;
}

// the cell id of the point p (finite components)
template <int D>
MMX_FHD int locate_cell(const LocateGrid& g, const double* p) {
  int id = 0;
#pragma unroll
  for (int k = D - 1; k >= 0; --k) id = id * g.n[k] + locate_cell_axis(g, k, p[k]);
  return id;
}

// the inclusive index box clo .. chi of the simplex with vertex positions xv
template <int D>
MMX_FHD void locate_simplex_box(const LocateGrid& g, const double (*xv)[D], int* clo, int* chi) {
#pragma unroll
  for (int k = 0; k < D; ++k) {
    double a = xv[0][k], b = a;
#pragma unroll
    for (int j = 1; j < D + 1; ++j) {
      const double c = xv[j][k];
      a = c < a ? c : a;
      b = c > b ? c : b;
    }
    clo[k] = locate_cell_axis(g, k, a - g.pad[k]);
    chi[k] = locate_cell_axis(g, k, b + g.pad[k]);
  }
#pragma unroll
  for (int k = D; k < 3; ++k) clo[k] = chi[k] = 0;
}

// one candidate offered to the state of a query: the simplex taken so far (qs, whether it contains p,
// its m with a NaN ranked -inf, its coordinates in lam).  A containing candidate replaces a
// non-containing one, or a containing one of higher id; a non-containing candidate replaces only a
// non-containing one of smaller m, or of equal m and higher id: a total order, so the order of the
// offers does not matter
template <int D>
MMX_FHD void locate_offer(int& qs, bool& qin, double& qm, double* lam, int s, double m, const double* l) {
  const bool in = transfer_contains(m);
  const double mc = m == m ? m : -__builtin_inf();
  const bool take = in ? (!qin || s < qs) : (!qin && (qs < 0 || mc > qm || (mc == qm && s < qs)));
  if (take) {
    qs = s;
    qin = in;
    qm = mc;
#pragma unroll
    for (int i = 0; i < D + 1; ++i) lam[i] = l[i];
  }
}

// the query of the point p: kSampleInside / kSampleOutside with *sOut and lam set, or kSampleNone.
// starts: ncell + 1 list offsets; pairs: the lists; X, F: the locator's positions and simplices.
// (The rows of kTransferChunk candidates are requested before any is tested.)
template <int D>
MMX_FHD int locate_query(const LocateGrid& g, const int* starts, const int* pairs, const double* X, const int* F,
                         const double* p, int* sOut, double* lam) {
#pragma unroll
  for (int k = 0; k < D; ++k)
    if (!locate_finite(p[k])) return kSampleNone;
  const int cell = locate_cell<D>(g, p);
  const int b = starts[cell], e = starts[cell + 1];
  if (e == b) return kSampleNone;
  int qs = -1;
  bool qin = false;
  double qm = 0.0;
  int t = b;
  for (; t + kTransferChunk <= e; t += kTransferChunk) {
    int s[kTransferChunk], f[kTransferChunk][D + 1];
    double xv[kTransferChunk][D + 1][D];
#pragma unroll
    for (int j = 0; j < kTransferChunk; ++j) s[j] = pairs[t + j];
#pragma unroll
    for (int j = 0; j < kTransferChunk; ++j) transfer_load_ids<D>(F, s[j], f[j]);
#pragma unroll
    for (int j = 0; j < kTransferChunk; ++j) transfer_load_simplex<D>(X, f[j], xv[j]);
#pragma unroll
    for (int j = 0; j < kTransferChunk; ++j) {
      double l[D + 1];
      const double m = transfer_bary<D>(xv[j], p, l);
      locate_offer<D>(qs, qin, qm, lam, s[j], m, l);
    }
  }
  for (; t < e; ++t) {
    const int s = pairs[t];
    int f[D + 1];
    double xv[D + 1][D], l[D + 1];
    transfer_load_ids<D>(F, s, f);
    transfer_load_simplex<D>(X, f, xv);
    const double m = transfer_bary<D>(xv, p, l);
    locate_offer<D>(qs, qin, qm, lam, s, m, l);
  }
  *sOut = qs;
  return qin ? kSampleInside : kSampleOutside;
}

// one query end to end: out[0 .. C) and the `where` code (-1 none, s inside, -2 - s outside)
template <int D>
MMX_FHD int locate_sample_point(const LocateGrid& g, const int* starts, const int* pairs, const double* X,
                                const int* F, const double* p, int C, const double* u, double* out, int* where) {
  int s = 0;
  double lam[D + 1];
  const int cat = locate_query<D>(g, starts, pairs, X, F, p, &s, lam);
  if (cat == kSampleNone) {
    double nan;
    const unsigned long long bits = kSampleNanBits;
    __builtin_memcpy(&nan, &bits, 8);
    for (int c = 0; c < C; ++c) out[c] = nan;
    *where = -1;
    return cat;
  }
  transfer_value<D>(F, s, lam, C, u, out);
  *where = cat == kSampleInside ? s : -2 - s;
  return cat;
}

}  // namespace mmx
