// slide_math.h -- the arithmetic of the sliding boundary, one text for the device
// kernel (slide_kernels.hip) and the host-only mmadmm_boundary_project_field (csrc/host/slide.cpp).
// Only + - * / and comparisons, every operation order fixed and every product rounded before it is
// added (-ffp-contract=off), so a restatement on IEEE doubles (tests/slide_py.py) reproduces both
// bit for bit.
//
//   surface   the boundary faces of the mesh at the positions X0 it was frozen at: D vertex ids a
//             face (a segment in 2D, a triangle in 3D), never the nodes' current positions
//   star(a)   the faces incident to the surface vertex a, in ascending face id (a CSR over node ids)
//   closest   the closest point c of a face to p, and the face's vertex that carries the largest
//             barycentric weight of c (the first wins ties).  A vertex region returns that vertex's
//             bits; an edge region A + t AB; the triangle's interior A + AB v + AC w (Ericson,
//             Real-Time Collision Detection §5.1.5).  A coordinate all the face's vertices share is
//             returned exactly: the differences in it are 0
//   project   from the node's anchor a: the face of star(a) with the smallest d2 = |p - c|^2 (sums left
//             to right, the first wins ties); it replaces the best so far when it is smaller; then
//             hop to that face's heaviest vertex, unless it is a itself or BOUNDARY_FIXED, at most
//             kSlideMaxHops times.  A NaN never compares smaller, so a position with a NaN (or a
//             star of degenerate faces) finds no face: the node and its anchor stay as they are
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

constexpr int kSlideMaxHops = 8;
constexpr int kSlideFixed = 1;  // NodeType BOUNDARY_FIXED (MMADMM_BOUNDARY_FIXED)
constexpr int kSlideFree = 0;   // NodeType BOUNDARY_FREE (MMADMM_BOUNDARY_FREE)
// counts[] of a projection; the first four partition the sliding nodes, at_pin is counted beside them
enum { kSlideUnmoved = 0, kSlideStar = 1, kSlideHopped = 2, kSlideExhausted = 3, kSlideAtPin = 4, kSlideCounts = 5 };

MMX_FHD unsigned long long slide_bits(double x) {
  unsigned long long b;
  __builtin_memcpy(&b, &x, 8);
  return b;
}

template <int D>
MMX_FHD bool slide_same_bits(const double* p, const double* q) {
  bool same = true;
#pragma unroll
  for (int k = 0; k < D; ++k) same = same && slide_bits(p[k]) == slide_bits(q[k]);
  return same;
}

template <int D>
MMX_FHD double slide_dot(const double* a, const double* b) {
  double s = a[0] * b[0];
#pragma unroll
  for (int k = 1; k < D; ++k) s = s + a[k] * b[k];
  return s;
}

// closest point of the segment xv[0] xv[1] to p -> c; returns the heavier vertex (0 or 1)
MMX_FHD int slide_closest(const double (*xv)[2], const double* p, double* c) {
  const double* A = xv[0];
  const double* B = xv[1];
  double ab[2], ap[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    ab[k] = B[k] - A[k];
    ap[k] = p[k] - A[k];
  }
  const double t = slide_dot<2>(ap, ab) / slide_dot<2>(ab, ab);
  if (t <= 0.0) {
    c[0] = A[0];
    c[1] = A[1];
    return 0;
  }
  if (t >= 1.0) {
    c[0] = B[0];
    c[1] = B[1];
    return 1;
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) c[k] = A[k] + t * ab[k];
  return t > 0.5 ? 1 : 0;
}

// closest point of the triangle xv[0] xv[1] xv[2] to p -> c; returns the heaviest vertex (0, 1 or 2)
MMX_FHD int slide_closest(const double (*xv)[3], const double* p, double* c) {
  const double* A = xv[0];
  const double* B = xv[1];
  const double* C = xv[2];
  double ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ab[k] = B[k] - A[k];
    ac[k] = C[k] - A[k];
    ap[k] = p[k] - A[k];
    bp[k] = p[k] - B[k];
    cp[k] = p[k] - C[k];
  }
  double v, w;  // c = A + AB v + AC w, weights (1 - v - w, v, w)
  const double d1 = slide_dot<3>(ab, ap), d2 = slide_dot<3>(ac, ap);
  const double d3 = slide_dot<3>(ab, bp), d4 = slide_dot<3>(ac, bp);
  const double d5 = slide_dot<3>(ab, cp), d6 = slide_dot<3>(ac, cp);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  if (d1 <= 0.0 && d2 <= 0.0) {  // vertex region A
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = A[k];
    return 0;
  }
  if (d3 >= 0.0 && d4 <= d3) {  // vertex region B
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = B[k];
    return 1;
  }
  if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {  // edge AB
    v = d1 / (d1 - d3);
    w = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = A[k] + v * ab[k];
  } else if (d6 >= 0.0 && d5 <= d6) {  // vertex region C
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = C[k];
    return 2;
  } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {  // edge AC
    v = 0.0;
    w = d2 / (d2 - d6);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = A[k] + w * ac[k];
  } else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {  // edge BC
    w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    v = 1.0 - w;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = B[k] + w * (C[k] - B[k]);
  } else {  // the interior
    const double sum = (va + vb) + vc;
    v = vb / sum;
    w = vc / sum;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (A[k] + ab[k] * v) + ac[k] * w;
  }
  double best = (1.0 - v) - w;
  int big = 0;
  if (v > best) {
    best = v;
    big = 1;
  }
  if (w > best) big = 2;
  return big;
}

// what a projection leaves besides the point
struct SlideResult {
  double d2;     // the squared distance p moved by (0 when no face was found)
  int face;      // the face the point lies on, -1: none found
  int hops;
  int exhausted;  // the hop limit ended the search
};

// p projected onto the frozen surface (X0: nP x D; faces: D vertex ids each; starPtr / starFace: the
// CSR of faces at every node id; mask: NodeType per node) from the anchor *anchor, which is advanced.
// out may not alias p.
template <int D>
MMX_FHD SlideResult slide_project(const double* X0, const int* faces, const int* starPtr, const int* starFace,
                                  const int* mask, const double* p, int* anchor, double* out) {
  int a = *anchor;
  SlideResult r;
  r.d2 = 0.0;
  r.face = -1;
  r.hops = 0;
  r.exhausted = 0;
  double best = __builtin_inf();
#pragma unroll
  for (int k = 0; k < D; ++k) out[k] = p[k];
  for (;;) {
    double sbest = __builtin_inf(), sc[D];
    int sface = -1, sbig = 0;
    const int e = starPtr[a + 1];
    for (int t = starPtr[a]; t < e; ++t) {
      const int f = starFace[t];
      double xv[D][D], c[D];
#pragma unroll
      for (int n = 0; n < D; ++n) {
        const int vtx = faces[(size_t)f * D + n];
#pragma unroll
        for (int k = 0; k < D; ++k) xv[n][k] = X0[(size_t)vtx * D + k];
      }
      const int big = slide_closest(xv, p, c);
      double df = p[0] - c[0];
      double d2 = df * df;
#pragma unroll
      for (int k = 1; k < D; ++k) {
        df = p[k] - c[k];
        d2 = d2 + df * df;
      }
      if (d2 < sbest) {
        sbest = d2;
        sface = f;
        sbig = big;
#pragma unroll
        for (int k = 0; k < D; ++k) sc[k] = c[k];
      }
    }
    if (sface < 0) break;
    if (sbest < best) {
      best = sbest;
      r.d2 = sbest;
      r.face = sface;
#pragma unroll
      for (int k = 0; k < D; ++k) out[k] = sc[k];
    }
    const int a2 = faces[(size_t)sface * D + sbig];
    if (a2 == a) break;
    if (mask[a2] == kSlideFixed) break;
    if (r.hops == kSlideMaxHops) {
      r.exhausted = 1;
      break;
    }
    a = a2;
    r.hops++;
  }
  *anchor = a;
  return r;
}

// the outcome of a projection: one of kSlideUnmoved .. kSlideExhausted, and *atPin = the result has
// the bits of a BOUNDARY_FIXED vertex of its face
template <int D>
MMX_FHD int slide_classify(const double* X0, const int* faces, const int* mask, const double* p, const double* out,
                           const SlideResult& r, int* atPin) {
  *atPin = 0;
  if (r.face >= 0) {
#pragma unroll
    for (int n = 0; n < D; ++n) {
      const int vtx = faces[(size_t)r.face * D + n];
      if (mask[vtx] == kSlideFixed && slide_same_bits<D>(out, X0 + (size_t)vtx * D)) *atPin = 1;
    }
  }
  if (r.exhausted) return kSlideExhausted;
  if (slide_same_bits<D>(p, out)) return kSlideUnmoved;
  return r.hops == 0 ? kSlideStar : kSlideHopped;
}

}  // namespace mmx
