// admm_kernels_euler.hip -- backward Euler (Mesh::backwardsEulerStep, src/Mesh.cpp:1263-1341): the
// finite-difference Jacobian blocks, their assembly and the Newton residual.
#include "admm_common.h"

namespace mmx {
// FSubJac's derivative blocks (src/Mesh.cpp:1173-1230), simplex-centric: thread (s, n) evaluates
// blockGrad at the vertices Vp (pass -1, the reference's Gk) and with coordinate i of vertex n
// moved by h (pass i), and writes derivs(i, :) = (Gkp1 - Gk) / h.  A BOUNDARY_FIXED vertex gets
// the reference's identity pattern, which is nonzero only for n == 0 (r == c in D*n..D*n+D-1).
// The node-centric reference evaluates Gk once per (node, simplex); the values are the same.
// EXACT = false (with `work`): the fast path -- a lane whose powers meet a rounding midpoint (or
// leave the double-double ranges) writes nothing and queues itself (work[0] counts, work[1 + q]
// lists), and k_fd_jac_fix recomputes the queued lanes with the exact decision.  On the regular
// initial meshes the exact path is common, and in the one-kernel form every wave with one such
// lane ran it, with its expansion arithmetic in 5 KB of scratch per lane (C4: 110 ms)
template <int D, int ISO, bool EXACT>
__device__ __forceinline__ void fd_jac_lane(const DeviceMesh<D>& m, const double* __restrict__ Vp, double h,
                                            double* __restrict__ dv, long long t, unsigned* work) {
  constexpr int K = D * (D + 1);
  const int s = (int)(t / (D + 1)), n = (int)(t % (D + 1));
  double* out = dv + (size_t)t * D * K;
  if (m.sbits[s] & (1u << n)) {
    for (int r = 0; r < D; ++r)
#pragma unroll
      for (int c = 0; c < K; ++c) out[r * K + c] = (c == r && c >= D * n && c < D * (n + 1)) ? 1.0 : 0.0;
    return;
  }
  int f[D + 1];
  loadVerts<D>(m, s, f);
  double xl[K], xi[K], gk[K], g1[K], xp[K], Igt;
  gatherX<D>(Vp, f, xl);
  loadXi<D>(m, f, xi);
  const GridView<D> g = gridOf<D, ISO>(m);
  const FunctionalConsts<D> fc = constsOf<D>(m);
  bool tie = false;
#pragma unroll 1
  for (int it = -1; it < D; ++it) {
    const int moved = (it < 0) ? -1 : D * n + it;
#pragma unroll
    for (int c = 0; c < K; ++c) xp[c] = (c == moved) ? xl[c] + h : xl[c];
    blockGrad<D, true, false, EXACT>(g, fc, xp, xi, nullptr, g1, Igt, nullptr, &tie);
    if (it < 0) {
#pragma unroll
      for (int c = 0; c < K; ++c) gk[c] = g1[c];
    } else {  // (a queued lane's rows are all written again by k_fd_jac_fix)
#pragma unroll
      for (int c = 0; c < K; ++c) out[it * K + c] = (g1[c] - gk[c]) / h;
    }
  }
  if constexpr (!EXACT) {
    if (tie) work[1 + atomicAdd(work, 1u)] = (unsigned)t;
  }
}
template <int D, int ISO = -1, bool EXACT = true>
__global__ void __launch_bounds__(kBlock) k_fd_jac(DeviceMesh<D> m, const double* __restrict__ Vp, double h,
                                                    double* __restrict__ dv, unsigned* work) {
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (t >= (long long)m.nF * (D + 1)) return;
  fd_jac_lane<D, ISO, EXACT>(m, Vp, h, dv, t, work);
}
// the lanes k_fd_jac<.., false> queued, exactly (a fixed grid striding over the queue)
template <int D, int ISO = -1>
__global__ void __launch_bounds__(kBlock) k_fd_jac_fix(DeviceMesh<D> m, const double* __restrict__ Vp, double h,
                                                        double* __restrict__ dv, const unsigned* __restrict__ work) {
  const unsigned nq = work[0];
  for (unsigned q = blockIdx.x * kBlock + threadIdx.x; q < nq; q += gridDim.x * kBlock)
    fd_jac_lane<D, ISO, true>(m, Vp, h, dv, (long long)work[1 + q], nullptr);
}

// buildEulerJac + FSubJac's scatter (src/Mesh.cpp:1112-1136, 1232-1258), row-centric: row
// r = D*pnt + p, entry (col node ci, offset co).  The reference adds, for each incident simplex
// in ascending id and each vertex j in pairsort order, derivs(p, D*rel[j]+co) where the sorted id
// equals ci and +0.0 elsewhere; the +0.0 adds only turn a -0.0 sum into +0.0, so the same value
// is v + 0.0 before the matching vertex (if it is not first), + d, + 0.0 after (if not last).
template <int D>
__global__ void __launch_bounds__(kBlock) k_jac_assemble(DeviceMesh<D> m, const int* __restrict__ ia,
                                                          const int* __restrict__ ja, const double* __restrict__ dv,
                                                          double dt_over_tau, int finish, double* __restrict__ a) {
  constexpr int K = D * (D + 1);
  const int r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= m.nP * D) return;
  const int pnt = r / D, p = r % D;
  const int tb = m.inc_ptr[pnt], te = m.inc_ptr[pnt + 1];
  for (int i = ia[r]; i < ia[r + 1]; ++i) {
    const int col = ja[i], ci = col / D, co = col % D;
    double v = 0.0;
    for (int t = tb; t < te; ++t) {
      const int off = m.inc_off[t];
      const int s = off / K, nl = (off % K) / D;
      int f[D + 1];
      loadVerts<D>(m, s, f);
      int hit = -1, rank = 0;
#pragma unroll
      for (int k = 0; k < D + 1; ++k) {
        if (f[k] == ci) hit = k;
        rank += (f[k] < ci) ? 1 : 0;
      }
      if (hit >= 0) {
        if (rank > 0) v = v + 0.0;
        v = v + dv[((size_t)(s * (D + 1) + nl) * D + p) * K + D * hit + co];
        if (rank < D) v = v + 0.0;
      } else {
        v = v + 0.0;
      }
    }
    if (finish) {  // buildEulerJac's scaling and identity (src/Mesh.cpp:1125-1134); else the FSubJac sums
      v *= dt_over_tau;
      if (col == r) v += 1.0;
    }
    a[i] = v;
  }
}

// The same sums simplex-outer: row r walks its node's incident simplices once (ascending id) and
// adds each simplex's derivative block to the entries of its D + 1 vertices, found by a binary
// search over the row's node-major columns.  Every entry receives its terms in the same order as
// above; the +0.0 adds are dropped because they change nothing here -- an entry starts at +0.0, and
// a sum that starts at +0.0 is never -0.0 under round-to-nearest (+0 + -0 = +0, x + -x = +0), so
// v + 0.0 = v at every step (bit-identical; C4: 26 ms for the entry-outer form, which loaded the
// node's incident simplices again for every entry of the row)
template <int D>
__global__ void __launch_bounds__(kBlock) k_jac_assemble_s(DeviceMesh<D> m, const int* __restrict__ ia,
                                                            const int* __restrict__ ja, const double* __restrict__ dv,
                                                            double dt_over_tau, int finish, double* __restrict__ a) {
  constexpr int K = D * (D + 1);
  const int r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= m.nP * D) return;
  const int pnt = r / D, p = r % D;
  const int rb = ia[r], re = ia[r + 1], nn = (re - rb) / D;
  for (int i = rb; i < re; ++i) a[i] = 0.0;
  const int tb = m.inc_ptr[pnt], te = m.inc_ptr[pnt + 1];
  for (int t = tb; t < te; ++t) {
    const int off = m.inc_off[t];
    const int s = off / K, nl = (off % K) / D;
    int f[D + 1];
    loadVerts<D>(m, s, f);
    const double* d = dv + ((size_t)(s * (D + 1) + nl) * D + p) * K;
#pragma unroll
    for (int k = 0; k < D + 1; ++k) {
      int lo = 0, hi = nn - 1;  // the node f[k] among the row's nodes (ascending; it is there)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ja[rb + mid * D] / D < f[k])
          lo = mid + 1;
        else
          hi = mid;
      }
      double* e = a + rb + lo * D;
#pragma unroll
      for (int co = 0; co < D; ++co) e[co] = e[co] + d[D * k + co];
    }
  }
  if (finish) {
    for (int i = rb; i < re; ++i) {
      double v = a[i] * dt_over_tau;
      if (ja[i] == r) v += 1.0;
      a[i] = v;
    }
  }
}

// The same sums with one wavefront per node: lane q holds the D x D entries (rows p, offsets co)
// of the node's q-th column node (the node's D rows share their node-major columns) and the wave
// walks the node's incident simplices once, in ascending id (uniform loads); the lanes of the
// simplex's vertices add its derivative values -- every entry its terms in the same order
// (bit-identical; at most 64 column nodes, checked by the launch).  A node that no simplex
// references (the Shoulder meshes have such nodes) has rows holding only their diagonal entry
// (mmx_struc_mesh_pattern), not node blocks: its entries are +0.0 (and the identity) as in the
// other forms.
template <int D>
__global__ void __launch_bounds__(256) k_jac_assemble_w(DeviceMesh<D> m, const int* __restrict__ ia,
                                                         const int* __restrict__ ja, const double* __restrict__ dv,
                                                         double dt_over_tau, int finish, double* __restrict__ a) {
  constexpr int K = D * (D + 1);
  const int pnt = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
  if (pnt >= m.nP) return;
  const int tb = m.inc_ptr[pnt], te = m.inc_ptr[pnt + 1];
  if (tb == te) {
#pragma unroll
    for (int p = 0; p < D; ++p) {
      const int r = pnt * D + p;
      for (int i = ia[r] + lane; i < ia[r + 1]; i += 64) {
        double v = 0.0;
        if (finish) {
          v *= dt_over_tau;
          if (ja[i] == r) v += 1.0;
        }
        a[i] = v;
      }
    }
    return;
  }
  const int r0 = pnt * D, rb = ia[r0], nn = (ia[r0 + 1] - rb) / D;
  const bool act = lane < nn;
  const int ci = act ? ja[rb + lane * D] / D : -1;
  double acc[D][D];
#pragma unroll
  for (int p = 0; p < D; ++p)
#pragma unroll
    for (int co = 0; co < D; ++co) acc[p][co] = 0.0;
  for (int t = tb; t < te; ++t) {
    const int off = m.inc_off[t];
    const int s = off / K, nl = (off % K) / D;
    int f[D + 1];
    loadVerts<D>(m, s, f);
    int hit = -1;
#pragma unroll
    for (int k = 0; k < D + 1; ++k)
      if (f[k] == ci) hit = k;
    if (hit >= 0) {
      const double* d = dv + ((size_t)(s * (D + 1) + nl) * D) * K + D * hit;
#pragma unroll
      for (int p = 0; p < D; ++p)
#pragma unroll
        for (int co = 0; co < D; ++co) acc[p][co] = acc[p][co] + d[p * K + co];
    }
  }
  if (!act) return;
#pragma unroll
  for (int p = 0; p < D; ++p) {
    const int r = r0 + p, i0 = ia[r] + lane * D;
#pragma unroll
    for (int co = 0; co < D; ++co) {
      double v = acc[p][co];
      if (finish) {  // buildEulerJac's scaling and identity (src/Mesh.cpp:1125-1134)
        v *= dt_over_tau;
        if (ja[i0 + co] == r) v += 1.0;
      }
      a[i0 + co] = v;
    }
  }
}

// Newton residual of backwardsEulerStep (src/Mesh.cpp:1301-1306): grad from eulerStepMod's
// INTERIOR-only scatter (ascending simplex id), F = grad * (dt/tau) + (x - xn), rhs = -F.
// ORD: the nodes in the x-update's processing order (their gathers from neighbouring simplices; C4
// 0.58 ms in node-id order) and no partials -- k_abs_partials then forms them from rhs in node-id
// order with this kernel's blocks, the same sums in the same order (bit-identical)
template <int D, bool ORD = false>
__global__ void __launch_bounds__(kBlock) k_be_residual(DeviceMesh<D> m, const double* __restrict__ gs,
                                                         const double* __restrict__ x, const double* __restrict__ xn,
                                                         double dt_over_tau, double* __restrict__ rhs,
                                                         double* __restrict__ partials, int xcd) {
  const int lb = logical_block(xcd);
  const int idx = lb * kBlock + threadIdx.x;
  const int v = (ORD && idx < m.nP) ? m.nodeOrder[idx] : idx;
  double pv[1] = {0.0};
  if (v < m.nP) {
    double g[D];
#pragma unroll
    for (int c = 0; c < D; ++c) g[c] = 0.0;
    if (m.nodeInterior[v]) {
      const int b = m.inc_ptr[v], e = m.inc_ptr[v + 1];
      for (int t = b; t < e; ++t) {
        const double* src = gs + m.inc_off[t];
#pragma unroll
        for (int c = 0; c < D; ++c) g[c] += src[c];
      }
    }
#pragma unroll
    for (int c = 0; c < D; ++c) {
      const double F = g[c] * dt_over_tau + (x[(size_t)v * D + c] - xn[(size_t)v * D + c]);
      pv[0] += __builtin_fabs(F);
      rhs[(size_t)v * D + c] = -F;
    }
  }
  if constexpr (!ORD) block_partials<1>(pv, partials, lb);
}
// the partials of k_be_residual<D, false> from rhs = -F (|-F| = |F| exactly)
template <int D>
__global__ void __launch_bounds__(kBlock) k_abs_partials(int nP, const double* __restrict__ rhs,
                                                          double* __restrict__ partials, int xcd) {
  const int lb = logical_block(xcd);
  const int v = lb * kBlock + threadIdx.x;
  double pv[1] = {0.0};
  if (v < nP) {
#pragma unroll
    for (int c = 0; c < D; ++c) pv[0] += __builtin_fabs(rhs[(size_t)v * D + c]);
  }
  block_partials<1>(pv, partials, lb);
}

__global__ void __launch_bounds__(kBlock) k_add_inplace(int n, double* __restrict__ x, const double* __restrict__ dx) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) x[i] += dx[i];
}

template <int D>
void launch_fd_jac(const DeviceMesh<D>& m, const double* Vp, double h, double* dv, hipStream_t st, unsigned* work) {
  const long long nt = (long long)m.nF * (D + 1);
  if (nt == 0) return;
  // the fix pass: one lane per possible queue entry (the queue's length is known on the device only;
  // lanes past it exit at once) -- the exact path is long, so every queued lane gets its own
  const dim3 gj((unsigned)((nt + kBlock - 1) / kBlock)), gf = gj;
  if (work && hipMemsetAsync(work, 0, sizeof(unsigned), st) != hipSuccess)
    throw std::runtime_error("launch_fd_jac: memset");
  dispatch_iso<D>(m, [&](auto iso) {
    constexpr int ISO = decltype(iso)::value;
    if (work) {  // fast pass + the exact recomputation of its queued lanes
      hipLaunchKernelGGL((k_fd_jac<D, ISO, false>), gj, dim3(kBlock), 0, st, m, Vp, h, dv, work);
      hipLaunchKernelGGL((k_fd_jac_fix<D, ISO>), gf, dim3(kBlock), 0, st, m, Vp, h, dv, (const unsigned*)work);
    } else {
      hipLaunchKernelGGL((k_fd_jac<D, ISO>), gj, dim3(kBlock), 0, st, m, Vp, h, dv, nullptr);
    }
  });
}
template <int D>
void launch_jac_assemble(const DeviceMesh<D>& m, const EngineKnobs& k, const int* ia, const int* ja, const double* dv,
                         double dt_over_tau, double* a, hipStream_t st, bool finish, int maxColNodes) {
  if (m.nP == 0) return;
  if (k.jacAssembleEntry)  // the entry-outer form
    hipLaunchKernelGGL(k_jac_assemble<D>, dim3(nblk(m.nP * D)), dim3(kBlock), 0, st, m, ia, ja, dv, dt_over_tau,
                       finish ? 1 : 0, a);
  else if (maxColNodes <= 64)
    hipLaunchKernelGGL(k_jac_assemble_w<D>, dim3((m.nP + 3) / 4), dim3(256), 0, st, m, ia, ja, dv, dt_over_tau,
                       finish ? 1 : 0, a);
  else
    hipLaunchKernelGGL(k_jac_assemble_s<D>, dim3(nblk(m.nP * D)), dim3(kBlock), 0, st, m, ia, ja, dv, dt_over_tau,
                       finish ? 1 : 0, a);
}
template <int D>
void launch_be_residual(const DeviceMesh<D>& m, const EngineKnobs& k, const double* gs, const double* x,
                        const double* xn, double dt_over_tau, double* rhs, double* partials, int* nblocks,
                        hipStream_t st) {
  *nblocks = nblk_xcd(m.nP, k.xcdMap);
  if (m.nP == 0) return;
  if (m.nodeOrder) {  // the node-ordered residual, then its partials in node-id order
    hipLaunchKernelGGL((k_be_residual<D, true>), dim3(*nblocks), dim3(kBlock), 0, st, m, gs, x, xn, dt_over_tau, rhs,
                       partials, k.xcdMap);
    hipLaunchKernelGGL(k_abs_partials<D>, dim3(*nblocks), dim3(kBlock), 0, st, m.nP, rhs, partials, k.xcdMap);
    return;
  }
  hipLaunchKernelGGL(k_be_residual<D>, dim3(*nblocks), dim3(kBlock), 0, st, m, gs, x, xn, dt_over_tau, rhs, partials,
                     k.xcdMap);
}
void launch_add_inplace(int n, double* x, const double* dx, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_add_inplace, dim3(nblk(n)), dim3(kBlock), 0, st, n, x, dx);
}
#define MMX_INST(D)                                                                                                 \
  template void launch_fd_jac<D>(const DeviceMesh<D>&, const double*, double, double*, hipStream_t, unsigned*);     \
  template void launch_jac_assemble<D>(const DeviceMesh<D>&, const EngineKnobs&, const int*, const int*,            \
                                       const double*, double, double*, hipStream_t, bool, int);                     \
  template void launch_be_residual<D>(const DeviceMesh<D>&, const EngineKnobs&, const double*, const double*,       \
                                      const double*, double, double*, double*, int*, hipStream_t);
MMX_INST(2)
MMX_INST(3)
}  // namespace mmx
extern "C" unsigned mmx_layout_admm_euler(void) { return mmx::kLayoutWord; }  // layout.h: this object's word
