// admm_kernels_step.hip -- the ADMM time step around the prox: z = D x, the simplex gradient, predictX,
// the x-update (x = (tau xBar + dt^2 sum_{s ∋ v} w (w (z - u))) / t_vv in ascending simplex order, Eigen's
// column-major D^T product order), the energy, the Euler scatter, the halo pack, the reductions.
#include "admm_common.h"

namespace mmx {
// z = D x (Dmat * x, src/MeshIntegrator.cpp:121,126): exact gather into simplex copies
template <int D>
__global__ void __launch_bounds__(kBlock) k_gather_z(DeviceMesh<D> m, const double* __restrict__ x,
                                                      double* __restrict__ z) {
  constexpr int K = D * (D + 1);
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= m.nF) return;
  int f[D + 1];
  loadVerts<D>(m, s, f);
  double v[K];
  gatherX<D>(x, f, v);
#pragma unroll
  for (int i = 0; i < K; ++i) z[zu_base<D>(s) + zu_i<D>(i)] = v[i];
}

// per-simplex gradient of the unregularised functional (Mesh::eulerGrad / eulerStepMod)
template <int D, int ISO = -1>
__global__ void __launch_bounds__(kBlock) k_grad_simplex(DeviceMesh<D> m, const double* __restrict__ x,
                                                          double* __restrict__ gs, int zeroFixedRows,
                                                          double* __restrict__ partials) {
  constexpr int K = D * (D + 1);
  const int s = blockIdx.x * kBlock + threadIdx.x;
  double pv[5] = {0, 0, 0, 0, 0};
  if (s < m.nF) {
    int f[D + 1];
    loadVerts<D>(m, s, f);
    double z[K], xi[K], g[K], Igt;
    gatherX<D>(x, f, z);
    loadXi<D>(m, f, xi);
    const double e = blockGrad<D, true, false>(gridOf<D, ISO>(m), constsOf<D>(m), z, xi, nullptr, g, Igt);
    if (zeroFixedRows) zeroFixed<D>(g, m.sbits[s] & 0xF);
#pragma unroll
    for (int i = 0; i < K; ++i) gs[(size_t)s * K + i] = g[i];
    pv[0] = e;
    pv[4] = (e == e) ? 0.0 : 1.0;
  }
  block_partials<5>(pv, partials);
}

// predictX (src/Mesh.cpp:649-674) fused with xPrev = x (src/MeshIntegrator.cpp:119):
// mode 0: xBar = x - (dt/tau) * sum_{s ∋ v} gs (ascending s);  mode 1: xBar = 2x - xPrev
template <int D>
__global__ void __launch_bounds__(kBlock) k_predict(DeviceMesh<D> m, int mode, const double* __restrict__ gs,
                                                     const double* __restrict__ x, double* __restrict__ xPrev,
                                                     double* __restrict__ xBar, double dt_over_tau, int xcd) {
  const int idx = logical_block(xcd) * kBlock + threadIdx.x;
  if (idx >= m.nP) return;
  // mode 0 gathers the incident gradients: in the x-update's order (neighbouring simplices); mode 1
  // streams x and xPrev in node-id order
  const int v = (mode == 0 && m.nodeOrder) ? m.nodeOrder[idx] : idx;
  double xv[D], xb[D];
#pragma unroll
  for (int c = 0; c < D; ++c) xv[c] = x[(size_t)v * D + c];
  if (mode == 0) {
    double g[D];
#pragma unroll
    for (int c = 0; c < D; ++c) g[c] = 0.0;
    const int b = m.inc_ptr[v], e = m.inc_ptr[v + 1];
    for (int t = b; t < e; ++t) {
      const int off = m.inc_off[t];
      const double* src = (off >= 0) ? gs + off : m.remote + (size_t)(-1 - off) * D;
#pragma unroll
      for (int c = 0; c < D; ++c) g[c] += src[c];
    }
#pragma unroll
    for (int c = 0; c < D; ++c) xb[c] = xv[c] - dt_over_tau * g[c];
  } else {
#pragma unroll
    for (int c = 0; c < D; ++c) xb[c] = 2 * xv[c] - xPrev[(size_t)v * D + c];
  }
#pragma unroll
  for (int c = 0; c < D; ++c) {
    xBar[(size_t)v * D + c] = xb[c];
    xPrev[(size_t)v * D + c] = xv[c];
  }
}

// x-update: vec = tau*xBar + dt^2 WD_T (w (z - u)), x = vec / t_vv (block-diagonal t),
// optional |D x - z|^2 partial sums (primal residual, src/MeshIntegrator.cpp:162).
// A node's incident slots are taken CH at a time: their offsets, then all their z and u values
// are requested before the first is added (branch-free: lanes past the end re-read the last
// slot, a slot of another rank reads its gathered row), then summed in ascending order.
//
// XupHead: what a lane knows of its node before the first gather -- the node, its slot range,
// invdiag and the first CH slot offsets.  From the records (DeviceMesh::xrec, host/xup_records.h)
// every address follows from the position, so the head is one load phase and the gathers the
// second; from the CSR (MMX_XUP_REC=0) it is three dependent phases.
template <int CH>
struct XupHead {
  int v, b, e;
  double inv;
  int off[CH];
};
template <int D, int CH>
__device__ __forceinline__ void xup_head_rec(const DeviceMesh<D>& m, int idx, XupHead<CH>& h) {
  const int* r = m.xrec + (size_t)idx * kXupRecInts;
  h.v = r[0];
  h.b = r[1];
  h.e = r[2];
  h.inv = m.xinv[idx];
#pragma unroll
  for (int j = 0; j < CH; ++j) h.off[j] = m.xslot[(size_t)j * m.xslotStride + idx];
}
template <int D, int CH>
__device__ __forceinline__ void xup_head_csr(const DeviceMesh<D>& m, int idx, XupHead<CH>& h) {
  // processing order: nodes by first incident simplex, so a workgroup's nodes share simplices
  h.v = m.nodeOrder ? m.nodeOrder[idx] : idx;
  h.b = m.inc_ptr[h.v];
  h.e = m.inc_ptr[h.v + 1];
  h.inv = m.invdiag[h.v];
#pragma unroll
  for (int j = 0; j < CH; ++j) h.off[j] = (h.e > h.b) ? m.inc_off[min(h.b + j, h.e - 1)] : 0;
}
template <int D, bool RESID, bool TS, int CH = 8, bool ZX = false, bool PRED = false, bool REM = false>
__device__ __forceinline__ void xupdate_node(const DeviceMesh<D>& m, const StepScalars& sc,
                                             const double* __restrict__ xBar, const double* __restrict__ z,
                                             const double* __restrict__ u, double* __restrict__ x,
                                             const XupHead<CH>& h, double (&pv)[3]) {
  {
    const int v = h.v, b = h.b, e = h.e;
    double acc[D];
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] = 0.0;
    double xb[D], zn[D];
    if constexpr (PRED) {  // predictX mode 1 for this node (k_predict): xBar = 2 x - xPrev, xPrev = x
      double xv[D];
#pragma unroll
      for (int c = 0; c < D; ++c) {
        xv[c] = x[(size_t)v * D + c];
        xb[c] = 2 * xv[c] - m.predPrev[(size_t)v * D + c];
      }
#pragma unroll
      for (int c = 0; c < D; ++c) {
        m.predBar[(size_t)v * D + c] = xb[c];
        m.predPrev[(size_t)v * D + c] = xv[c];
      }
    } else {
#pragma unroll
      for (int c = 0; c < D; ++c) xb[c] = xBar[(size_t)v * D + c];
    }
    // ZX: a step's first x-update without z (DeviceMesh::zx): every local slot of node v holds z = zx_v
    // (with PRED, zx is this step's xBar: the node's own xb); REM: an element partition, whose
    // remote slots still come from the exchange (their terms formed by launch_pack_export)
    constexpr bool zv0 = ZX && !TS;
    if constexpr (zv0) {
      if constexpr (PRED) {
#pragma unroll
        for (int c = 0; c < D; ++c) zn[c] = xb[c];
      } else {
#pragma unroll
        for (int c = 0; c < D; ++c) zn[c] = m.zx[(size_t)v * D + c];
      }
    }
    const double inv = h.inv;
    // one chunk: the slots t0 .. t0 + CH - 1 at the offsets off
    auto addChunk = [&](int t0, const int(&off)[CH]) {
      double zv[CH][D], uv[CH][D];
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const bool loc = off[j] >= 0;
        if constexpr (TS) {  // the prox's terms; another rank's slot from `remote`
          const double* pt = loc ? m.tslot + off[j] : m.remote + (size_t)(-1 - off[j]) * D;
#pragma unroll
          for (int c = 0; c < D; ++c) zv[j][c] = pt[c];
        } else {
          const double* pz = loc ? z + zu_off<D>(off[j]) : m.remote + (size_t)(-1 - off[j]) * D;
          const double* pu = loc ? u + zu_off<D>(off[j]) : pz;
#pragma unroll
          for (int c = 0; c < D; ++c) {
            if constexpr (zv0 && REM)
              zv[j][c] = loc ? zn[c] : pz[c];
            else if constexpr (zv0)  // (one rank only: no slot of another rank)
              zv[j][c] = zn[c];
            else
              zv[j][c] = pz[c];
            uv[j][c] = pu[c];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        if (t0 + j < e) {
#pragma unroll
          for (int c = 0; c < D; ++c) {  // another rank's slot: the term formed there (launch_pack_export mode 0)
            if constexpr (TS)
              acc[c] += zv[j][c];
            else
              acc[c] += (off[j] >= 0) ? sc.w * (sc.w * (zv[j][c] - uv[j][c])) : zv[j][c];
          }
        }
      }
    };
    // the first chunk's offsets came with the head; the rest (a node of more than CH slots) from the CSR
    if (b < e) addChunk(b, h.off);
    for (int t0 = b + CH; t0 < e; t0 += CH) {
      int off[CH];
#pragma unroll
      for (int j = 0; j < CH; ++j) off[j] = m.inc_off[min(t0 + j, e - 1)];
      addChunk(t0, off);
    }
    double xn[D];
#pragma unroll
    for (int c = 0; c < D; ++c) {
      xn[c] = ((sc.tau * xb[c]) + sc.dtsq * acc[c]) * inv;
      x[(size_t)v * D + c] = xn[c];
    }
    if constexpr (RESID) {  // same chunking; a slot of another rank is counted by its owner
      double r2 = 0.0;
      auto residChunk = [&](int t0, const int(&off)[CH]) {
        double zv[CH][D];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const double* pz = z + zu_off<D>(off[j] >= 0 ? off[j] : 0);
#pragma unroll
          for (int c = 0; c < D; ++c) zv[j][c] = pz[c];
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          if (t0 + j < e && off[j] >= 0) {
#pragma unroll
            for (int c = 0; c < D; ++c) {
              const double d = xn[c] - zv[j][c];
              r2 += d * d;
            }
          }
        }
      };
      if (b < e) residChunk(b, h.off);  // (the offsets it already holds)
      for (int t0 = b + CH; t0 < e; t0 += CH) {
        int off[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) off[j] = m.inc_off[min(t0 + j, e - 1)];
        residChunk(t0, off);
      }
      pv[2] = r2;
    }
  }
}
template <int D, int CH, bool REC>
__device__ __forceinline__ void xup_head(const DeviceMesh<D>& m, int idx, XupHead<CH>& h) {
  if constexpr (REC)
    xup_head_rec<D, CH>(m, idx, h);
  else
    xup_head_csr<D, CH>(m, idx, h);
}
template <int D, bool RESID, bool TS, bool ZX = false, bool PRED = false, bool REM = false, bool REC = false>
__global__ void __launch_bounds__(kBlock) k_xupdate(DeviceMesh<D> m, StepScalars sc,
                                                     const double* __restrict__ xBar,
                                                     const double* __restrict__ z,
                                                     const double* __restrict__ u, double* __restrict__ x,
                                                     double* __restrict__ partials, int xcd) {
  constexpr int CH = (D == 2 ? MMX_XU_CH2D : 8);
  const int lb = logical_block(xcd);
  const int idx = m.xupLo + lb * kBlock + threadIdx.x;
  double pv[3] = {0, 0, 0};
  if (idx < m.xupHi) {
    XupHead<CH> h;
    xup_head<D, CH, REC>(m, idx, h);
    xupdate_node<D, RESID, TS, CH, ZX, PRED, REM>(m, sc, xBar, z, u, x, h, pv);
  }
  if constexpr (RESID) block_partials<3>(pv, partials, lb);
}
// The slot-term x-update (no residual) as a sweep: XCD c (= blockIdx % 8) takes the node-order
// positions [c n8, (c + 1) n8) and its gridDim / 8 workgroups walk them in rounds, so the slot
// terms a round gathers are mostly still in that XCD's L2 for the neighbouring rounds.
// CH: incident slots requested at once per node (3D slot terms: 24 covers a grid vertex's
// tetrahedra in one batch)
// RESID: the primal residual too (a step's last iteration, or every iteration with the early exit):
// each lane sums its nodes' terms in its round order and the workgroup's partial record is
// blockIdx.x -- a fixed grouping for a fixed grid, so runs are bit-reproducible
// EARLY (on the records): a lane requests the head of its next position before it waits for the
// current node's gathers -- loads return in order, so the head has arrived when the gathers have,
// and one exposed load phase per node is left
template <int D, bool TS, int CH, bool RESID = false, bool REC = false, bool EARLY = false>
__global__ void __launch_bounds__(kBlock) k_xupdate_sweep(DeviceMesh<D> m, StepScalars sc,
                                                           const double* __restrict__ xBar,
                                                           const double* __restrict__ z, const double* __restrict__ u,
                                                           double* __restrict__ x, int n8, double* __restrict__ partials) {
  static_assert(REC || !EARLY, "the early request reads the records");
  const int c = (int)(blockIdx.x % 8), w = (int)(blockIdx.x / 8), per = (int)(gridDim.x / 8);
  const int lo = m.xupLo + c * n8, hi = min(lo + n8, m.xupHi);
  double pv[3], r2 = 0.0;
  int idx = lo + w * kBlock + (int)threadIdx.x;
  if constexpr (EARLY) {
    XupHead<CH> cur, nxt;
    if (idx < hi) xup_head<D, CH, true>(m, idx, cur);
    nxt = cur;
    for (; idx < hi; idx += per * kBlock) {
      if (idx + per * kBlock < hi) xup_head<D, CH, true>(m, idx + per * kBlock, nxt);
      __builtin_amdgcn_sched_barrier(0);  // (the next head's loads stay ahead of this node's gathers)
      xupdate_node<D, RESID, TS, CH>(m, sc, xBar, z, u, x, cur, pv);
      if constexpr (RESID) r2 += pv[2];
      cur = nxt;
    }
  } else {
    for (; idx < hi; idx += per * kBlock) {
      XupHead<CH> h;
      xup_head<D, CH, REC>(m, idx, h);
      xupdate_node<D, RESID, TS, CH>(m, sc, xBar, z, u, x, h, pv);
      if constexpr (RESID) r2 += pv[2];
    }
  }
  if constexpr (RESID) {
    double q[3] = {0.0, 0.0, r2};
    block_partials<3>(q, partials, (int)blockIdx.x);
  }
}

// Mesh::computeEnergy (src/Mesh.cpp:496-530) on positions x
template <int D, int ISO = -1>
__global__ void __launch_bounds__(kBlock) k_energy(DeviceMesh<D> m, const double* __restrict__ x,
                                                    double* __restrict__ partials) {
  constexpr int K = D * (D + 1);
  const int s = blockIdx.x * kBlock + threadIdx.x;
  double pv[5] = {0, 0, 0, 0, 0};
  if (s < m.nF) {
    int f[D + 1];
    loadVerts<D>(m, s, f);
    double z[K], xi[K], Igt;
    gatherX<D>(x, f, z);
    loadXi<D>(m, f, xi);
    const double e = blockGrad<D, false, false>(gridOf<D, ISO>(m), constsOf<D>(m), z, xi, nullptr, nullptr, Igt);
    pv[0] = e;
    pv[4] = (e == e) ? 0.0 : 1.0;
  }
  block_partials<5>(pv, partials);
}

// Mesh::eulerStepMod scatter (src/Mesh.cpp:566-572): INTERIOR nodes only; x -= (dt/tau) grad
template <int D>
__global__ void __launch_bounds__(kBlock) k_euler_apply(DeviceMesh<D> m, const double* __restrict__ gs,
                                                         double* __restrict__ x, double dt_over_tau, int xcd) {
  const int idx = logical_block(xcd) * kBlock + threadIdx.x;
  if (idx >= m.nP) return;
  // nodes in the x-update's processing order (first incident simplex; 3D: y slabs): a workgroup's
  // nodes gather from neighbouring simplices (C4: 0.58 ms in node-id order)
  const int v = m.nodeOrder ? m.nodeOrder[idx] : idx;
  double g[D];
#pragma unroll
  for (int c = 0; c < D; ++c) g[c] = 0.0;
  if (m.nodeInterior[v]) {
    const int b = m.inc_ptr[v], e = m.inc_ptr[v + 1];
    for (int t = b; t < e; ++t) {
      const int off = m.inc_off[t];
      const double* src = (off >= 0) ? gs + off : m.remote + (size_t)(-1 - off) * D;
#pragma unroll
      for (int c = 0; c < D; ++c) g[c] += src[c];
    }
  }
#pragma unroll
  for (int c = 0; c < D; ++c) x[(size_t)v * D + c] -= dt_over_tau * g[c];
}

template <int D>
__global__ void __launch_bounds__(kBlock) k_pack_export(int mode, int nExp, const int* __restrict__ expOff,
                                                         const double* __restrict__ z, const double* __restrict__ u,
                                                         const double* __restrict__ gs, double w,
                                                         double* __restrict__ out, PackZX zx) {
  constexpr int K = D * (D + 1);
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= nExp) return;
  const size_t off = (size_t)expOff[e], zo = zu_off<D>(expOff[e]);
  double zv[D];
  if (mode == 0 && zx.zx) {  // z of the slot = zx of its node (DeviceMesh::zx); predicted: 2 x - xPrev
    const int s = expOff[e] / K, n = (expOff[e] % K) / D;
    const size_t v = (size_t)zx.F[(size_t)s * (D + 1) + n];
#pragma unroll
    for (int c = 0; c < D; ++c) zv[c] = zx.x ? 2 * zx.x[v * D + c] - zx.xPrev[v * D + c] : zx.zx[v * D + c];
  } else {
#pragma unroll
    for (int c = 0; c < D; ++c) zv[c] = z[zo + c];
  }
#pragma unroll
  for (int c = 0; c < D; ++c)
    out[(size_t)e * D + c] = (mode == 0) ? w * (w * (zv[c] - u[zo + c])) : gs[off + c];
}

constexpr int kRed = 1024;
__device__ void reduce_set(const double* __restrict__ partials, int nblocks, double* __restrict__ out);

__global__ void __launch_bounds__(kRed) k_reduce_partials(const double* __restrict__ partials, int nblocks,
                                                           double* __restrict__ out, const double* __restrict__ partials2,
                                                           int nblocks2, double* __restrict__ out2) {
  if (blockIdx.x == 1)  // second set in the same launch
    reduce_set(partials2, nblocks2, out2);
  else
    reduce_set(partials, nblocks, out);
}

// a whole step's reductions in one launch (early exit off): workgroup i < n reduces the prox
// partials of iteration i (slices of `stride` doubles), workgroup n the last x-update's
__global__ void __launch_bounds__(kRed) k_reduce_steps(const double* __restrict__ partA, size_t stride, int nbA,
                                                        const double* __restrict__ partB, int nbB, int n,
                                                        double* __restrict__ results) {
  const int i = blockIdx.x;
  if (i < n)
    reduce_set(partA + (size_t)i * stride, nbA, results + (size_t)i * 2 * kNumPartials);
  else
    reduce_set(partB, nbB, results + (size_t)(n - 1) * 2 * kNumPartials + kNumPartials);
}

// The split form, two launches (a kernel boundary orders them: no fences or counters, which on the
// eight-XCD chip cost a device-wide L2 write-back each -- the one-launch form with an arrival counter
// measured 93 us against 45 us for one workgroup per set): k_reduce_split's workgroup (set q, range
// r) reduces range r of set q into the scratch, k_reduce_combine sums the kRedSplit range results of
// each set in range order.  Sets: q < nA are slices of partA (stride apart), q = nA the set partB
// (when nbB >= 0).
constexpr int kRedLanes = 256;
__global__ void __launch_bounds__(kRedLanes) k_reduce_split(const double* __restrict__ partA, size_t stride, int nbA,
                                                            int nA, const double* __restrict__ partB, int nbB,
                                                            double* __restrict__ scratch) {
  __shared__ double red[kRedLanes / 64][kNumPartials];
  const int q = (int)blockIdx.x / kRedSplit, r = (int)blockIdx.x % kRedSplit;
  const bool isA = q < nA;
  const double* p = isA ? partA + (size_t)q * stride : partB;
  const int nb = isA ? nbA : nbB;
  const int per = (nb + kRedSplit - 1) / kRedSplit, lo = min(nb, r * per), hi = min(nb, lo + per);
  const int tid = (int)threadIdx.x;
  double acc[kNumPartials];
#pragma unroll
  for (int i = 0; i < kNumPartials; ++i) acc[i] = 0.0;
  for (int b = lo + tid; b < hi; b += kRedLanes)
#pragma unroll
    for (int i = 0; i < kNumPartials; ++i) {
      const double v = p[(size_t)b * kNumPartials + i];
      acc[i] = (i == 5) ? fmax(acc[i], v) : acc[i] + v;
    }
#pragma unroll
  for (int i = 0; i < kNumPartials; ++i) acc[i] = (i == 5) ? wave_max(acc[i]) : wave_sum(acc[i]);
  if ((tid & 63) == 0)
#pragma unroll
    for (int i = 0; i < kNumPartials; ++i) red[tid >> 6][i] = acc[i];
  __syncthreads();
  if (tid < kNumPartials) {
    double v = red[0][tid];
    for (int w = 1; w < kRedLanes / 64; ++w) v = (tid == 5) ? fmax(v, red[w][tid]) : v + red[w][tid];
    scratch[(size_t)blockIdx.x * kNumPartials + tid] = v;
  }
}
__global__ void __launch_bounds__(64) k_reduce_combine(const double* __restrict__ scratch, int nA,
                                                       double* __restrict__ outA, size_t outStride,
                                                       double* __restrict__ outB) {
  const int q = (int)blockIdx.x, t = (int)threadIdx.x;
  if (t >= kNumPartials) return;
  const double* base = scratch + (size_t)q * kRedSplit * kNumPartials + t;
  double acc = base[0];
  for (int k = 1; k < kRedSplit; ++k) acc = (t == 5) ? fmax(acc, base[(size_t)k * kNumPartials]) : acc + base[(size_t)k * kNumPartials];
  (q < nA ? outA + (size_t)q * outStride : outB)[t] = acc;
}

__device__ void reduce_set(const double* __restrict__ partials, int nblocks, double* __restrict__ out) {
  // one workgroup of 1024: lane-strided sums in a fixed order (four rows requested at a time),
  // then the wavefront butterflies and the 16 wavefront results in order -- a fixed shape
  __shared__ double red[kRed / 64][kNumPartials];
  const int tid = threadIdx.x;
  double acc[kNumPartials];
#pragma unroll
  for (int i = 0; i < kNumPartials; ++i) acc[i] = 0.0;  // entry 5 (a max of counts >= 0) too
  int b = tid;
  for (; b + 3 * kRed < nblocks; b += 4 * kRed) {
    double v[4][kNumPartials];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < kNumPartials; ++i) v[q][i] = partials[(size_t)(b + q * kRed) * kNumPartials + i];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < kNumPartials; ++i) acc[i] = (i == 5) ? fmax(acc[i], v[q][i]) : acc[i] + v[q][i];
  }
  for (; b < nblocks; b += kRed)
#pragma unroll
    for (int i = 0; i < kNumPartials; ++i) {
      const double v = partials[(size_t)b * kNumPartials + i];
      acc[i] = (i == 5) ? fmax(acc[i], v) : acc[i] + v;
    }
#pragma unroll
  for (int i = 0; i < kNumPartials; ++i) acc[i] = (i == 5) ? wave_max(acc[i]) : wave_sum(acc[i]);
  if ((tid & 63) == 0)
#pragma unroll
    for (int i = 0; i < kNumPartials; ++i) red[tid >> 6][i] = acc[i];
  __syncthreads();
  if (tid < kNumPartials) {
    double r = red[0][tid];
    for (int w = 1; w < kRed / 64; ++w) r = (tid == 5) ? fmax(r, red[w][tid]) : r + red[w][tid];
    out[tid] = r;
  }
}

template <int D>
void launch_gather_z(const DeviceMesh<D>& m, const double* x, double* z, hipStream_t st) {
  if (m.nF == 0) return;
  hipLaunchKernelGGL(k_gather_z<D>, dim3(nblk(m.nF)), dim3(kBlock), 0, st, m, x, z);
}
template <int D>
void launch_grad_simplex(const DeviceMesh<D>& m, const double* x, double* gs, bool zeroFixedRows,
                         double* partials, int* nblocks, hipStream_t st) {
  *nblocks = nblk(m.nF);
  if (m.nF == 0) return;
  dispatch_iso<D>(m, [&](auto iso) {
    hipLaunchKernelGGL((k_grad_simplex<D, decltype(iso)::value>), dim3(*nblocks), dim3(kBlock), 0, st, m, x, gs,
                       zeroFixedRows ? 1 : 0, partials);
  });
}
template <int D>
void launch_predict(const DeviceMesh<D>& m, const EngineKnobs& k, int mode, const double* gs, double* x,
                    double* xPrev, double* xBar, double dt_over_tau, hipStream_t st) {
  if (m.nP == 0) return;
  hipLaunchKernelGGL(k_predict<D>, dim3(nblk_xcd(m.nP, k.xcdMap)), dim3(kBlock), 0, st, m, mode, gs, x, xPrev, xBar,
                     dt_over_tau, k.xcdMap);
}
template <int D>
void launch_xupdate(const DeviceMesh<D>& m, const EngineKnobs& k, const StepScalars& sc, const double* xBar,
                    const double* z, const double* u, double* x, double* partials, int* nblocks, bool resid,
                    hipStream_t st, bool useTslot) {
  const int nsub = m.xupHi - m.xupLo;  // the launch's share of the node order
  *nblocks = nblk_xcd(nsub, k.xcdMap);
  if (nsub <= 0) {
    *nblocks = 0;
    return;
  }
  const bool ts = useTslot && m.tslot;
  const bool rem = m.remote != nullptr;
  const bool rec = m.xrec != nullptr;  // the node records (MMX_XUP_REC=0: the CSR)
  auto needCols = [&](int ch) {  // a kernel's first chunk is the table's first ch columns
    if (rec && m.xslotCh < ch) throw std::logic_error("launch_xupdate: the slot table has fewer columns than the chunk");
  };
  if (m.zx && !resid && !ts) {  // a step's first x-update: z from DeviceMesh::zx
    needCols(D == 2 ? MMX_XU_CH2D : 8);
    dispatch_bool(m.predBar != nullptr, [&](auto pred) {  // ... and predictX's extrapolation fused in
      dispatch_bool(rem, [&](auto r) {
        dispatch_bool(rec, [&](auto rc) {
          hipLaunchKernelGGL(
              (k_xupdate<D, false, false, true, decltype(pred)::value, decltype(r)::value, decltype(rc)::value>),
              dim3(*nblocks), dim3(kBlock), 0, st, m, sc, xBar, z, u, x, partials, k.xcdMap);
        });
      });
    });
    return;
  }
  // the fused extrapolation exists only in the form above: a caller that set it for another form
  // would lose predictX silently
  if (m.predBar || m.predPrev)
    throw std::logic_error("launch_xupdate: predBar set for an x-update that cannot fuse predictX");
  // the sweep (persistent) form, MMX_XUP_SWEEP workgroups per CU; with the residual in the slot-term
  // form (3D): C4's last x-update of a step 0.334 -> ~0.17 ms (MMX_XUP_SWEEP_RESID=0: one node per lane)
  const bool sweepResid = resid && ts && k.xupSweepResid;
  if (m.xupSweep > 0 && (!resid || sweepResid)) {
    const int n8 = ((nsub + kBlock - 1) / kBlock + 7) / 8 * kBlock;  // = the node order's XCD groups
    const dim3 g(256 * m.xupSweep);
    // on the records, with or without the next node's early request (DeviceMesh::xupEarly); else the CSR
    auto sweep = [&](auto tsT, auto chT, auto residT, double* part) {
      constexpr bool TS = decltype(tsT)::value, RS = decltype(residT)::value;
      constexpr int CH = decltype(chT)::value;
      needCols(CH);
      if (rec && m.xupEarly)
        hipLaunchKernelGGL((k_xupdate_sweep<D, TS, CH, RS, true, true>), g, dim3(kBlock), 0, st, m, sc, xBar, z, u, x, n8,
                           part);
      else if (rec)
        hipLaunchKernelGGL((k_xupdate_sweep<D, TS, CH, RS, true, false>), g, dim3(kBlock), 0, st, m, sc, xBar, z, u, x, n8,
                           part);
      else
        hipLaunchKernelGGL((k_xupdate_sweep<D, TS, CH, RS>), g, dim3(kBlock), 0, st, m, sc, xBar, z, u, x, n8, part);
    };
    using T = std::true_type;
    using F = std::false_type;
    if (sweepResid) {
      *nblocks = (int)g.x;
      sweep(T{}, std::integral_constant<int, 8>{}, T{}, partials);
    } else if (ts && m.xupCh >= 24)
      sweep(T{}, std::integral_constant<int, 24>{}, F{}, nullptr);
    else if (ts && m.xupCh >= 16)
      sweep(T{}, std::integral_constant<int, 16>{}, F{}, nullptr);
    else if (ts)
      sweep(T{}, std::integral_constant<int, 8>{}, F{}, nullptr);
    else
      sweep(F{}, std::integral_constant<int, (D == 2 ? MMX_XU_CH2D : 8)>{}, F{}, nullptr);
    return;
  }
  needCols(D == 2 ? MMX_XU_CH2D : 8);
  dispatch_bool(resid, [&](auto r) {
    dispatch_bool(ts, [&](auto t) {
      dispatch_bool(rec, [&](auto rc) {
        hipLaunchKernelGGL((k_xupdate<D, decltype(r)::value, decltype(t)::value, false, false, false, decltype(rc)::value>),
                           dim3(*nblocks), dim3(kBlock), 0, st, m, sc, xBar, z, u, x, partials, k.xcdMap);
      });
    });
  });
}
template <int D>
void launch_energy(const DeviceMesh<D>& m, const double* x, double* partials, int* nblocks, hipStream_t st) {
  *nblocks = nblk(m.nF);
  if (m.nF == 0) return;
  dispatch_iso<D>(m, [&](auto iso) {
    hipLaunchKernelGGL((k_energy<D, decltype(iso)::value>), dim3(*nblocks), dim3(kBlock), 0, st, m, x, partials);
  });
}
template <int D>
void launch_euler_apply(const DeviceMesh<D>& m, const EngineKnobs& k, const double* gs, double* x, double dt_over_tau,
                        hipStream_t st) {
  if (m.nP == 0) return;
  hipLaunchKernelGGL(k_euler_apply<D>, dim3(nblk_xcd(m.nP, k.xcdMap)), dim3(kBlock), 0, st, m, gs, x, dt_over_tau,
                     k.xcdMap);
}
// one workgroup per set reads its partials at ~0.1 TB/s (C3: 10 sets of 31 k prox partials took 45 us
// per step); the split form spreads each set over kRedSplit workgroups
static bool split_ok(const RedWork& w, int nblocks) { return w.scratch && nblocks >= w.splitMin; }
static void reduce_split(const double* partA, size_t stride, int nbA, int nA, double* outA, size_t outStride,
                         const double* partB, int nbB, double* outB, const RedWork& w, hipStream_t st) {
  const int sets = nA + (nbB >= 0 ? 1 : 0);
  hipLaunchKernelGGL(k_reduce_split, dim3(sets * kRedSplit), dim3(kRedLanes), 0, st, partA, stride, nbA, nA, partB,
                     nbB, w.scratch);
  hipLaunchKernelGGL(k_reduce_combine, dim3(sets), dim3(64), 0, st, w.scratch, nA, outA, outStride, outB);
}
void launch_reduce_partials(const double* partials, int nblocks, double* out, hipStream_t st, const RedWork& w) {
  if (split_ok(w, nblocks))
    reduce_split(partials, 0, nblocks, 1, out, 0, partials, -1, out, w, st);
  else
    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(kRed), 0, st, partials, nblocks, out, partials, nblocks, out);
}
void launch_reduce_steps(const double* partA, size_t stride, int nbA, const double* partB, int nbB, int n,
                         double* results, hipStream_t st, const RedWork& w) {
  if (split_ok(w, nbA) && n + 1 <= kRedSets)
    reduce_split(partA, stride, nbA, n, results, (size_t)2 * kNumPartials, partB, nbB,
                 results + (size_t)(n - 1) * 2 * kNumPartials + kNumPartials, w, st);
  else
    hipLaunchKernelGGL(k_reduce_steps, dim3(n + 1), dim3(kRed), 0, st, partA, stride, nbA, partB, nbB, n, results);
}
void launch_reduce_partials2(const double* partials, int nblocks, double* out, const double* partials2, int nblocks2,
                             double* out2, hipStream_t st, const RedWork& w) {
  if (split_ok(w, nblocks))
    reduce_split(partials, 0, nblocks, 1, out, 0, partials2, nblocks2, out2, w, st);
  else
    hipLaunchKernelGGL(k_reduce_partials, dim3(2), dim3(kRed), 0, st, partials, nblocks, out, partials2, nblocks2,
                       out2);
}
template <int D>
void launch_pack_export(int mode, int nExp, const int* expOff, const double* z, const double* u, const double* gs,
                        double w, double* out, hipStream_t st, const PackZX& zx) {
  if (nExp <= 0) return;
  hipLaunchKernelGGL(k_pack_export<D>, dim3((nExp + kBlock - 1) / kBlock), dim3(kBlock), 0, st, mode, nExp, expOff, z, u,
                     gs, w, out, zx);
}
#define MMX_INST(D)                                                                                                   \
  template void launch_pack_export<D>(int, int, const int*, const double*, const double*, const double*, double,      \
                                      double*, hipStream_t, const PackZX&);                                           \
  template void launch_gather_z<D>(const DeviceMesh<D>&, const double*, double*, hipStream_t);                        \
  template void launch_grad_simplex<D>(const DeviceMesh<D>&, const double*, double*, bool, double*, int*, hipStream_t); \
  template void launch_predict<D>(const DeviceMesh<D>&, const EngineKnobs&, int, const double*, double*, double*,     \
                                  double*, double, hipStream_t);                                                      \
  template void launch_xupdate<D>(const DeviceMesh<D>&, const EngineKnobs&, const StepScalars&, const double*,        \
                                  const double*, const double*, double*, double*, int*, bool, hipStream_t, bool);     \
  template void launch_energy<D>(const DeviceMesh<D>&, const double*, double*, int*, hipStream_t);                    \
  template void launch_euler_apply<D>(const DeviceMesh<D>&, const EngineKnobs&, const double*, double*, double,       \
                                      hipStream_t);
MMX_INST(2)
MMX_INST(3)
}  // namespace mmx
extern "C" unsigned mmx_layout_admm_step(void) { return mmx::kLayoutWord; }  // layout.h: this object's word
