// admm_common.h -- what every stage of the ADMM kernels (admm_kernels_*.hip, CDNA4 gfx950; reference
// hot path MeshIntegrator<D>::step, src/MeshIntegrator.cpp:101-191) uses: workgroup partial sums (per-
// workgroup slots, reduced in a fixed order: deterministic), the XCD block mappings, the z / u slot
// layout, a simplex kernel's views of DeviceMesh, the launchers' helpers.  Build: -ffp-contract=off.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <type_traits>
#include "admm_device.h"
#include "admm_kernels.h"

namespace mmx {
constexpr int kBlock = 256;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// Workgroup reduction of NV values into partials[blockIdx.x * kNumPartials + i].
// Values 0..3 are summed, 4 is or-ed (as a sum of flags), 5 is a max.
template <int NV, int BS = kBlock>
__device__ __forceinline__ void block_partials(double (&v)[NV], double* partials, int slot = -1) {
  __shared__ double red[BS / 64][kNumPartials];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = (i == 5) ? wave_max(v[i]) : wave_sum(v[i]);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < kNumPartials; ++i) red[wid][i] = (i < NV) ? v[i] : 0.0;
  }
  __syncthreads();
  if (threadIdx.x < kNumPartials) {
    double s = red[0][threadIdx.x];
    for (int w = 1; w < BS / 64; ++w)
      s = (threadIdx.x == 5) ? fmax(s, red[w][threadIdx.x]) : s + red[w][threadIdx.x];
    partials[(size_t)(slot < 0 ? (int)blockIdx.x : slot) * kNumPartials + threadIdx.x] = s;
  }
}

__device__ __forceinline__ int logical_block(int xcd) {
  return xcd ? (int)(blockIdx.x % 8) * (int)(gridDim.x / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
}

// any grid size: XCD x (= blockIdx % 8) takes a contiguous range of q or q + 1 logical blocks
__device__ __forceinline__ int logical_block_any() {
  const int g = (int)gridDim.x, q = g / 8, r = g % 8, x = (int)(blockIdx.x % 8);
  return x * q + min(x, r) + (int)(blockIdx.x / 8);
}

// z and u of simplex s, slot layout i = n D + c (the reference's D x order).  With MMX_ZU_INTER=1
// (2D, a build option, off: measured slower) the two are interleaved per vertex slot,
// [z_n0 z_n1 u_n0 u_n1] (32 B), so the x-update's two gathers of a slot fall in one cache line; the
// buffer then holds 2 K doubles per simplex and u = z + D.  Default: two arrays.
template <int D>
constexpr bool kZUInter = (D == 2) && MMX_ZU_INTER;
template <int D>
__device__ __forceinline__ size_t zu_base(int s) {
  return (size_t)s * (kZUInter<D> ? 2 : 1) * (D * (D + 1));
}
template <int D>
__device__ __forceinline__ int zu_i(int i) {
  return kZUInter<D> ? (i / D) * 2 * D + i % D : i;
}
// an incidence entry's slot offset s K + n D -> where its z values start
template <int D>
__device__ __forceinline__ size_t zu_off(int off) {
  return kZUInter<D> ? 2 * (size_t)off : (size_t)off;
}

// ISO: -1 the monitor path chosen at run time from m.giso; 0 the full-row path only; 1 the
// isotropic path only (m.giso set).  3D kernels are instantiated per path and launched by m.giso
// (dispatch_iso), so neither path's registers count against the other's.
template <int D, int ISO = -1>
__device__ __forceinline__ GridView<D> gridOf(const DeviceMesh<D>& m) {
  GridView<D> g;
  g.gx = m.gx;
  g.gy = m.gy;
  g.gz = m.gz;
  g.vals = m.gvals;
  g.pad = m.gpad;
  g.cell[0] = m.gcell[0];
  g.cell[1] = m.gcell[1];
  g.cell[2] = m.gcell[2];
  g.iso = m.giso;
  g.nx = m.gnx;
  g.ny = m.gny;
  g.nz = m.gnz;
  g.hx = m.ghx;
  g.hy = m.ghy;
  g.hz = m.ghz;
  g.rhx = m.grhx;
  g.rhy = m.grhy;
  g.rhz = m.grhz;
  g.ax = m.gax;
  g.ay = m.gay;
  g.az = m.gaz;
  g.spx = m.gspx;
  g.spy = m.gspy;
  g.spz = m.gspz;
  g.nsx = m.gnsx;
  g.nsy = m.gnsy;
  g.nsz = m.gnsz;
  g.rnsx = m.grnsx;
  g.rnsy = m.grnsy;
  g.rnsz = m.grnsz;
  g.invFlag = m.invFlag;
  if constexpr (ISO == 0)
    g.iso = nullptr;
  else if constexpr (ISO == 1)
    __builtin_assume(g.iso != nullptr);
  return g;
}

template <int D>
__device__ __forceinline__ FunctionalConsts<D> constsOf(const DeviceMesh<D>& m) {
  FunctionalConsts<D> c;
#pragma unroll
  for (int i = 0; i < D * D; ++i) c.Ehat[i] = m.Ehat[i];
  c.powd = m.powd;
  c.w = m.w;
  c.compMesh = m.compMesh;
  return c;
}

template <int D>
__device__ __forceinline__ void loadVerts(const DeviceMesh<D>& m, int s, int (&f)[D + 1]) {
#pragma unroll
  for (int n = 0; n < D + 1; ++n) f[n] = m.F[(size_t)s * (D + 1) + n];
}

template <int D>
__device__ __forceinline__ void gatherX(const double* x, const int (&f)[D + 1], double* out) {
#pragma unroll
  for (int n = 0; n < D + 1; ++n) {
    if constexpr (D == 2) {
      const double2 v = *reinterpret_cast<const double2*>(x + (size_t)f[n] * 2);
      out[n * 2] = v.x;
      out[n * 2 + 1] = v.y;
    } else {
#pragma unroll
      for (int c = 0; c < D; ++c) out[n * D + c] = x[(size_t)f[n] * D + c];
    }
  }
}

template <int D>
__device__ __forceinline__ void loadXi(const DeviceMesh<D>& m, const int (&f)[D + 1], double* xi) {
  if (m.compMesh) gatherX<D>(m.Vc, f, xi);
}

// the x-update's term of the simplex's slots (DeviceMesh::tslot, the layout of z): the same
// expression the x-update forms from z and u (bit-identical)
template <int D>
__device__ __forceinline__ void write_tslot(const DeviceMesh<D>& m, int s, const double* z, const double* u) {
  if (!m.tslot) return;
  constexpr int K = D * (D + 1);
  double* ts = m.tslot + (size_t)s * K;
#pragma unroll
  for (int i = 0; i < K; ++i) ts[i] = m.w * (m.w * (z[i] - u[i]));
}

// ---- host side ----
inline int nblk(int n) { return (n + kBlock - 1) / kBlock; }
// node kernels: grid padded to a multiple of the 8 XCDs, logical blocks dealt in contiguous runs
// per XCD (blocks b and b+8 share an XCD, MI355X_MICROARCH.md §Workgroup dispatch), so the z/u
// lines a run of nodes shares stay in one L2.  xcdMap (EngineKnobs::xcdMap) = 0: the identity mapping.
inline int nblk_xcd(int n, int xcdMap) { return xcdMap ? (nblk(n) + 7) / 8 * 8 : nblk(n); }

// The monitor path of a launch as a compile-time constant, f(std::integral_constant<int, ISO>) with gridOf's
// ISO -- 3D: 1 with an isotropic grid (m.giso), else 0; 2D: -1: a dimension instantiates only what it launches
template <int D, class F>
inline void dispatch_iso(const DeviceMesh<D>& m, F&& f) {
  if constexpr (D != 3)
    f(std::integral_constant<int, -1>{});
  else if (m.giso)
    f(std::integral_constant<int, 1>{});
  else
    f(std::integral_constant<int, 0>{});
}
// a run-time flag as a compile-time constant: f(std::true_type) or f(std::false_type)
template <class F>
inline void dispatch_bool(bool b, F&& f) {
  b ? f(std::true_type{}) : f(std::false_type{});
}
}  // namespace mmx
