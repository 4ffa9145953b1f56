// quality_kernels.hip -- Huang's alignment, geometry and equidistribution measures of a mesh on the
// device (arithmetic: quality_math.h, shared with the host's mmadmm_mesh_quality).
//   element pass   one simplex per lane in natural simplex id: gathers its vertex ids (3D: one
//                  16-byte load), then its D + 1 positions, its D + 1 tensors (when there are any)
//                  and its D + 1 computational vertices (when there is such a mesh) -- all of them
//                  requested before any is used -- and stores Q_geo, Q_ali and e_K component-major
//                  (coalesced).  Per workgroup: the partials of sigma, |Omega|, Vhat, sum Q_geo,
//                  sum Q_ali and the invalid count by the block tree, and the two maxima
//   finaliser      one workgroup: fin_sum<256> over each row of partials, the maxima, the record
//   Q_eq pass      e_K -> Q_eq in place, the per-workgroup maxima
//   finaliser      one workgroup: max Q_eq into the record
// The partials change hands at the kernel boundaries: no in-launch ticket, no float atomics, every
// sum in the fixed order of block_reduce.h -- bitwise reproducible, and equal to the host's.
#include <hip/hip_runtime.h>

#include "block_reduce.h"
#include "quality_kernels.h"
#include "quality_math.h"

namespace mmx {
namespace {

constexpr int kQB = 256;

// the block's maxima of NV values per thread (quality_max: from 0.0, no NaN) into v on every thread
template <int NV>
__device__ __forceinline__ void block_max(double (&v)[NV], double (*red)[NV]) {
#pragma unroll
  for (int i = 0; i < NV; ++i) red[threadIdx.x][i] = v[i];
  __syncthreads();
  for (int w = kQB / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
#pragma unroll
      for (int i = 0; i < NV; ++i) red[threadIdx.x][i] = quality_max(red[threadIdx.x][i], red[threadIdx.x + w][i]);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = red[0][i];
}

template <int D>
__device__ __forceinline__ void load_simplex(const int* __restrict__ F, int s, int* f) {
  if (D == 3) {
    const int4 r = reinterpret_cast<const int4*>(F)[s];
    f[0] = r.x;
    f[1] = r.y;
    f[2] = r.z;
    f[3 % (D + 1)] = r.w;
  } else {
#pragma unroll
    for (int n = 0; n < D + 1; ++n) f[n] = F[(size_t)s * (D + 1) + n];
  }
}

template <int D, bool TENSORS, bool XC>
__global__ void __launch_bounds__(kQB) k_quality_elem(const double* __restrict__ X, const int* __restrict__ F, int nF,
                                                      const double* __restrict__ M, const double* __restrict__ Xc,
                                                      QualityRef ref, double* __restrict__ qGeo,
                                                      double* __restrict__ qAli, double* __restrict__ eK,
                                                      double* __restrict__ cK, double* __restrict__ part) {
  constexpr int DD = D * D;
  __shared__ double red[kQB][kQualitySums];
  __shared__ double mred[kQB][2];
  const int s = blockIdx.x * kQB + threadIdx.x;
  double sum[kQualitySums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double mx[2] = {0.0, 0.0};
  if (s < nF) {
    int f[D + 1];
    load_simplex<D>(F, s, f);
    double x[D + 1][D], eh[D][D], m[TENSORS ? (D + 1) * DD : 1];
    double xc[XC ? D + 1 : 1][D];
    // every gather of the simplex before the first use of one
#pragma unroll
    for (int n = 0; n < D + 1; ++n)
#pragma unroll
      for (int k = 0; k < D; ++k) x[n][k] = X[(size_t)f[n] * D + k];
    if (XC) {
#pragma unroll
      for (int n = 0; n < D + 1; ++n)
#pragma unroll
        for (int k = 0; k < D; ++k) xc[n][k] = Xc[(size_t)f[n] * D + k];
    }
    if (TENSORS) {
#pragma unroll
      for (int n = 0; n < D + 1; ++n)
#pragma unroll
        for (int i = 0; i < DD; ++i) m[n * DD + i] = M[(size_t)f[n] * DD + i];
    }
    if (XC) {
#pragma unroll
      for (int j = 0; j < D; ++j)
#pragma unroll
        for (int k = 0; k < D; ++k) eh[j][k] = xc[(j + 1) % (XC ? D + 1 : 1)][k] - xc[0][k];
    } else {
      quality_ref_edges<D>(ref.Ehat, eh);
    }
    const QualityElem r = quality_element<D>(x, eh, TENSORS ? m : nullptr);
    if (qGeo) {
      qGeo[s] = r.geo;
      qAli[s] = r.ali;
    }
    eK[s] = r.e;
    if (XC) cK[s] = r.c;
    sum[0] = r.valid ? r.e : 0.0;
    sum[1] = r.vol;
    sum[2] = quality_c_term(r.c);
    sum[3] = r.geo;
    sum[4] = r.ali;
    sum[5] = r.valid ? 0.0 : 1.0;
    mx[0] = quality_max(0.0, r.geo);
    mx[1] = quality_max(0.0, r.ali);
  }
  block_sum<kQualitySums, kQB>(sum, red);
  block_max<2>(mx, mred);
  if (threadIdx.x == 0) {
    const size_t nblk = gridDim.x;
#pragma unroll
    for (int k = 0; k < kQualitySums; ++k) part[k * nblk + blockIdx.x] = sum[k];
    part[kQualitySums * nblk + blockIdx.x] = mx[0];
    part[(kQualitySums + 1) * nblk + blockIdx.x] = mx[1];
  }
}

// one workgroup: fin_sum<256> (block_reduce.h) of NV rows of nblk partials at once.  Per row the same
// additions in the same order -- lane t adds the partials t, t + 256, ... to 0.0 one by one, then the
// block tree -- but the loads of kFinAhead strides of every row are requested before any is added:
// a lane of the plain loop waits for one load per addition (measured: 81 us for the eight rows of
// the C3 disc's 7,803 partials, twice the element pass)
constexpr int kFinAhead = 4;
template <int NV, bool MAX>
__device__ __forceinline__ void fin_rows(const double* __restrict__ part, int nblk, double (&v)[NV],
                                         double (*red)[NV]) {
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = 0.0;
  for (int b = threadIdx.x; b < nblk; b += kFinAhead * kQB) {
    double t[kFinAhead][NV];
#pragma unroll
    for (int u = 0; u < kFinAhead; ++u)
#pragma unroll
      for (int i = 0; i < NV; ++i) t[u][i] = b + u * kQB < nblk ? part[(size_t)i * nblk + b + u * kQB] : 0.0;
#pragma unroll
    for (int u = 0; u < kFinAhead; ++u)
      if (b + u * kQB < nblk) {
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = MAX ? quality_max(v[i], t[u][i]) : v[i] + t[u][i];
      }
  }
  if (MAX)
    block_max<NV>(v, red);
  else
    block_sum<NV, kQB>(v, red);
  __syncthreads();
}

__global__ void __launch_bounds__(kQB) k_quality_fin(const double* __restrict__ part, int nblk, int nF,
                                                     double* __restrict__ rec) {
  __shared__ double red[kQB][kQualitySums];
  __shared__ double mred[kQB][2];
  double s[kQualitySums], m[2];
  fin_rows<kQualitySums, false>(part, nblk, s, red);
  fin_rows<2, true>(part + (size_t)kQualitySums * nblk, nblk, m, mred);
  const double mg = m[0], ma = m[1];
  if (threadIdx.x == 0) {
    rec[0] = mg;
    rec[1] = ma;
    rec[2] = 0.0;
    rec[3] = s[3] / (double)nF;
    rec[4] = s[4] / (double)nF;
    rec[5] = s[0];
    rec[6] = s[1];
    rec[7] = s[5];
    rec[kQualityVhat] = s[2];
  }
}

// e_K -> Q_eq in place (store false: only the maxima); cK null: cConst for every simplex
__global__ void __launch_bounds__(kQB) k_quality_eq(double* __restrict__ e, const double* __restrict__ cK,
                                                    double cConst, int nF, const double* __restrict__ rec, bool store,
                                                    double* __restrict__ part) {
  __shared__ double red[kQB][1];
  const int s = blockIdx.x * kQB + threadIdx.x;
  const double sigma = rec[5], vhat = rec[kQualityVhat];
  double mx[1] = {0.0};
  if (s < nF) {
    const double q = quality_eq(e[s], cK ? cK[s] : cConst, sigma, vhat);
    if (store) e[s] = q;
    mx[0] = quality_max(0.0, q);
  }
  block_max<1>(mx, red);
  if (threadIdx.x == 0) part[blockIdx.x] = mx[0];
}

__global__ void __launch_bounds__(kQB) k_quality_fin_eq(const double* __restrict__ part, int nblk,
                                                        double* __restrict__ rec) {
  __shared__ double red[kQB][1];
  double m[1];
  fin_rows<1, true>(part, nblk, m, red);
  if (threadIdx.x == 0) rec[2] = m[0];
}

template <int D, bool TENSORS, bool XC>
void launch_elem(const double* X, const int* F, int nF, const double* M, const double* Xc, const QualityRef& ref,
                 double* qGeo, double* qAli, double* e, double* cK, double* part, hipStream_t st) {
  hipLaunchKernelGGL((k_quality_elem<D, TENSORS, XC>), dim3(quality_blocks(nF)), dim3(kQB), 0, st, X, F, nF, M, Xc, ref,
                     qGeo, qAli, e, cK, part);
}

}  // namespace

template <int D>
void launch_quality(const double* X, const int* F, int nF, const double* M, const double* Xc, const QualityRef& ref,
                    double* q, double* eK, double* cK, double* part, double* rec, hipStream_t st) {
  if (nF < 1) return;
  const int nblk = quality_blocks(nF);
  double* qGeo = q;
  double* qAli = q ? q + nF : nullptr;
  double* e = q ? q + (size_t)2 * nF : eK;
  if (M && Xc)
    launch_elem<D, true, true>(X, F, nF, M, Xc, ref, qGeo, qAli, e, cK, part, st);
  else if (M)
    launch_elem<D, true, false>(X, F, nF, M, Xc, ref, qGeo, qAli, e, cK, part, st);
  else if (Xc)
    launch_elem<D, false, true>(X, F, nF, M, Xc, ref, qGeo, qAli, e, cK, part, st);
  else
    launch_elem<D, false, false>(X, F, nF, M, Xc, ref, qGeo, qAli, e, cK, part, st);
  hipLaunchKernelGGL(k_quality_fin, dim3(1), dim3(kQB), 0, st, (const double*)part, nblk, nF, rec);
  double cConst = 0.0;
  if (!Xc) {  // one reference simplex: c_K as quality_element forms it
    double eh[D][D], cr[D][D];
    quality_ref_edges<D>(ref.Ehat, eh);
    cConst = quality_abs(quality_adjugate<D>(eh, cr)) / (D == 2 ? 2.0 : 6.0);
  }
  double* part2 = part + (size_t)kQualityPartials * nblk;
  hipLaunchKernelGGL(k_quality_eq, dim3(nblk), dim3(kQB), 0, st, e, (const double*)(Xc ? cK : nullptr), cConst, nF,
                     (const double*)rec, q != nullptr, part2);
  hipLaunchKernelGGL(k_quality_fin_eq, dim3(1), dim3(kQB), 0, st, (const double*)part2, nblk, rec);
}

template void launch_quality<2>(const double*, const int*, int, const double*, const double*, const QualityRef&,
                                double*, double*, double*, double*, double*, hipStream_t);
template void launch_quality<3>(const double*, const int*, int, const double*, const double*, const QualityRef&,
                                double*, double*, double*, double*, double*, hipStream_t);

}  // namespace mmx
