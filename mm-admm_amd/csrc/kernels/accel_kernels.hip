// accel_kernels.hip -- the LASolver accelerators besides CG-STAB and the row scaling, as HIP
// kernels for gfx950: scal (ILU_class.cpp:904-954), scaler_orthomin::acc_scaler
// (accel_class.cpp:105-191) and scaler_conj::acc_scaler (accel_class.cpp:402-491).  All arithmetic
// is fp64 with every product and sum rounded as the reference writes it (-ffp-contract=off).
//
// Every sum has the shape of the CG-STAB vector kernels (sparse_kernels.hip): grid vec_grid(n),
// element i = block * 256 + lane, stride grid * 256, a fixed 256-lane tree per workgroup, then the
// strided 256-lane finaliser over the per-workgroup partials -- vecTree / finTree of
// oracle/lasolver.cpp.  The order is pinned so the iterates are reproducible bit for bit
// (tests/accel_restate.py restates it); no floating-point atomics, no wave shuffles.
//
// Partials are laid out [value][block], so the finalisers read them coalesced.
#include <hip/hip_runtime.h>

#include "block_reduce.h"  // block_sum, fin_sum: the reduction shared with sparse_kernels.hip
#include "sparse_kernels.h"

namespace mmx {

namespace {

constexpr int kDotGroup = 4;  // stored Aq vectors per read of Avk in k_omin_dots

// max(a, b) of <algorithm> as the reference's convergence test uses it (a NaN first operand stays)
__device__ __forceinline__ double max_ref(double a, double b) { return (a < b) ? b : a; }

}  // namespace

// ---------------------------------------------------------------------------------------------
// scal(n, ia, ja, a, b, scal_fac, 0): one workgroup per SpMV row block {r0, r1, ia[r0], ia[r1]}.
// The block's factors f = 1 / (a[diag] + 1e-300) and row starts go to LDS (lanes over rows, which
// also scale b and store a_scal); after a barrier the block's entries are streamed once, coalesced,
// each multiplied by its row's factor (the row found by bisection of the staged row starts).
__global__ void __launch_bounds__(kSpmvBlock) k_scale_rows(const int4* __restrict__ desc, const int* __restrict__ ia,
                                                            const int* __restrict__ adiag, double* __restrict__ a,
                                                            double* __restrict__ b, double* __restrict__ a_scal) {
  constexpr int kMaxRows = 4 * kSpmvBlock;  // rows of one SpMV row block at most (sparse.cpp)
  __shared__ double s_f[kMaxRows];
  __shared__ int s_ia[kMaxRows + 1];
  const int4 d = desc[blockIdx.x];
  const int r0 = d.x, nr = d.y - d.x, k0 = d.z, k1 = d.w;
  const double eps = 1.0e-300;
  for (int r = threadIdx.x; r < nr; r += kSpmvBlock) {
    const double f = 1.0 / (a[adiag[r0 + r]] + eps);
    s_f[r] = f;
    s_ia[r] = ia[r0 + r];
    a_scal[r0 + r] = f;
    b[r0 + r] = b[r0 + r] * f;
  }
  if (threadIdx.x == 0) s_ia[nr] = k1;
  __syncthreads();
  for (int k = k0 + (int)threadIdx.x; k < k1; k += kSpmvBlock) {
    int lo = 0, hi = nr - 1;  // the last row whose start is <= k
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (s_ia[mid] <= k)
        lo = mid;
      else
        hi = mid - 1;
    }
    a[k] = a[k] * s_f[lo];
  }
}

// ---------------------------------------------------------------------------------------------
// ORTHOMIN.  q / Aq: north vectors of n, vector j at j * n.  oms: AqAq[north], then a_mult[north].

// partials[j][block] of (Avk, Aq[j]) for j < k: Avk is read once per group of kDotGroup vectors.
__global__ void __launch_bounds__(kVecBlock) k_omin_dots(int n, int k, const double* __restrict__ avk,
                                                          const double* __restrict__ Aq, double* __restrict__ partials) {
  __shared__ double red[kVecBlock][kDotGroup];
  for (int g0 = 0; g0 < k; g0 += kDotGroup) {
    const int cnt = (k - g0 < kDotGroup) ? k - g0 : kDotGroup;
    double pv[kDotGroup];
#pragma unroll
    for (int g = 0; g < kDotGroup; ++g) pv[g] = 0.0;
    for (int i = blockIdx.x * kVecBlock + threadIdx.x; i < n; i += gridDim.x * kVecBlock) {
      const double x = avk[i];
#pragma unroll
      for (int g = 0; g < kDotGroup; ++g)
        if (g < cnt) pv[g] += x * Aq[(size_t)(g0 + g) * n + i];
    }
    block_sum<kDotGroup, kVecBlock>(pv, red);
    if (threadIdx.x == 0)
#pragma unroll
      for (int g = 0; g < kDotGroup; ++g)
        if (g < cnt) partials[(size_t)(g0 + g) * gridDim.x + blockIdx.x] = pv[g];
    __syncthreads();  // red is reused by the next group
  }
}

// a_mult[j] = -(Avk, Aq[j]) / (AqAq[j] + tiny), j < k: workgroup j finalises dot j
__global__ void __launch_bounds__(kVecBlock) k_omin_fin_dots(const double* __restrict__ partials, int nblk, int north,
                                                              double* __restrict__ oms) {
  __shared__ double red[kVecBlock][1];
  const double tiny = 1.e-300;
  const int j = blockIdx.x;
  const double s = fin_sum<kVecBlock>(partials + (size_t)j * nblk, nblk, red);
  if (threadIdx.x == 0) oms[north + j] = -s / (oms[j] + tiny);
}

// q[k] = vk + sum a_mult[j] q[j], Aq[k] = Avk + sum a_mult[j] Aq[j] (j ascending, each term rounded
// as written), and the partials of (Aq[k], Aq[k]) and (Aq[k], res) from the values just formed.
__global__ void __launch_bounds__(kVecBlock) k_omin_orth(int n, int k, int north, const double* __restrict__ vk,
                                                          const double* __restrict__ avk, const double* __restrict__ res,
                                                          double* q, double* Aq, const double* __restrict__ oms,
                                                          double* __restrict__ partials) {
  __shared__ double red[kVecBlock][2];
  const double* amult = oms + north;
  double pv[2] = {0.0, 0.0};
  for (int i = blockIdx.x * kVecBlock + threadIdx.x; i < n; i += gridDim.x * kVecBlock) {
    double qv = vk[i], aq = avk[i];
    for (int j = 0; j < k; ++j) {
      const double am = amult[j];
      qv = qv + am * q[(size_t)j * n + i];
      aq = aq + am * Aq[(size_t)j * n + i];
    }
    q[(size_t)k * n + i] = qv;
    Aq[(size_t)k * n + i] = aq;
    pv[0] += aq * aq;
    pv[1] += aq * res[i];
  }
  block_sum<2, kVecBlock>(pv, red);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = pv[0];
    partials[gridDim.x + blockIdx.x] = pv[1];
  }
}

// AqAq[k] = (Aq[k], Aq[k]); ohm = (Aq[k], res) / (AqAq[k] + tiny)
__global__ void __launch_bounds__(kVecBlock) k_omin_fin_orth(const double* __restrict__ partials, int nblk, int k,
                                                              double* __restrict__ oms, AccelScalars* sc) {
  __shared__ double red[kVecBlock][1];
  const double aqaq = fin_sum<kVecBlock>(partials, nblk, red);
  const double aqr = fin_sum<kVecBlock>(partials + nblk, nblk, red);
  if (threadIdx.x != 0) return;
  const double tiny = 1.e-300;
  oms[k] = aqaq;
  sc->ohm = aqr / (aqaq + tiny);
}

// sol += ohm q[k]; res -= ohm Aq[k]; partials [res^2, #max(|step|, |vk|, |q[k]|) > |toler|]
__global__ void __launch_bounds__(kVecBlock) k_omin_update(int n, const double* __restrict__ qk,
                                                            const double* __restrict__ aqk, const double* __restrict__ vk,
                                                            const double* __restrict__ toler, double* __restrict__ x,
                                                            double* __restrict__ res, const AccelScalars* __restrict__ sc,
                                                            double* __restrict__ partials) {
  __shared__ double red[kVecBlock][2];
  const double ohm = sc->ohm;
  double pv[2] = {0.0, 0.0};
  for (int i = blockIdx.x * kVecBlock + threadIdx.x; i < n; i += gridDim.x * kVecBlock) {
    const double qi = qk[i];
    const double step = ohm * qi;
    x[i] = x[i] + step;
    const double r = res[i] - ohm * aqk[i];
    res[i] = r;
    double temp = max_ref(fabs(step), fabs(vk[i]));
    temp = max_ref(temp, fabs(qi));
    const double tl = toler ? toler[i] : 0.0;
    if (temp > fabs(tl)) pv[1] += 1.0;
    pv[0] += r * r;
  }
  block_sum<2, kVecBlock>(pv, red);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = pv[0];
    partials[gridDim.x + blockIdx.x] = pv[1];
  }
}

// ---------------------------------------------------------------------------------------------
// Conjugate gradients.

// first: q = v, aq = avk; later: q = v + aconj q, aq = avk + aconj aq.  Partials of (q, aq).
__global__ void __launch_bounds__(kVecBlock) k_cg_dir(int n, int first, const double* __restrict__ v,
                                                       const double* __restrict__ avk, double* __restrict__ q,
                                                       double* __restrict__ aq, const AccelScalars* __restrict__ sc,
                                                       double* __restrict__ partials) {
  __shared__ double red[kVecBlock][1];
  const double aconj = first ? 0.0 : sc->aconj;
  double pv[1] = {0.0};
  for (int i = blockIdx.x * kVecBlock + threadIdx.x; i < n; i += gridDim.x * kVecBlock) {
    double qi, aqi;
    if (first) {
      qi = v[i];
      aqi = avk[i];
    } else {
      qi = v[i] + aconj * q[i];
      aqi = avk[i] + aconj * aq[i];
    }
    q[i] = qi;
    aq[i] = aqi;
    pv[0] += qi * aqi;
  }
  block_sum<1, kVecBlock>(pv, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = pv[0];
}

// x += ohm q; res -= ohm aq; partials [res^2, #(|ohm q| or |q| or |v|) > |toler|]
__global__ void __launch_bounds__(kVecBlock) k_cg_update(int n, const double* __restrict__ q,
                                                          const double* __restrict__ aq, const double* __restrict__ v,
                                                          const double* __restrict__ toler, double* __restrict__ x,
                                                          double* __restrict__ res, const AccelScalars* __restrict__ sc,
                                                          double* __restrict__ partials) {
  __shared__ double red[kVecBlock][2];
  const double ohm = sc->ohm;
  double pv[2] = {0.0, 0.0};
  for (int i = blockIdx.x * kVecBlock + threadIdx.x; i < n; i += gridDim.x * kVecBlock) {
    const double qi = q[i];
    const double step = ohm * qi;
    x[i] = x[i] + step;
    const double r = res[i] - ohm * aq[i];
    res[i] = r;
    pv[0] += r * r;
    const double tl = fabs(toler ? toler[i] : 0.0);
    if (fabs(step) > tl || fabs(qi) > tl || fabs(v[i]) > tl) pv[1] += 1.0;
  }
  block_sum<2, kVecBlock>(pv, red);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = pv[0];
    partials[gridDim.x + blockIdx.x] = pv[1];
  }
}

// ---------------------------------------------------------------------------------------------
// Scalar finalisers (one workgroup).  MODE 0: rmsi from k_cgs_init's partials ([block][2]);
// 1: CG's rvk = (res, v) from k_dot_into's partials ([block][2], slot 1) and aconj = rvk / rvkm;
// 2: CG's ohm = rvk / (q, aq), rvkm = rvk; 3: rms, iconv and the convergence flag of an update.
template <int MODE>
__global__ void __launch_bounds__(kVecBlock) k_acc_fin(const double* __restrict__ partials, int nblk, int first,
                                                        AccelScalars* sc) {
  __shared__ double red[kVecBlock][1];
  if (MODE == 0 || MODE == 1) {
    double v[1] = {0.0};
    for (int b = threadIdx.x; b < nblk; b += kVecBlock) v[0] += partials[(size_t)b * 2 + MODE];
    block_sum<1, kVecBlock>(v, red);
    if (threadIdx.x != 0) return;
    if (MODE == 0) {
      sc->rmsi = sqrt(v[0]);
      sc->rms = 0.0;
      sc->iconv = 0.0;
      sc->conv = 0;
    } else {
      sc->rvk = v[0];
      if (!first) sc->aconj = v[0] / sc->rvkm;
    }
  } else if (MODE == 2) {
    const double qaq = fin_sum<kVecBlock>(partials, nblk, red);
    if (threadIdx.x != 0) return;
    sc->ohm = sc->rvk / qaq;
    sc->rvkm = sc->rvk;
  } else {
    const double r2 = fin_sum<kVecBlock>(partials, nblk, red);
    const double cnt = fin_sum<kVecBlock>(partials + nblk, nblk, red);
    if (threadIdx.x != 0) return;
    const double rms = sqrt(r2);
    sc->rms = rms;
    sc->iconv = cnt;
    sc->conv = (cnt == 0.0 || (rms / sc->rmsi) < sc->ctol) ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------
void launch_scale_rows(int nblk, const int4* desc, const int* ia, const int* adiag, double* a, double* b,
                       double* a_scal, hipStream_t st) {
  if (nblk <= 0) return;
  hipLaunchKernelGGL(k_scale_rows, dim3(nblk), dim3(kSpmvBlock), 0, st, desc, ia, adiag, a, b, a_scal);
}

void launch_omin_dots(int n, int k, int north, const double* avk, const double* Aq, double* oms, double* partials,
                      hipStream_t st) {
  if (k <= 0) return;
  const int g = vec_grid(n);
  hipLaunchKernelGGL(k_omin_dots, dim3(g), dim3(kVecBlock), 0, st, n, k, avk, Aq, partials);
  hipLaunchKernelGGL(k_omin_fin_dots, dim3(k), dim3(kVecBlock), 0, st, partials, g, north, oms);
}

void launch_omin_orth(int n, int k, int north, const double* vk, const double* avk, const double* res, double* q,
                      double* Aq, double* oms, AccelScalars* sc, double* partials, hipStream_t st) {
  const int g = vec_grid(n);
  hipLaunchKernelGGL(k_omin_orth, dim3(g), dim3(kVecBlock), 0, st, n, k, north, vk, avk, res, q, Aq, oms, partials);
  hipLaunchKernelGGL(k_omin_fin_orth, dim3(1), dim3(kVecBlock), 0, st, partials, g, k, oms, sc);
}

void launch_omin_update(int n, const double* qk, const double* aqk, const double* vk, const double* toler, double* x,
                        double* res, AccelScalars* sc, double* partials, hipStream_t st) {
  const int g = vec_grid(n);
  hipLaunchKernelGGL(k_omin_update, dim3(g), dim3(kVecBlock), 0, st, n, qk, aqk, vk, toler, x, res, sc, partials);
  hipLaunchKernelGGL(k_acc_fin<3>, dim3(1), dim3(kVecBlock), 0, st, partials, g, 0, sc);
}

void launch_cg_dir(int n, int first, const double* v, const double* avk, double* q, double* aq, AccelScalars* sc,
                   double* partials, hipStream_t st) {
  const int g = vec_grid(n);
  hipLaunchKernelGGL(k_cg_dir, dim3(g), dim3(kVecBlock), 0, st, n, first, v, avk, q, aq, sc, partials);
  hipLaunchKernelGGL(k_acc_fin<2>, dim3(1), dim3(kVecBlock), 0, st, partials, g, first, sc);
}

void launch_cg_update(int n, const double* q, const double* aq, const double* v, const double* toler, double* x,
                      double* res, AccelScalars* sc, double* partials, hipStream_t st) {
  const int g = vec_grid(n);
  hipLaunchKernelGGL(k_cg_update, dim3(g), dim3(kVecBlock), 0, st, n, q, aq, v, toler, x, res, sc, partials);
  hipLaunchKernelGGL(k_acc_fin<3>, dim3(1), dim3(kVecBlock), 0, st, partials, g, 0, sc);
}

void launch_acc_fin(int mode, const double* partials, int nblk, int first, AccelScalars* sc, hipStream_t st) {
  const dim3 g(1), b(kVecBlock);
  if (mode == 0)
    hipLaunchKernelGGL(k_acc_fin<0>, g, b, 0, st, partials, nblk, first, sc);
  else
    hipLaunchKernelGGL(k_acc_fin<1>, g, b, 0, st, partials, nblk, first, sc);
}

}  // namespace mmx
