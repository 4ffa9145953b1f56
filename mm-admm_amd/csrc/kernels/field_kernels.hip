// field_kernels.hip -- the monitor from a nodal scalar field on the device: gradient recovery by
// volume-weighted averaging, applied twice (u -> g -> G), then H = sym(G), |H| by Jacobi and
// M = I + |H| / alpha (arithmetic: field_math.h, shared with the host's mmadmm_field_monitor).
//   element pass  one simplex per lane: gathers its D + 1 vertices' positions and C values (C = 1
//                 for u, C = D for g: every component in one launch), stores {w, g} simplex-major
//   node pass     one node per lane, in the x-update's node order (neighbouring lanes gather
//                 neighbouring simplices): walks the node's incidence list in ascending simplex id
//                 and sums the element rows -- every contribution stored once with plain stores
//                 and summed per destination in a fixed order: no atomics, bitwise reproducible
// Huang's normalised monitor: the last node pass stores |H|, the Jacobi diagonal l
// and omega per node instead of M; alpha is given, or solved on the device by (k_field_sigma,
// k_field_update) pairs -- the partial sums change hands at the kernel boundary, the state record
// of the search (FieldSolve) lives in device memory -- and a final pass writes M.
// Several components: U is nP x C, the metric A = sum_c w_c |H_c|.  The first recovery
// runs in batches of up to D components that share a simplex's geometry, the second per component
// with a node pass that accumulates A (one lane per node and launch); the last component's launch
// leaves M = I + A / alpha, or {A, l, omega} for the solve and the final pass above.
#include <hip/hip_runtime.h>

#include "block_reduce.h"
#include "field_kernels.h"
#include "field_math.h"

namespace mmx {
namespace {

constexpr int kFB = 256;
inline int fblocks(int n) { return (n + kFB - 1) / kFB; }

template <int D, int C>
__global__ void __launch_bounds__(kFB) k_field_elem(const double* __restrict__ X, const double* __restrict__ val,
                                                    const int* __restrict__ F, int nF, double* __restrict__ ebuf) {
  const int s = blockIdx.x * kFB + threadIdx.x;
  if (s >= nF) return;
  int f[D + 1];
#pragma unroll
  for (int n = 0; n < D + 1; ++n) f[n] = F[(size_t)s * (D + 1) + n];
  double out[1 + C * D];
  field_element<D, C>(X, val, f, out);
  field_store_row<1 + C * D>(out, ebuf + (size_t)s * (1 + C * D));
}

// C = 1: grad[v] = r(u)_v.  C = D: the epilogue, H and / or M of node v
template <int D, int C>
__global__ void __launch_bounds__(kFB) k_field_node(const int* __restrict__ incPtr, const int* __restrict__ incOff,
                                                    const int* __restrict__ nodeOrder, int nP,
                                                    const double* __restrict__ ebuf, double* __restrict__ grad,
                                                    double alpha, double* __restrict__ H, double* __restrict__ M) {
  const int idx = blockIdx.x * kFB + threadIdx.x;
  if (idx >= nP) return;
  const int v = nodeOrder[idx];
  const int b = incPtr[v], e = incPtr[v + 1];
  double r[C * D];
  field_node<D, C>(incOff + b, e - b, ebuf, r);
  if (C == 1) {
#pragma unroll
    for (int i = 0; i < D; ++i) grad[(size_t)v * D + i] = r[i];
  } else {
    field_epilogue<D>(r, alpha, H ? H + (size_t)v * D * D : nullptr, M ? M + (size_t)v * D * D : nullptr);
  }
}

// the epilogue of Huang's monitor: |H| (nP x D*D), and lw = {l_0 .. l_{D-1}, omega}, each nP
// values, component-major (the sums of k_field_sigma stream them by natural node id)
template <int D>
__global__ void __launch_bounds__(kFB) k_field_node_huang(const int* __restrict__ incPtr,
                                                          const int* __restrict__ incOff,
                                                          const int* __restrict__ nodeOrder, int nP,
                                                          const double* __restrict__ ebuf, double* __restrict__ absH,
                                                          double* __restrict__ lw) {
  const int idx = blockIdx.x * kFB + threadIdx.x;
  if (idx >= nP) return;
  const int v = nodeOrder[idx];
  const int b = incPtr[v], e = incPtr[v + 1];
  double r[D * D], sw, A[D * D], l[D], om;
  field_node<D, D>(incOff + b, e - b, ebuf, r, &sw);
  field_huang_node<D>(r, sw, nullptr, A, l, &om);
#pragma unroll
  for (int i = 0; i < D * D; ++i) absH[(size_t)v * D * D + i] = A[i];
#pragma unroll
  for (int k = 0; k < D; ++k) lw[(size_t)k * nP + v] = l[k];
  lw[(size_t)D * nP + v] = om;
}

// ---- several components ----
// first recovery of a batch of B <= D components, columns c0 .. c0 + B - 1 of U (nP x ldu): the
// simplex's positions, adjugate and det are gathered and formed once for the batch; the element row
// {w, g[B][D]} has one of the shapes of k_field_elem's rows
template <int D, int B>
__global__ void __launch_bounds__(kFB) k_fields_elem(const double* __restrict__ X, const double* __restrict__ U,
                                                     int ldu, const int* __restrict__ F, int nF,
                                                     double* __restrict__ ebuf) {
  const int s = blockIdx.x * kFB + threadIdx.x;
  if (s >= nF) return;
  int f[D + 1];
#pragma unroll
  for (int n = 0; n < D + 1; ++n) f[n] = F[(size_t)s * (D + 1) + n];
  double out[1 + B * D];
  field_element_ld<D, B>(X, U, ldu, f, out);
  field_store_row<1 + B * D>(out, ebuf + (size_t)s * (1 + B * D));
}

// the batch's nodal gradients, each component into its own plane (nP x D) of planes: component b of
// the batch into planes + b nP D, the layout k_field_elem<D, D> reads a scalar's gradient in
template <int D, int B>
__global__ void __launch_bounds__(kFB) k_fields_node_grad(const int* __restrict__ incPtr,
                                                          const int* __restrict__ incOff,
                                                          const int* __restrict__ nodeOrder, int nP,
                                                          const double* __restrict__ ebuf,
                                                          double* __restrict__ planes) {
  const int idx = blockIdx.x * kFB + threadIdx.x;
  if (idx >= nP) return;
  const int v = nodeOrder[idx];
  const int b = incPtr[v], e = incPtr[v + 1];
  double r[B * D];
  field_node<D, B>(incOff + b, e - b, ebuf, r);
#pragma unroll
  for (int c = 0; c < B; ++c)
#pragma unroll
    for (int i = 0; i < D; ++i) planes[((size_t)c * nP + v) * D + i] = r[c * D + i];
}

// second recovery of component c with the accumulating epilogue: H_c (Hc: nP rows of ldh doubles,
// may be null), A = w_0 |H_0| (first) or A + w_c |H_c| (Aio, nP x D*D, may be null: H alone).  One
// lane per node and launch, the launches ordered by the stream: no atomics.  The last component's
// launch ends the metric -- FIN = kFieldsPlain: M = I + A / alpha goes to Aio in A's place;
// kFieldsHuang: A stays and lw = {l of A, omega} is written, component-major
template <int D, int FIN>
__global__ void __launch_bounds__(kFB) k_fields_node_acc(const int* __restrict__ incPtr,
                                                         const int* __restrict__ incOff,
                                                         const int* __restrict__ nodeOrder, int nP,
                                                         const double* __restrict__ ebuf, double w, int first,
                                                         double* __restrict__ Hc, int ldh, double* Aio, double alpha,
                                                         double* __restrict__ lw) {
  const int idx = blockIdx.x * kFB + threadIdx.x;
  if (idx >= nP) return;
  const int v = nodeOrder[idx];
  const int b = incPtr[v], e = incPtr[v + 1];
  double r[D * D], sw, h[D * D];
  field_node<D, D>(incOff + b, e - b, ebuf, r, &sw);
  field_symmetrise<D>(r, h);
  if (Hc) {
#pragma unroll
    for (int i = 0; i < D * D; ++i) Hc[(size_t)v * ldh + i] = h[i];
  }
  if (!Aio) return;
  double ab[D * D], a[D * D];
  field_abs_sym<D>(h, ab);
  double* Av = Aio + (size_t)v * D * D;
  field_accumulate<D>(ab, w, first != 0, Av, a);
  if (FIN == kFieldsPlain) {
    double m[D * D];
    field_plain_monitor<D>(a, alpha, m);
#pragma unroll
    for (int i = 0; i < D * D; ++i) Av[i] = m[i];
    return;
  }
#pragma unroll
  for (int i = 0; i < D * D; ++i) Av[i] = a[i];
  if (FIN == kFieldsHuang) {
    double l[D];
    field_metric_diag<D>(a, l);
#pragma unroll
    for (int k = 0; k < D; ++k) lw[(size_t)k * nP + v] = l[k];
    lw[(size_t)D * nP + v] = sw / (double)(D + 1);
  }
}

// the state of the search before its first pass; alpha > 0: nothing to solve
__global__ void k_field_solve_set(FieldSolve* st, double alpha) {
  FieldSolve s;
  s.lo = s.hi = s.trial = s.twoOmega = s.lambda = 0.0;
  s.alpha = alpha;
  s.phase = alpha > 0.0 ? kFieldDone : kFieldInit;
  s.passes = 0;
  *st = s;
}

// one pass of the search: workgroup b sums omega_v rho_v(trial) over the node ids 256 b .. 256 b + 255
// (missing lanes 0.0) by the block tree into part[b].  The first pass (kFieldInit) sums omega_v
// alone and takes the largest l into part[nblk + b].  Nothing once the search is done.
template <int D>
__global__ void __launch_bounds__(kFB) k_field_sigma(const double* __restrict__ lw, int nP, const FieldSolve* st,
                                                     double* __restrict__ part) {
  __shared__ double red[kFB][1];
  const int phase = st->phase;
  if (phase == kFieldDone) return;
  const double trial = st->trial;
  const int v = blockIdx.x * kFB + threadIdx.x;
  double val[1] = {0.0};
  double mx = 0.0;
  if (v < nP) {
    double l[D];
#pragma unroll
    for (int k = 0; k < D; ++k) l[k] = lw[(size_t)k * nP + v];
    const double om = lw[(size_t)D * nP + v];
    if (phase == kFieldInit) {
      val[0] = om;
#pragma unroll
      for (int k = 0; k < D; ++k) mx = l[k] > mx ? l[k] : mx;
    } else {
      val[0] = om * field_huang_rho<D>(l, trial, nullptr);
    }
  }
  block_sum<1, kFB>(val, red);
  if (threadIdx.x == 0) part[blockIdx.x] = val[0];
  if (phase != kFieldInit) return;
  __syncthreads();  // every lane has read red[0]
  red[threadIdx.x][0] = mx;
  __syncthreads();
  for (int w = kFB / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const double o = red[threadIdx.x + w][0];
      if (o > red[threadIdx.x][0]) red[threadIdx.x][0] = o;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) part[gridDim.x + blockIdx.x] = red[0][0];
}

// one workgroup: the pass's sum by fin_sum, then the state record advanced (field_math.h)
__global__ void __launch_bounds__(kFB) k_field_update(FieldSolve* st, const double* __restrict__ part, int nblk) {
  __shared__ double red[kFB][1];
  const int phase = st->phase;
  if (phase == kFieldDone) return;
  const double sum = fin_sum<kFB>(part, nblk, red);
  if (phase == kFieldInit) {
    double mx = 0.0;
    for (int b = threadIdx.x; b < nblk; b += kFB) mx = part[nblk + b] > mx ? part[nblk + b] : mx;
    red[threadIdx.x][0] = mx;
    __syncthreads();
    for (int w = kFB / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) {
        const double o = red[threadIdx.x + w][0];
        if (o > red[threadIdx.x][0]) red[threadIdx.x][0] = o;
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    FieldSolve s = *st;
    if (phase == kFieldInit)
      field_solve_begin(&s, sum, red[0][0]);
    else
      field_solve_advance(&s, sum);
    *st = s;
  }
}

// M = (I + |H| / alpha) / t per node, alpha from the state record
template <int D>
__global__ void __launch_bounds__(kFB) k_field_huang_final(const double* __restrict__ absH,
                                                           const double* __restrict__ lw, int nP,
                                                           const FieldSolve* __restrict__ st, double* __restrict__ M) {
  const int v = blockIdx.x * kFB + threadIdx.x;
  if (v >= nP) return;
  const double alpha = st->alpha;
  double A[D * D], l[D], m[D * D];
#pragma unroll
  for (int i = 0; i < D * D; ++i) A[i] = absH[(size_t)v * D * D + i];
#pragma unroll
  for (int k = 0; k < D; ++k) l[k] = lw[(size_t)k * nP + v];
  field_huang_monitor<D>(A, l, alpha, m);
#pragma unroll
  for (int i = 0; i < D * D; ++i) M[(size_t)v * D * D + i] = m[i];
}

}  // namespace

template <int D>
void launch_field_hessian(const double* X, const double* u, const int* F, int nF, const int* incPtr, const int* incOff,
                          const int* nodeOrder, int nP, double* ebuf, double* grad, double alpha, double* H, double* M,
                          hipStream_t st) {
  if (nF < 1 || nP < 1) return;
  hipLaunchKernelGGL((k_field_elem<D, 1>), dim3(fblocks(nF)), dim3(kFB), 0, st, X, u, F, nF, ebuf);
  hipLaunchKernelGGL((k_field_node<D, 1>), dim3(fblocks(nP)), dim3(kFB), 0, st, incPtr, incOff, nodeOrder, nP, ebuf,
                     grad, alpha, (double*)nullptr, (double*)nullptr);
  hipLaunchKernelGGL((k_field_elem<D, D>), dim3(fblocks(nF)), dim3(kFB), 0, st, X, grad, F, nF, ebuf);
  hipLaunchKernelGGL((k_field_node<D, D>), dim3(fblocks(nP)), dim3(kFB), 0, st, incPtr, incOff, nodeOrder, nP, ebuf,
                     (double*)nullptr, alpha, H, M);
}

template void launch_field_hessian<2>(const double*, const double*, const int*, int, const int*, const int*, const int*,
                                      int, double*, double*, double, double*, double*, hipStream_t);
template void launch_field_hessian<3>(const double*, const double*, const int*, int, const int*, const int*, const int*,
                                      int, double*, double*, double, double*, double*, hipStream_t);

template <int D>
void launch_field_huang_recover(const double* X, const double* u, const int* F, int nF, const int* incPtr,
                                const int* incOff, const int* nodeOrder, int nP, double* ebuf, double* grad,
                                double* absH, double* lw, hipStream_t st) {
  if (nF < 1 || nP < 1) return;
  hipLaunchKernelGGL((k_field_elem<D, 1>), dim3(fblocks(nF)), dim3(kFB), 0, st, X, u, F, nF, ebuf);
  hipLaunchKernelGGL((k_field_node<D, 1>), dim3(fblocks(nP)), dim3(kFB), 0, st, incPtr, incOff, nodeOrder, nP, ebuf,
                     grad, 1.0, (double*)nullptr, (double*)nullptr);
  hipLaunchKernelGGL((k_field_elem<D, D>), dim3(fblocks(nF)), dim3(kFB), 0, st, X, grad, F, nF, ebuf);
  hipLaunchKernelGGL((k_field_node_huang<D>), dim3(fblocks(nP)), dim3(kFB), 0, st, incPtr, incOff, nodeOrder, nP, ebuf,
                     absH, lw);
}

namespace {
template <int D, int B>
void fields_first_recovery(const double* X, const double* U, int ldu, const int* F, int nF, const int* incPtr,
                           const int* incOff, const int* nodeOrder, int nP, double* ebuf, double* planes,
                           hipStream_t st) {
  hipLaunchKernelGGL((k_fields_elem<D, B>), dim3(fblocks(nF)), dim3(kFB), 0, st, X, U, ldu, F, nF, ebuf);
  hipLaunchKernelGGL((k_fields_node_grad<D, B>), dim3(fblocks(nP)), dim3(kFB), 0, st, incPtr, incOff, nodeOrder, nP,
                     (const double*)ebuf, planes);
}
}  // namespace

template <int D>
void launch_fields_recover(const double* X, const double* U, int C, const double* w, const int* F, int nF,
                           const int* incPtr, const int* incOff, const int* nodeOrder, int nP, double* ebuf,
                           double* planes, double* H, double* A, int fin, double alpha, double* lw, hipStream_t st) {
  if (nF < 1 || nP < 1 || C < 1) return;
  for (int c0 = 0; c0 < C; c0 += D) {
    const int B = C - c0 < D ? C - c0 : D;
    double* pl = planes + (size_t)c0 * nP * D;
    if (B == 1)
      fields_first_recovery<D, 1>(X, U + c0, C, F, nF, incPtr, incOff, nodeOrder, nP, ebuf, pl, st);
    else if (B == 2)
      fields_first_recovery<D, 2>(X, U + c0, C, F, nF, incPtr, incOff, nodeOrder, nP, ebuf, pl, st);
    else
      fields_first_recovery<D, D>(X, U + c0, C, F, nF, incPtr, incOff, nodeOrder, nP, ebuf, pl, st);
  }
  const dim3 grid(fblocks(nP)), block(kFB);
  for (int c = 0; c < C; ++c) {
    hipLaunchKernelGGL((k_field_elem<D, D>), dim3(fblocks(nF)), dim3(kFB), 0, st, X,
                       (const double*)(planes + (size_t)c * nP * D), F, nF, ebuf);
    double* Hc = H ? H + (size_t)c * D * D : nullptr;
    const int ldh = C * D * D, first = c == 0;
    const int f = c == C - 1 ? fin : kFieldsNone;
    if (f == kFieldsPlain)
      hipLaunchKernelGGL((k_fields_node_acc<D, kFieldsPlain>), grid, block, 0, st, incPtr, incOff, nodeOrder, nP,
                         (const double*)ebuf, w[c], first, Hc, ldh, A, alpha, lw);
    else if (f == kFieldsHuang)
      hipLaunchKernelGGL((k_fields_node_acc<D, kFieldsHuang>), grid, block, 0, st, incPtr, incOff, nodeOrder, nP,
                         (const double*)ebuf, w[c], first, Hc, ldh, A, alpha, lw);
    else
      hipLaunchKernelGGL((k_fields_node_acc<D, kFieldsNone>), grid, block, 0, st, incPtr, incOff, nodeOrder, nP,
                         (const double*)ebuf, w[c], first, Hc, ldh, A, alpha, lw);
  }
}

template void launch_fields_recover<2>(const double*, const double*, int, const double*, const int*, int, const int*,
                                       const int*, const int*, int, double*, double*, double*, double*, int, double,
                                       double*, hipStream_t);
template void launch_fields_recover<3>(const double*, const double*, int, const double*, const int*, int, const int*,
                                       const int*, const int*, int, double*, double*, double*, double*, int, double,
                                       double*, hipStream_t);

void launch_field_solve_set(FieldSolve* state, double alpha, hipStream_t st) {
  hipLaunchKernelGGL(k_field_solve_set, dim3(1), dim3(1), 0, st, state, alpha);
}

template <int D>
void launch_field_solve_passes(const double* lw, int nP, FieldSolve* state, double* part, int passes, hipStream_t st) {
  const int nblk = field_solve_blocks(nP);
  for (int i = 0; i < passes; ++i) {
    hipLaunchKernelGGL((k_field_sigma<D>), dim3(nblk), dim3(kFB), 0, st, lw, nP, (const FieldSolve*)state, part);
    hipLaunchKernelGGL(k_field_update, dim3(1), dim3(kFB), 0, st, state, (const double*)part, nblk);
  }
}

template <int D>
void launch_field_huang_final(const double* absH, const double* lw, int nP, const FieldSolve* state, double* M,
                              hipStream_t st) {
  if (nP < 1) return;
  hipLaunchKernelGGL((k_field_huang_final<D>), dim3(fblocks(nP)), dim3(kFB), 0, st, absH, lw, nP, state, M);
}

#define MMX_FIELD_HUANG(D)                                                                                          \
  template void launch_field_huang_recover<D>(const double*, const double*, const int*, int, const int*, const int*, \
                                              const int*, int, double*, double*, double*, double*, hipStream_t);    \
  template void launch_field_solve_passes<D>(const double*, int, FieldSolve*, double*, int, hipStream_t);           \
  template void launch_field_huang_final<D>(const double*, const double*, int, const FieldSolve*, double*, hipStream_t);
MMX_FIELD_HUANG(2)
MMX_FIELD_HUANG(3)
#undef MMX_FIELD_HUANG

}  // namespace mmx
