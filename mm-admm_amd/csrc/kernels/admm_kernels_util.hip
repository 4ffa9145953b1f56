// admm_kernels_util.hip -- outside the time step: the two test kernels (one-simplex blockGrad, device
// math) and the monitor grid's padded and isotropic copies.
#include "admm_common.h"

namespace mmx {
// one-simplex evaluation for tests: Mesh::computeBlockGrad (regularised, FIXED rows zeroed)
template <int D>
__global__ void k_debug_blockgrad(DeviceMesh<D> m, int s, const double* __restrict__ zin,
                                  const double* __restrict__ dxin, double* __restrict__ out, int flags) {
  constexpr int K = D * (D + 1);
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int f[D + 1];
  loadVerts<D>(m, s, f);
  double z[K], dx[K], xi[K], g[K], Igt = 0;
  for (int i = 0; i < K; ++i) {
    z[i] = zin[i];
    dx[i] = dxin[i];
    g[i] = 0;
  }
  loadXi<D>(m, f, xi);
  double e;
  if (flags & 1) {
    e = (flags & 2) ? blockGrad<D, true, true>(gridOf<D>(m), constsOf<D>(m), z, xi, dx, g, Igt)
                    : blockGrad<D, true, false>(gridOf<D>(m), constsOf<D>(m), z, xi, dx, g, Igt);
    zeroFixed<D>(g, m.sbits[s] & 0xF);
  } else {
    e = (flags & 2) ? blockGrad<D, false, true>(gridOf<D>(m), constsOf<D>(m), z, xi, dx, g, Igt)
                    : blockGrad<D, false, false>(gridOf<D>(m), constsOf<D>(m), z, xi, dx, g, Igt);
  }
  out[0] = e;
  out[1] = Igt;
  for (int i = 0; i < K; ++i) out[2 + i] = g[i];
}

__global__ void k_devmath(int op, int n, const double* __restrict__ in, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (op == 5) {  // quotient pairs (x, c) -> RN(x/c) by div_mk (no range check here)
    if (2 * i + 1 < n) {
      const double xx = in[2 * i], c = in[2 * i + 1];
      out[i] = div_mk(xx, c, 1.0 / c);
    }
    return;
  }
  if (op == 10) {  // the double-double sqrt the powers use: pairs (s, e) for in[0 .. n/2)
    if (2 * i + 1 < n) {
      double sv, ev, hv;
      dd_sqrt_h(in[i], sv, ev, hv);
      out[2 * i] = sv;
      out[2 * i + 1] = ev;
    }
    return;
  }
  const double x = in[i];
  double r;
  bool tie = false;
  switch (op) {
    case 0: r = cr_sqrt(x); break;
    case 1: r = cr_pow_p15(x); break;
    case 2: r = cr_pow_m05(x); break;
    case 3: r = cr_pow_p225(x); break;
    case 4: r = cr_pow_p125(x); break;
    // the prox kernels' fast path (no tie resolution): NaN where it would defer to the exact path
    case 6: r = cr_pow_p15<false>(x, tie); break;
    case 7: r = cr_pow_m05<false>(x, tie); break;
    case 8: r = cr_pow_p225<false>(x, tie); break;
    default: r = cr_pow_p125<false>(x, tie); break;
  }
  out[i] = tie ? __builtin_nan("") : r;
}

// the monitor grid's derived copies (admm_kernels.h: launch_pad_rows, launch_iso_compact)
__global__ void __launch_bounds__(kBlock) k_pad_rows(const double* __restrict__ vals, long long rows,
                                                      double* __restrict__ pad) {
  const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (r >= rows) return;
  for (int n = 0; n < 9; ++n) pad[r * 10 + n] = vals[r * 9 + n];
  pad[r * 10 + 9] = 0.0;
}
template <int D>
__global__ void __launch_bounds__(kBlock) k_iso_compact(const double* __restrict__ vals, long long n,
                                                        double* __restrict__ iso, int* __restrict__ notIso) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double* v = vals + i * D * D;
  const unsigned long long d0 = __double_as_longlong(v[0]);
  bool ok = true, nan = true;
#pragma unroll
  for (int k = 0; k < D * D; ++k) {
    const unsigned long long b = __double_as_longlong(v[k]);
    ok = ok && (b == ((k / D == k % D) ? d0 : 0ull));
    nan = nan && (v[k] != v[k]);
  }
  if (!(ok || nan)) *notIso = 1;  // (every writer stores the same value)
  iso[i] = v[0];
}
template <int D>
void launch_iso_compact(const double* vals, long long points, double* iso, int* notIso, hipStream_t st) {
  if (points > 0)
    hipLaunchKernelGGL(k_iso_compact<D>, dim3((unsigned)((points + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, vals,
                       points, iso, notIso);
}
template void launch_iso_compact<2>(const double*, long long, double*, int*, hipStream_t);
template void launch_iso_compact<3>(const double*, long long, double*, int*, hipStream_t);

void launch_pad_rows(const double* vals, long long rows, double* pad, hipStream_t st) {
  if (rows > 0) hipLaunchKernelGGL(k_pad_rows, dim3((unsigned)((rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, vals, rows, pad);
}
template <int D>
void launch_debug_blockgrad(const DeviceMesh<D>& m, int s, const double* z, const double* dx, double* out, int flags,
                            hipStream_t st) {
  hipLaunchKernelGGL(k_debug_blockgrad<D>, dim3(1), dim3(64), 0, st, m, s, z, dx, out, flags);
}
template void launch_debug_blockgrad<2>(const DeviceMesh<2>&, int, const double*, const double*, double*, int, hipStream_t);
template void launch_debug_blockgrad<3>(const DeviceMesh<3>&, int, const double*, const double*, double*, int, hipStream_t);
void launch_devmath(int op, int n, const double* in, double* out, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_devmath, dim3((n + 255) / 256), dim3(256), 0, st, op, n, in, out);
}
}  // namespace mmx
extern "C" unsigned mmx_layout_admm_util(void) { return mmx::kLayoutWord; }  // layout.h: this object's word
