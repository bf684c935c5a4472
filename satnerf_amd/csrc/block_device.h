// Wave and workgroup primitives shared by the data and evaluation kernels.  They carry those kernels'
// exactness claims, so each states the order it guarantees.
//
// Deliberately NOT unified here -- each of these is a different function or a different schedule, not a copy:
//   * dsm_register.hip's reduce_kernel sums with an LDS tree, not block_sum: switching would change the last bits of the
//     registration statistics.
//   * the two `reflect` helpers: image_metrics.hip's is torch's reflect (-1 -> 1), tie_points.hip's is scipy's half-sample-symmetric
//     one (-1 -> 0).
//   * the two exclusive scans: tie_points.hip scans in place in one workgroup, cloud_grid.hip in three launches; merging them changes
//     launches and time.
//   * tie_points.hip's grid_setup_kernel reduction: 1024 threads, fmin / fmax on doubles, and NaN handled differently from keys.
#pragma once
#include <hip/hip_runtime.h>

namespace sr {

// fp bits <-> unsigned key whose integer order is the numeric order (-0 below +0): min / max become exact integer compares and
// atomics, independent of arrival order
__device__ __forceinline__ unsigned long long order_key(double x) {
  const unsigned long long b = __double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double from_key(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
__device__ __forceinline__ unsigned order_key(float x) {
  const unsigned b = __float_as_uint(x);
  return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float from_key(unsigned k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }
constexpr unsigned kKeyPosInf = 0xff800000u;  // order_key(+inf) in fp32: the neutral element of min
constexpr unsigned kKeyNegInf = 0x007fffffu;  // order_key(-inf) in fp32: the neutral element of max

// Wave min / max of N keys by xor shuffles: even slots take the minimum, odd slots the maximum; all 64 lanes take part and all end
// with the result.  One step (for a kernel that reduces something else in the same loop), and the whole order 32, 16, .. 1.
template <typename K, int N>
__device__ __forceinline__ void wave_minmax_step(K (&k)[N], int off) {
#pragma unroll
  for (int v = 0; v < N; ++v) {
    const K o = __shfl_xor(k[v], off);
    k[v] = (v & 1) ? (o > k[v] ? o : k[v]) : (o < k[v] ? o : k[v]);
  }
}
template <typename K, int N>
__device__ __forceinline__ void wave_minmax(K (&k)[N]) {
  for (int off = 32; off >= 1; off >>= 1) wave_minmax_step(k, off);
}

// Fixed-order sum over a 256-thread workgroup: xor shuffles 32 .. 1 within each wave, then thread 0 adds the four wave sums in wave
// order and holds the totals.  Every thread calls it (one barrier).
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N]) {
  __shared__ double red[N][4];
  for (int off = 32; off >= 1; off >>= 1)
    for (int q = 0; q < N; ++q) v[q] += __shfl_xor(v[q], off);
  if ((threadIdx.x & 63) == 0)
    for (int q = 0; q < N; ++q) red[q][threadIdx.x / 64] = v[q];
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int q = 0; q < N; ++q) v[q] = red[q][0];
  for (int k = 1; k < 4; ++k)
    for (int q = 0; q < N; ++q) v[q] += red[q][k];
}

// v[q] = from 0.0, elements t, t + 256, .. (t = this thread) of row q of part's N rows of P doubles, in that order
template <int N>
__device__ __forceinline__ void strided_sum(const double* __restrict__ part, int P, double (&v)[N]) {
  for (int q = 0; q < N; ++q) v[q] = 0.0;
  for (int k = threadIdx.x; k < P; k += 256)
    for (int q = 0; q < N; ++q) v[q] += part[q * P + k];
}

}  // namespace sr
