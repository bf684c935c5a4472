// Image metrics for gfx950: the reference's metrics.mse / psnr / ssim (metrics.py:105-121), the PSNR and SSIM
// that eval_satnerf.eval_aoi prints and main.py's validation_step logs.
//
// Two fp64 reductions.  sse_kernel sums (pred - gt)^2 over n fp32 elements (optionally masked); ssim_kernel sums kornia 0.5.3's SSIM
// map (window 3, reflect border) over every pixel of B*C planes.  Each workgroup writes one partial {sum, count} to caller-owned
// scratch and finalize_kernel adds the partials in a fixed order.  The grid, and so every summation order, depends only on the
// shapes: results are bitwise repeatable, with no float atomics and no host synchronisation (capturable).
#include <math.h>

#include "block_device.h"
#include "common.h"

namespace sr {
namespace imgm {

constexpr int kThreads = 256;
constexpr int kMaxPartials = 2048;  // workgroups (= partial slots) of one launch: 8 per CU, grid-strided beyond that
constexpr int kTH = 32, kTW = 64;   // SSIM output tile: 64 columns x 4 row groups of 8 rows
constexpr int kRows = kTH / (kThreads / kTW);
constexpr int kSW = kTW + 2;        // staged tile row: the tile plus a one-pixel halo either side
constexpr int kStage = (kTH + 2) * kSW, kStagePer = (kStage + kThreads - 1) / kThreads;
constexpr int kMaxSide = 1 << 20;

// the 1-D Gaussian of kornia.filters.get_gaussian_kernel1d(3, 1.5): exp(-x^2 / 4.5) at x = -1, 0, 1, normalised to sum 1
constexpr double kG0 = 0.30780132912346997;  // x = +-1
constexpr double kG1 = 0.38439734175306;     // x = 0
constexpr double kC1 = 0.01 * 0.01, kC2 = 0.03 * 0.03, kEps = 1e-12;

inline long sse_partials(int64_t n) { return partial_slots((n + 3) / 4, kThreads, kMaxPartials); }

inline long ssim_tiles(int64_t planes, int h, int w) { return (long)planes * ((h + kTH - 1) / kTH) * ((w + kTW - 1) / kTW); }

inline long ssim_partials(int64_t planes, int h, int w) { return partial_slots(ssim_tiles(planes, h, w), 1, kMaxPartials); }

// ---- sum of squared error ----------------------------------------------------------------------------------------------------------
// Thread t of workgroup g owns the element quads q = g * 256 + t + k * (P * 256), k = 0, 1, ..., and adds the squares of quad q's
// elements 4q .. 4q + 3 (those < n) in order.  d = pred - gt is exact in fp64 for fp32 inputs of similar magnitude; d^2 is rounded
// once in fp64.  mask (optional): element i counts when mask[i / mask_div] != 0.  VEC reads a quad as one float4 (both pointers 16-byte
// aligned); the scalar form reads the same elements in the same order, so the result does not depend on alignment.
template <bool VEC>
__global__ void __launch_bounds__(kThreads) sse_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                       const uint8_t* __restrict__ mask, int64_t mask_div, double* __restrict__ part) {
  const int64_t P = gridDim.x, quads = (n + 3) / 4;
  double s = 0.0, c = 0.0;
  for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < quads; q += P * kThreads) {
    const int64_t i0 = 4 * q;
    float x[4], y[4];
    if (VEC && i0 + 4 <= n) {
      const float4 u = reinterpret_cast<const float4*>(a)[q], v = reinterpret_cast<const float4*>(b)[q];
      x[0] = u.x, x[1] = u.y, x[2] = u.z, x[3] = u.w;
      y[0] = v.x, y[1] = v.y, y[2] = v.z, y[3] = v.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = i0 + k < n ? a[i0 + k] : 0.f, y[k] = i0 + k < n ? b[i0 + k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t i = i0 + k;
      if (i < n && (!mask || mask[i / mask_div])) {
        const double d = (double)x[k] - (double)y[k];
        s += d * d, c += 1.0;
      }
    }
  }
  double v[2] = {s, c};
  block_sum(v);
  if (threadIdx.x == 0) part[blockIdx.x] = v[0], part[P + blockIdx.x] = v[1];
}

// ---- SSIM map sum ------------------------------------------------------------------------------------------------------------------
// Reflect indexing of torch F.pad(mode='reflect') / kornia filter2D's default border: -1 -> 1, n -> n - 2 (n >= 2).  Rows and columns
// further out are only staged for output pixels outside the image, which are never evaluated: they are clamped into the image so
// that every read stays in bounds.
__device__ __forceinline__ int reflect(int i, int n) {
  i = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
  return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

// The workgroup owns tiles t = g, g + P, g + 2P, ... of kTH x kTW output pixels (plane-major, then tile rows, then tile columns).  A
// tile and its one-pixel halo of both images are staged in LDS (fp32, exact).  Thread (column cx, row group ry) walks its 8 output
// rows: the horizontal 3-tap sums of the five moment images (x, y, x^2, y^2, xy, in fp64) of rows r - 1, r, r + 1 roll through
// registers, the vertical taps combine them into mu1, mu2, f(x^2), f(y^2), f(xy), and the map is evaluated in fp64.  Within a tile a
// thread adds its pixels top to bottom; partials are one {sum, count} per workgroup.
__global__ void __launch_bounds__(kThreads) ssim_kernel(const float* __restrict__ img1, const float* __restrict__ img2, int64_t planes,
                                                        int h, int w, double* __restrict__ part) {
  __shared__ float s1[kStage], s2[kStage];
  const int tid = threadIdx.x, cx = tid % kTW, ry = tid / kTW;
  const int tiles_x = (w + kTW - 1) / kTW, tiles_y = (h + kTH - 1) / kTH;
  const int64_t per_plane = (int64_t)tiles_x * tiles_y, ntiles = planes * per_plane, P = gridDim.x;
  double acc = 0.0, cnt = 0.0;
  for (int64_t t = blockIdx.x; t < ntiles; t += P) {
    const int64_t plane = t / per_plane;
    const int tr = (int)(t % per_plane);
    const int y0 = (tr / tiles_x) * kTH, x0 = (tr % tiles_x) * kTW;
    const float* p1 = img1 + plane * h * (int64_t)w;
    const float* p2 = img2 + plane * h * (int64_t)w;
    // every load of the tile is issued before the first LDS write, so a thread waits for memory once per tile, not once per element
    float va[kStagePer], vb[kStagePer];
#pragma unroll
    for (int k = 0; k < kStagePer; ++k) {
      const int e = tid + k * kThreads;
      if (e < kStage) {
        const int r = e / kSW, c = e % kSW;
        const int64_t off = (int64_t)reflect(y0 - 1 + r, h) * w + reflect(x0 - 1 + c, w);
        va[k] = p1[off], vb[k] = p2[off];
      }
    }
    __syncthreads();  // the previous tile's reads of s1 / s2 are done
#pragma unroll
    for (int k = 0; k < kStagePer; ++k) {
      const int e = tid + k * kThreads;
      if (e < kStage) s1[e] = va[k], s2[e] = vb[k];
    }
    __syncthreads();
    const int x = x0 + cx;
    if (x >= w) continue;
    const int rb = ry * kRows;  // first output row of this thread, tile-relative
    int rn = h - (y0 + rb);
    rn = rn < kRows ? rn : kRows;
    if (rn <= 0) continue;
    // horizontal sums of staged row k (tile-relative output row k - 1): m[0..4] = x, y, x^2, y^2, xy
    auto hrow = [&](int k, double* m) {
      const float* a = s1 + k * kSW + cx;
      const float* b = s2 + k * kSW + cx;
      const double a0 = a[0], a1 = a[1], a2 = a[2], b0 = b[0], b1 = b[1], b2 = b[2];
      m[0] = kG0 * a0 + kG1 * a1 + kG0 * a2;
      m[1] = kG0 * b0 + kG1 * b1 + kG0 * b2;
      m[2] = kG0 * (a0 * a0) + kG1 * (a1 * a1) + kG0 * (a2 * a2);
      m[3] = kG0 * (b0 * b0) + kG1 * (b1 * b1) + kG0 * (b2 * b2);
      m[4] = kG0 * (a0 * b0) + kG1 * (a1 * b1) + kG0 * (a2 * b2);
    };
    double up[5], mid[5], dn[5];
    hrow(rb, up);
    hrow(rb + 1, mid);
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      if (j >= rn) break;
      hrow(rb + j + 2, dn);
      double f[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) f[q] = kG0 * up[q] + kG1 * mid[q] + kG0 * dn[q];
      const double mu1 = f[0], mu2 = f[1];
      const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
      const double sig1 = f[2] - mu1_sq, sig2 = f[3] - mu2_sq, sig12 = f[4] - mu1_mu2;
      acc += ((2.0 * mu1_mu2 + kC1) * (2.0 * sig12 + kC2)) / ((mu1_sq + mu2_sq + kC1) * (sig1 + sig2 + kC2) + kEps);
      cnt += 1.0;
#pragma unroll
      for (int q = 0; q < 5; ++q) up[q] = mid[q], mid[q] = dn[q];
    }
  }
  double v[2] = {acc, cnt};
  block_sum(v);
  if (tid == 0) part[blockIdx.x] = v[0], part[P + blockIdx.x] = v[1];
}

// out[0] = the P partial sums, out[1] = the P partial counts, each by strided_sum, then block_sum's fixed tree.  One workgroup.
__global__ void __launch_bounds__(kThreads) finalize_kernel(const double* __restrict__ part, int P, double* __restrict__ out) {
  double v[2];
  strided_sum(part, P, v);
  block_sum(v);
  if (threadIdx.x == 0) out[0] = v[0], out[1] = v[1];
}

}  // namespace imgm
}  // namespace sr

using namespace sr;
using namespace sr::imgm;

static int check_ssim_shape(const char* fn, int64_t planes, int h, int w) {
  SR_REQUIRE(planes >= 0 && h >= 2 && w >= 2 && h <= kMaxSide && w <= kMaxSide,
             "%s: need planes >= 0 and 2 <= h, w <= %d (reflect padding is undefined below 2; got %lld planes of %d x %d)", fn, kMaxSide,
             (long long)planes, h, w);
  SR_REQUIRE(planes <= ((int64_t)1 << 40) / ((int64_t)h * w), "%s: %lld planes of %d x %d is too large", fn, (long long)planes, h, w);
  return 0;
}

extern "C" int sr_image_metrics_scratch(int64_t n, int64_t planes, int h, int w, int64_t* bytes) {
  SR_REQUIRE(bytes, "sr_image_metrics_scratch: null pointer");
  SR_REQUIRE(n >= 0, "sr_image_metrics_scratch: n must be >= 0 (got %lld)", (long long)n);
  long p = sse_partials(n);
  if (planes > 0) {
    if (check_ssim_shape("sr_image_metrics_scratch", planes, h, w)) return 1;
    const long q = ssim_partials(planes, h, w);
    p = q > p ? q : p;
  }
  *bytes = (int64_t)2 * p * (int64_t)sizeof(double);
  return 0;
}

extern "C" int sr_image_sse(const float* pred, const float* gt, int64_t n, const uint8_t* mask, int64_t mask_div, void* scratch,
                            int64_t scratch_bytes, double* out, void* stream) {
  SR_REQUIRE(out && scratch && (n == 0 || (pred && gt)), "sr_image_sse: null pointer");
  SR_REQUIRE(n >= 0 && n <= ((int64_t)1 << 40), "sr_image_sse: n must be in 0..2^40 (got %lld)", (long long)n);
  SR_REQUIRE(!mask || (mask_div >= 1 && mask_div <= (n > 0 ? n : 1)), "sr_image_sse: mask_div must be in 1..n (got %lld)",
             (long long)mask_div);
  const long P = sse_partials(n);
  if (require_scratch("sr_image_sse", scratch_bytes, 2 * P * (int64_t)sizeof(double))) return 1;
  hipStream_t s = (hipStream_t)stream;
  double* part = static_cast<double*>(scratch);
  const bool vec = ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(gt)) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(sse_kernel<true>, dim3((unsigned)P), dim3(kThreads), 0, s, pred, gt, n, mask, mask_div, part);
  else
    hipLaunchKernelGGL(sse_kernel<false>, dim3((unsigned)P), dim3(kThreads), 0, s, pred, gt, n, mask, mask_div, part);
  if (check_launch("sse_kernel")) return 2;
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(kThreads), 0, s, (const double*)part, (int)P, out);
  return check_launch("finalize_kernel");
}

extern "C" int sr_ssim_sum(const float* img1, const float* img2, int64_t planes, int h, int w, void* scratch, int64_t scratch_bytes,
                           double* out, void* stream) {
  SR_REQUIRE(out && scratch && (planes == 0 || (img1 && img2)), "sr_ssim_sum: null pointer");
  if (check_ssim_shape("sr_ssim_sum", planes, h, w)) return 1;
  const long P = ssim_partials(planes, h, w);
  if (require_scratch("sr_ssim_sum", scratch_bytes, 2 * P * (int64_t)sizeof(double))) return 1;
  hipStream_t s = (hipStream_t)stream;
  double* part = static_cast<double*>(scratch);
  hipLaunchKernelGGL(ssim_kernel, dim3((unsigned)P), dim3(kThreads), 0, s, img1, img2, planes, h, w, part);
  if (check_launch("ssim_kernel")) return 2;
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(kThreads), 0, s, (const double*)part, (int)P, out);
  return check_launch("finalize_kernel");
}
