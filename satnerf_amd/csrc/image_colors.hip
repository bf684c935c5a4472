// A dataset's colours for gfx950: the reference's load_tensor_from_rgb_geotiff (datasets/satellite.py:67-80) from
// the 8-bit image the file holds: v = u8 / 255 and, for img_downscale > 1, torchvision's tensor Resize(BICUBIC) = ATen's
// upsample_bicubic2d (align_corners=False, no antialias, A = -0.75, border taps clamped, output not clamped), written as the
// (out_h * out_w, 3) fp32 rows that sit beside all_rays.
//
// Memory-bound: one thread per output pixel doing the three channels, 12 contiguous bytes stored per lane; the source bytes are read
// through three byte strides, so HWC and CHW images run the same code and give the same bits.  The 256 values u8 / 255 are divided once
// per workgroup into LDS (one per thread), so a tap costs a byte load and a table read.  No fp64, no scratch, no read-back (capturable).
//
// fp32 contraction is off in this file: the source coordinate scale * (dst + 0.5) - 0.5 is defined with a rounded product (its last
// bit picks the taps' weights at widths near 2048), and the weighted sums are rounded products and adds in one fixed order.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace sr {
namespace imgc {

constexpr int kThreads = 256;
constexpr unsigned kGridX = 1u << 22;  // blocks along x; the rest of a larger image goes along y (x * 256 threads stays below 2^32)
constexpr float kA = -0.75f;

// table[b] = (float)b / 255.0f (correctly rounded fp32 division), b = threadIdx.x: the workgroup has exactly 256 threads
__device__ __forceinline__ void fill_table(float* table) {
  table[threadIdx.x] = (float)threadIdx.x / 255.0f;
  __syncthreads();
}

__device__ __forceinline__ int64_t global_index() {
  return ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kThreads + threadIdx.x;
}

// cubic convolution, |x| <= 1 and 1 < |x| < 2
__device__ __forceinline__ float cubic1(float x) { return ((kA + 2.f) * x - (kA + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cubic2(float x) { return ((kA * x - 5.f * kA) * x + 8.f * kA) * x - 4.f * kA; }

// One axis of output index dst: the four clamped tap indices and their weights.  scale = (float)n_in / (float)n_out from the host.
__device__ __forceinline__ void axis_taps(int dst, float scale, int n_in, int idx[4], float w[4]) {
  const float src = scale * ((float)dst + 0.5f) - 0.5f;  // rounded product, then rounded difference (contraction is off)
  const float fl = floorf(src);
  const float t = src - fl;
  const int i0 = (int)fl;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = i0 - 1 + k;
    idx[k] = i < 0 ? 0 : (i > n_in - 1 ? n_in - 1 : i);
  }
  w[0] = cubic2(t + 1.f), w[1] = cubic1(t), w[2] = cubic1(1.f - t), w[3] = cubic2(2.f - t);
}

// Output pixel p = r * out_w + c: per channel, the four row sums ((w0 v0 + w1 v1) + w2 v2) + w3 v3 over the column taps, then the same
// sum of those over the row taps.
__global__ void __launch_bounds__(kThreads) resize_kernel(const uint8_t* __restrict__ src, int src_h, int src_w, int64_t row_stride,
                                                          int64_t pix_stride, int64_t chan_stride, int out_w, int64_t n, float scale_h,
                                                          float scale_w, float* __restrict__ out) {
  __shared__ float table[256];
  fill_table(table);
  const int64_t p = global_index();
  if (p >= n) return;
  int r, c;
  if (n <= 0xffffffffll) {  // uniform over the launch: a 32-bit division where the index fits
    r = (int)((uint32_t)p / (uint32_t)out_w), c = (int)((uint32_t)p % (uint32_t)out_w);
  } else {
    r = (int)(p / out_w), c = (int)(p % out_w);
  }
  int iy[4], ix[4];
  float wy[4], wx[4];
  axis_taps(r, scale_h, src_h, iy, wy);
  axis_taps(c, scale_w, src_w, ix, wx);
  int64_t col[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) col[k] = ix[k] * pix_stride;
  float acc[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const uint8_t* plane = src + ch * chan_stride;
    float rows[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint8_t* line = plane + iy[j] * row_stride;
      const float v0 = table[line[col[0]]], v1 = table[line[col[1]]], v2 = table[line[col[2]]], v3 = table[line[col[3]]];
      rows[j] = ((wx[0] * v0 + wx[1] * v1) + wx[2] * v2) + wx[3] * v3;
    }
    acc[ch] = ((wy[0] * rows[0] + wy[1] * rows[1]) + wy[2] * rows[2]) + wy[3] * rows[3];
  }
  float* o = out + 3 * p;
  o[0] = acc[0], o[1] = acc[1], o[2] = acc[2];
}

// The plain conversion of an image in any layout: thread p converts pixel p's three bytes.
__global__ void __launch_bounds__(kThreads) convert_pixels_kernel(const uint8_t* __restrict__ src, int src_w, int64_t row_stride,
                                                                  int64_t pix_stride, int64_t chan_stride, int64_t n,
                                                                  float* __restrict__ out) {
  __shared__ float table[256];
  fill_table(table);
  const int64_t p = global_index();
  if (p >= n) return;
  int64_t r, c;
  if (n <= 0xffffffffll) {
    r = (uint32_t)p / (uint32_t)src_w, c = (uint32_t)p % (uint32_t)src_w;
  } else {
    r = p / src_w, c = p % src_w;
  }
  const uint8_t* s = src + r * row_stride + c * pix_stride;
  float* o = out + 3 * p;
  o[0] = table[s[0]], o[1] = table[s[chan_stride]], o[2] = table[s[2 * chan_stride]];
}

// The plain conversion of a dense HWC image: byte e becomes float e, four per thread.  VEC (src 4-byte and out 16-byte aligned) reads
// a dword and stores a float4; the scalar form moves the same elements, so the result does not depend on alignment.
template <bool VEC>
__global__ void __launch_bounds__(kThreads) convert_flat_kernel(const uint8_t* __restrict__ src, int64_t n, float* __restrict__ out) {
  __shared__ float table[256];
  fill_table(table);
  const int64_t q = global_index(), e0 = 4 * q;
  if (e0 >= n) return;
  if (VEC && e0 + 4 <= n) {
    const uint32_t u = reinterpret_cast<const uint32_t*>(src)[q];
    reinterpret_cast<float4*>(out)[q] = make_float4(table[u & 255u], table[(u >> 8) & 255u], table[(u >> 16) & 255u], table[u >> 24]);
  } else {
    for (int k = 0; k < 4 && e0 + k < n; ++k) out[e0 + k] = table[src[e0 + k]];
  }
}

// (blocks along x, blocks along y) for `threads` threads; false when the image is beyond what one launch holds
inline bool grid_for(int64_t threads, dim3* grid) {
  const int64_t blocks = (threads + kThreads - 1) / kThreads;
  const int64_t gx = blocks < (int64_t)kGridX ? blocks : (int64_t)kGridX, gy = (blocks + gx - 1) / gx;
  if (gy > 65535) return false;
  *grid = dim3((unsigned)gx, (unsigned)gy);
  return true;
}

}  // namespace imgc
}  // namespace sr

using namespace sr;
using namespace sr::imgc;

extern "C" int sr_image_colors(const uint8_t* src, int src_h, int src_w, int64_t row_stride, int64_t pix_stride, int64_t chan_stride, int out_h,
                               int out_w, float* out, void* stream) {
  SR_REQUIRE(src_h >= 1 && src_w >= 1, "sr_image_colors: the source must be at least 1 x 1 (got %d x %d)", src_h, src_w);
  SR_REQUIRE(out_h >= 0 && out_w >= 0, "sr_image_colors: the output size must be >= 0 (got %d x %d)", out_h, out_w);
  SR_REQUIRE(row_stride >= 1 && pix_stride >= 1 && chan_stride >= 1,
             "sr_image_colors: strides must be positive byte counts (got row %lld, pixel %lld, channel %lld)", (long long)row_stride,
             (long long)pix_stride, (long long)chan_stride);
  const int64_t n = (int64_t)out_h * out_w;
  if (n == 0) return 0;
  SR_REQUIRE(src && out, "sr_image_colors: null pointer");
  hipStream_t s = (hipStream_t)stream;
  dim3 grid;
  if (out_h == src_h && out_w == src_w) {
    if (pix_stride == 3 && chan_stride == 1 && row_stride == 3 * (int64_t)src_w) {
      SR_REQUIRE(grid_for((3 * n + 3) / 4, &grid), "sr_image_colors: %d x %d is too large", out_h, out_w);
      const bool vec = (reinterpret_cast<uintptr_t>(src) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
      if (vec)
        hipLaunchKernelGGL(convert_flat_kernel<true>, grid, dim3(kThreads), 0, s, src, 3 * n, out);
      else
        hipLaunchKernelGGL(convert_flat_kernel<false>, grid, dim3(kThreads), 0, s, src, 3 * n, out);
      return check_launch("convert_flat_kernel");
    }
    SR_REQUIRE(grid_for(n, &grid), "sr_image_colors: %d x %d is too large", out_h, out_w);
    hipLaunchKernelGGL(convert_pixels_kernel, grid, dim3(kThreads), 0, s, src, src_w, row_stride, pix_stride, chan_stride, n, out);
    return check_launch("convert_pixels_kernel");
  }
  SR_REQUIRE(grid_for(n, &grid), "sr_image_colors: %d x %d is too large", out_h, out_w);
  const float scale_h = (float)src_h / (float)out_h, scale_w = (float)src_w / (float)out_w;
  hipLaunchKernelGGL(resize_kernel, grid, dim3(kThreads), 0, s, src, src_h, src_w, row_stride, pix_stride, chan_stride, out_w, n, scale_h,
                     scale_w, out);
  return check_launch("resize_kernel");
}
