// Evaluation image products for gfx950: what the reference does to rendered images after the render.
//   sr_nearest_fill  quickly_interpolate_nans_from_singlechannel_img (study_solar_interpolation.py:53-68) = scipy's
//                    griddata(method="nearest"), with the ties scipy leaves to its KD-tree decided by (row, column)
//   sr_colorize      train_utils.visualize_depth (train_utils.py:59-72) and the body of hstack_dsm_tifs_v1
//                    (study_solar_interpolation.py:85-93) after the fill: range, normalise, truncate to a byte, look the colour up
//   sr_unit_to_u8    hstack_sun_tifs / hstack_rgb_tifs (study_solar_interpolation.py:23-51): (img * 255).astype(uint8) into a strip
// Every image is read through element strides, so a column of the (N, 13) image buffer or a crop window is read in place.
//
// The fill is separable and works in integers only.  column_nearest_kernel finds, for every pixel, the nearest valid row of its own
// column (ties to the upper row) from a bit mask of the column held in LDS; row_nearest_kernel then minimises the packed key
// (d^2 << 26 | r' << 13 | c') over the columns of the pixel's row, walking outwards from its own column over the row's candidates in
// LDS and stopping once dx^2 exceeds the best d^2 -- every column further out is strictly worse.  Within one column the candidate with
// the smallest (dy^2, r') is the column pass's answer, so the minimum over columns is the minimum of (d^2, r', c') over the image.
//
// fp32 contraction is off in this file: q = (x - mi) / d and y = 255 q are one rounded operation each, as numpy evaluates them.
#include <float.h>

#include "block_device.h"
#include "common.h"

#pragma clang fp contract(off)

namespace sr {
namespace imgp {

constexpr int kThreads = 256;
constexpr int kMaxSide = 8192;      // the fill's sides: 13 bits of row and of column in the key, one row of candidates in 16 KiB of LDS
constexpr int kColTile = 32;        // columns per workgroup of the column pass; the other 8 = kThreads / kColTile threads split the rows
constexpr int kMaxWords = kMaxSide / 32;
constexpr int kRowSpan = 1024;      // pixels of one row per workgroup of the row pass
constexpr int kRangeBlocks = 1024;  // most workgroups of the range reduction (grid-strided beyond)
constexpr int kMaxColorSide = 65535;

__device__ __forceinline__ bool is_nan_bits(uint32_t u) { return (u & 0x7fffffffu) > 0x7f800000u; }

// near[r * w + c] = the valid row of column c nearest to r, the upper one of two at the same distance; -1 for a column without any
__global__ void __launch_bounds__(kThreads) column_nearest_kernel(const uint32_t* __restrict__ img, int h, int w, int64_t row_stride,
                                                                  int64_t col_stride, int16_t* __restrict__ near) {
  __shared__ uint32_t bits[kMaxWords * kColTile];  // [word][column]: bit b of word k = row 32 k + b is valid
  const int col = threadIdx.x % kColTile, g = threadIdx.x / kColTile;
  const int c = blockIdx.x * kColTile + col;
  const int words = (h + 31) >> 5;
  for (int k = g; k < words; k += kThreads / kColTile) {
    uint32_t m = 0;
    if (c < w) {
      const uint32_t* p = img + (int64_t)k * 32 * row_stride + c * col_stride;
      const int nb = h - k * 32 < 32 ? h - k * 32 : 32;
#pragma unroll 8
      for (int b = 0; b < nb; ++b) m |= (uint32_t)!is_nan_bits(p[b * row_stride]) << b;
    }
    bits[k * kColTile + col] = m;
  }
  __syncthreads();
  if (c >= w) return;
  for (int k = g; k < words; k += kThreads / kColTile) {
    const uint32_t m = bits[k * kColTile + col];
    int up = -1, down = -1;  // the nearest valid rows outside this word
    for (int j = k - 1; j >= 0; --j) {
      const uint32_t q = bits[j * kColTile + col];
      if (q) {
        up = j * 32 + 31 - __clz(q);
        break;
      }
    }
    for (int j = k + 1; j < words; ++j) {
      const uint32_t q = bits[j * kColTile + col];
      if (q) {
        down = j * 32 + __ffs(q) - 1;
        break;
      }
    }
    const int nb = h - k * 32 < 32 ? h - k * 32 : 32;
    for (int b = 0; b < nb; ++b) {
      const int r = k * 32 + b;
      const uint32_t lo = m & (0xffffffffu >> (31 - b)), hi = m & (0xffffffffu << b);  // the word's valid rows <= r and >= r
      const int u = lo ? k * 32 + 31 - __clz(lo) : up;
      const int d = hi ? k * 32 + __ffs(hi) - 1 : down;
      const int n = u < 0 ? d : (d < 0 ? u : (r - u <= d - r ? u : d));
      near[(int64_t)r * w + c] = (int16_t)n;
    }
  }
}

// Workgroup (x, r) fills pixels [x kRowSpan, (x + 1) kRowSpan) of row r from the whole row of candidates.
__global__ void __launch_bounds__(kThreads) row_nearest_kernel(const uint32_t* __restrict__ img, int w, int64_t row_stride,
                                                               int64_t col_stride, const int16_t* __restrict__ near,
                                                               uint32_t* __restrict__ out, int32_t* __restrict__ index) {
  __shared__ int16_t cand[kMaxSide];
  const int r = blockIdx.y;
  const int16_t* row = near + (int64_t)r * w;
  for (int c = threadIdx.x; c < w; c += kThreads) cand[c] = row[c];
  __syncthreads();
  const int c0 = blockIdx.x * kRowSpan, c1 = c0 + kRowSpan < w ? c0 + kRowSpan : w;
  for (int c = c0 + threadIdx.x; c < c1; c += kThreads) {
    unsigned long long best = ~0ull;
    for (int dx = 0;; ++dx) {
      const int l = c - dx, rr = c + dx;
      if (l < 0 && rr >= w) break;
      const unsigned long long dx2 = (unsigned long long)dx * dx;
      if (dx2 > (best >> 26)) break;
      if (l >= 0) {
        const int n = cand[l];
        if (n >= 0) {
          const unsigned long long dy = (unsigned long long)(r > n ? r - n : n - r);
          const unsigned long long key = ((dy * dy + dx2) << 26) | ((unsigned long long)n << 13) | (unsigned long long)l;
          best = key < best ? key : best;
        }
      }
      if (dx > 0 && rr < w) {
        const int n = cand[rr];
        if (n >= 0) {
          const unsigned long long dy = (unsigned long long)(r > n ? r - n : n - r);
          const unsigned long long key = ((dy * dy + dx2) << 26) | ((unsigned long long)n << 13) | (unsigned long long)rr;
          best = key < best ? key : best;
        }
      }
    }
    const int64_t o = (int64_t)r * w + c;
    if (best == ~0ull) {  // no valid pixel anywhere: the pixel keeps its own NaN
      out[o] = img[r * row_stride + c * col_stride];
      if (index) index[o] = -1;
    } else {
      const int rs = (int)((best >> 13) & 8191u), cs = (int)(best & 8191u);
      out[o] = img[rs * row_stride + cs * col_stride];
      if (index) index[o] = rs * w + cs;
    }
  }
}

// ---- colouring ---------------------------------------------------------------------------------------------------------------------
// np.nan_to_num's replacements (policy 1): NaN -> 0, +-inf -> +-FLT_MAX; policy 0 keeps the value
__device__ __forceinline__ float replace_nonfinite(float x, int nan_to_zero) {
  if (!nan_to_zero) return x;
  if (x != x) return 0.0f;
  if (x == INFINITY) return FLT_MAX;
  if (x == -INFINITY) return -FLT_MAX;
  return x;
}

__global__ void range_init_kernel(unsigned* keys) { keys[0] = kKeyPosInf, keys[1] = kKeyNegInf; }

// keys = {order_key(min), order_key(max)} over the window after the replacement; a NaN (policy 0 only) touches neither.  Integer
// atomics on keys: no arrival order can change the result.
__global__ void __launch_bounds__(kThreads) range_kernel(const float* __restrict__ img, int cols, int64_t n, int64_t row_stride,
                                                         int64_t col_stride, int nan_to_zero, unsigned* __restrict__ keys) {
  unsigned k[2] = {kKeyPosInf, kKeyNegInf};
  for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < n; p += (int64_t)gridDim.x * kThreads) {
    const int64_t r = p / cols, c = p - r * cols;
    const float x = replace_nonfinite(img[r * row_stride + c * col_stride], nan_to_zero);
    if (x == x) {
      const unsigned kx = order_key(x);
      k[0] = kx < k[0] ? kx : k[0];
      k[1] = kx > k[1] ? kx : k[1];
    }
  }
  wave_minmax(k);
  if ((threadIdx.x & 63) == 0) {
    // a stored key only moves towards its extreme, so a wave that does not beat the value it reads (however stale) skips its atomic
    if (k[0] < __hip_atomic_load(keys + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(keys + 0, k[0]);
    if (k[1] > __hip_atomic_load(keys + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(keys + 1, k[1]);
  }
}

// One thread per window pixel.  bounds bit 0: mi = vmin, bit 1: ma = vmax; the other bound is read from keys.
__global__ void __launch_bounds__(kThreads) colorize_kernel(const float* __restrict__ img, int cols, int64_t n, int64_t row_stride,
                                                            int64_t col_stride, int nan_to_zero, int bounds, float vmin, float vmax,
                                                            float denom, const unsigned* __restrict__ keys,
                                                            const uint8_t* __restrict__ lut, uint8_t* __restrict__ index_out,
                                                            uint8_t* __restrict__ strip, int64_t strip_cols, int64_t strip_col0,
                                                            float* __restrict__ chw) {
  __shared__ float unit[256];     // (float)b / 255.0f, as sr_image_colors
  __shared__ uint8_t colors[768];
  unit[threadIdx.x] = (float)threadIdx.x / 255.0f;
  if (lut)
    for (int k = threadIdx.x; k < 768; k += kThreads) colors[k] = lut[k];
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= n) return;
  const float mi = (bounds & 1) ? vmin : from_key(keys[0]);
  const float ma = (bounds & 2) ? vmax : from_key(keys[1]);
  const float d = bounds == 3 ? denom : (ma - mi) + 1e-8f;
  const int64_t r = p / cols, c = p - r * cols;
  float x = replace_nonfinite(img[r * row_stride + c * col_stride], nan_to_zero);
  if (bounds) {  // np.clip: a NaN stays a NaN
    x = x < mi ? mi : x;
    x = x > ma ? ma : x;
  }
  const float q = (x - mi) / d;
  const float y = 255.0f * q;
  const int i = y >= 255.0f ? (y == INFINITY ? 0 : 255) : (y >= 0.0f ? (int)y : 0);  // NaN and +-inf give 0
  if (index_out) index_out[p] = (uint8_t)i;
  if (strip) {
    uint8_t* o = strip + (r * strip_cols + strip_col0 + c) * 3;
    o[0] = colors[3 * i], o[1] = colors[3 * i + 1], o[2] = colors[3 * i + 2];
  }
  if (chw) chw[p] = unit[colors[3 * i]], chw[n + p] = unit[colors[3 * i + 1]], chw[2 * n + p] = unit[colors[3 * i + 2]];
}

// One thread per window pixel and channel: byte = trunc(x * 255.0f), clamped to 0..255, NaN -> 0
__global__ void __launch_bounds__(kThreads) unit_to_u8_kernel(const float* __restrict__ img, int cols, int channels, int64_t n,
                                                              int64_t row_stride, int64_t col_stride, int64_t chan_stride,
                                                              uint8_t* __restrict__ strip, int64_t strip_cols, int64_t strip_col0) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= n) return;
  const int64_t p = e / channels, k = e - p * channels;
  const int64_t r = p / cols, c = p - r * cols;
  const float y = img[r * row_stride + c * col_stride + k * chan_stride] * 255.0f;
  const int b = y >= 255.0f ? 255 : (y >= 0.0f ? (int)y : 0);
  strip[(r * strip_cols + strip_col0 + c) * channels + k] = (uint8_t)b;
}

inline int check_window(const char* fn, int rows, int cols, int64_t row_stride, int64_t col_stride) {
  SR_REQUIRE(rows >= 0 && cols >= 0 && rows <= kMaxColorSide && cols <= kMaxColorSide, "%s: the window must be 0..%d on each side (got %d x %d)",
             fn, kMaxColorSide, rows, cols);
  SR_REQUIRE(row_stride >= 1 && col_stride >= 1, "%s: strides must be positive element counts (got row %lld, column %lld)", fn,
             (long long)row_stride, (long long)col_stride);
  return 0;
}

inline int check_strip(const char* fn, int cols, int64_t strip_cols, int64_t strip_col0) {
  SR_REQUIRE(strip_col0 >= 0 && strip_col0 + cols <= strip_cols, "%s: columns %lld..%lld do not fit a strip of %lld columns", fn,
             (long long)strip_col0, (long long)(strip_col0 + cols), (long long)strip_cols);
  return 0;
}

}  // namespace imgp
}  // namespace sr

using namespace sr;
using namespace sr::imgp;

extern "C" int sr_nearest_fill_scratch(int h, int w, int64_t* bytes) {
  SR_REQUIRE(bytes, "sr_nearest_fill_scratch: null pointer");
  SR_REQUIRE(h >= 0 && w >= 0 && h <= kMaxSide && w <= kMaxSide, "sr_nearest_fill_scratch: sides must be in 0..%d (got %d x %d)", kMaxSide, h, w);
  ScratchCarver sc(nullptr);
  sc.take<int16_t>((int64_t)h * w, 16);
  *bytes = sc.bytes();
  return 0;
}

extern "C" int sr_nearest_fill(const float* image, int h, int w, int64_t row_stride, int64_t col_stride, void* scratch, int64_t scratch_bytes,
                               float* out, int32_t* index, void* stream) {
  SR_REQUIRE(h >= 0 && w >= 0 && h <= kMaxSide && w <= kMaxSide, "sr_nearest_fill: sides must be in 0..%d (got %d x %d)", kMaxSide, h, w);
  SR_REQUIRE(row_stride >= 1 && col_stride >= 1, "sr_nearest_fill: strides must be positive element counts (got row %lld, column %lld)",
             (long long)row_stride, (long long)col_stride);
  if ((int64_t)h * w == 0) return 0;
  SR_REQUIRE(image && out && scratch, "sr_nearest_fill: null pointer");
  SR_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 1) == 0, "sr_nearest_fill: scratch must be 2-byte aligned");
  ScratchCarver sc(scratch);
  int16_t* near = sc.take<int16_t>((int64_t)h * w, 16);
  if (require_scratch("sr_nearest_fill", scratch_bytes, sc.bytes())) return 1;
  hipStream_t s = (hipStream_t)stream;
  const uint32_t* bits = reinterpret_cast<const uint32_t*>(image);
  hipLaunchKernelGGL(column_nearest_kernel, dim3((w + kColTile - 1) / kColTile), dim3(kThreads), 0, s, bits, h, w, row_stride, col_stride, near);
  if (check_launch("column_nearest_kernel")) return 2;
  hipLaunchKernelGGL(row_nearest_kernel, dim3((w + kRowSpan - 1) / kRowSpan, h), dim3(kThreads), 0, s, bits, w, row_stride, col_stride, near,
                     reinterpret_cast<uint32_t*>(out), index);
  return check_launch("row_nearest_kernel");
}

extern "C" int sr_colorize_scratch(int bounds, int64_t* bytes) {
  SR_REQUIRE(bytes, "sr_colorize_scratch: null pointer");
  SR_REQUIRE(bounds >= 0 && bounds <= 3, "sr_colorize_scratch: bounds must be 0..3 (got %d)", bounds);
  *bytes = bounds == 3 ? 0 : 2 * (int64_t)sizeof(unsigned);
  return 0;
}

extern "C" int sr_colorize(const float* image, int rows, int cols, int64_t row_stride, int64_t col_stride, int nan_to_zero, int bounds,
                           float vmin, float vmax, float denom, const uint8_t* lut, uint8_t* index_out, uint8_t* strip, int64_t strip_cols,
                           int64_t strip_col0, float* chw, void* scratch, int64_t scratch_bytes, void* stream) {
  if (check_window("sr_colorize", rows, cols, row_stride, col_stride)) return 1;
  SR_REQUIRE(nan_to_zero == 0 || nan_to_zero == 1, "sr_colorize: nan_to_zero must be 0 or 1 (got %d)", nan_to_zero);
  SR_REQUIRE(bounds >= 0 && bounds <= 3, "sr_colorize: bounds must be 0..3 (got %d)", bounds);
  SR_REQUIRE(!(bounds & 1) || vmin == vmin, "sr_colorize: vmin is NaN");
  SR_REQUIRE(!(bounds & 2) || vmax == vmax, "sr_colorize: vmax is NaN");
  SR_REQUIRE(bounds != 3 || denom == denom, "sr_colorize: denom is NaN");
  SR_REQUIRE(index_out || strip || chw, "sr_colorize: no output requested");
  SR_REQUIRE(lut || !(strip || chw), "sr_colorize: a coloured output needs a lut");
  if (strip && check_strip("sr_colorize", cols, strip_cols, strip_col0)) return 1;
  const int64_t n = (int64_t)rows * cols;
  if (n == 0) return 0;
  SR_REQUIRE(image, "sr_colorize: null pointer");
  unsigned* keys = nullptr;
  if (bounds != 3) {
    SR_REQUIRE(scratch && (reinterpret_cast<uintptr_t>(scratch) & 3) == 0, "sr_colorize: scratch must be a 4-byte aligned pointer");
    if (require_scratch("sr_colorize", scratch_bytes, 2 * (int64_t)sizeof(unsigned))) return 1;
    keys = static_cast<unsigned*>(scratch);
  }
  hipStream_t s = (hipStream_t)stream;
  if (keys) {
    hipLaunchKernelGGL(range_init_kernel, dim3(1), dim3(1), 0, s, keys);
    if (check_launch("range_init_kernel")) return 2;
    hipLaunchKernelGGL(range_kernel, dim3(partial_slots(n, kThreads, kRangeBlocks)), dim3(kThreads), 0, s, image, cols, n, row_stride, col_stride,
                       nan_to_zero, keys);
    if (check_launch("range_kernel")) return 2;
  }
  hipLaunchKernelGGL(colorize_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, image, cols, n, row_stride, col_stride, nan_to_zero, bounds, vmin,
                     vmax, denom, keys, lut, index_out, strip, strip_cols, strip_col0, chw);
  return check_launch("colorize_kernel");
}

extern "C" int sr_unit_to_u8(const float* image, int rows, int cols, int channels, int64_t row_stride, int64_t col_stride, int64_t chan_stride,
                             uint8_t* strip, int64_t strip_cols, int64_t strip_col0, void* stream) {
  if (check_window("sr_unit_to_u8", rows, cols, row_stride, col_stride)) return 1;
  SR_REQUIRE(channels == 1 || channels == 3, "sr_unit_to_u8: channels must be 1 or 3 (got %d)", channels);
  SR_REQUIRE(chan_stride >= 1, "sr_unit_to_u8: the channel stride must be a positive element count (got %lld)", (long long)chan_stride);
  if (check_strip("sr_unit_to_u8", cols, strip_cols, strip_col0)) return 1;
  const int64_t n = (int64_t)rows * cols * channels;
  if (n == 0) return 0;
  SR_REQUIRE(image && strip, "sr_unit_to_u8: null pointer");
  hipLaunchKernelGGL(unit_to_u8_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream, image, cols, channels, n, row_stride,
                     col_stride, chan_stride, strip, strip_cols, strip_col0);
  return check_launch("unit_to_u8_kernel");
}
