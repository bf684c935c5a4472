// A Blender scene's colours and rays for gfx950: what the reference's BlenderDataset (datasets/blender.py:12-209)
// computes per frame after the PNG is decoded.
//
// sr_blender_colors: Pillow's 8-bit Image.resize(LANCZOS) of one RGBA image -- integer arithmetic, so the bytes are Pillow's exactly --
// and the reference's ToTensor + blend onto white.  Two launches, horizontal then vertical, with the (src_h, out_w) premultiplied
// intermediate in caller-owned scratch; a pass whose size does not change is skipped, and the last pass that runs un-premultiplies and
// writes the outputs.  A pixel is one packed dword (R in the low byte): one lane per output pixel, a wave = 64 adjacent columns of one
// row of the image the pass writes, so the vertical pass' loads and every store are contiguous across the wave.  The row is
// wave-uniform (readfirstlane), so the vertical pass reads its coefficients and bounds through the scalar cache; the horizontal pass
// reads, per lane, ksize contiguous ints of its table (20 KB at 800 -> 400: 400 x 13 ints).  Neighbouring outputs share all but
// `scale` of their 6 * scale taps: the re-reads are served by the L1 (a wave's footprint is 64 * scale source pixels and 64 * ksize
// coefficients), which is why nothing is staged in LDS -- both launches are bound by launch latency at the workload's 800 x 800 ->
// 400 x 400 (section 7.8).
// The bounds of an output index are recomputed in the kernel from (n_in, n_out) in fp64 -- products, sums and a truncation, which IEEE
// arithmetic gives identically on the host and the device -- so no bounds table exists that could point outside the source.
//
// sr_blender_perturb: add_perturbation (datasets/blender.py:61-79) on the decoded bytes, in front of sr_blender_colors: a per-band byte
// table ("color": every band is a function of its own byte, built in fp64 on the host) and up to 16 filled rectangles ("occ").  One
// launch, 8 bytes of traffic per pixel; the table and the rectangles travel by value in the kernel arguments, so nothing is uploaded
// and nothing waits.  The table is staged in LDS as 256 packed dwords (one ds_read_b32 per band, each keeping its own byte); the
// rectangles are read at a uniform index, i.e. through the scalar cache.
//
// sr_pinhole_rays: get_ray_directions + get_rays + the near / far columns; fp64 per pixel from the fp32 inputs, one rounding per
// direction component, 32 contiguous bytes stored per lane.
//
// Contraction is off in this file: the fp32 blend and the fp64 ray chain are defined with every product and sum rounded.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace sr {
namespace blender {

constexpr int kLanes = 64, kRows = 4;  // a workgroup: 4 waves, each 64 adjacent columns of one row
constexpr int kBits = 22;              // Pillow's PRECISION_BITS for 8-bit data
constexpr int kMaxSide = 65536;        // every side; rows / kRows must fit gridDim.y
constexpr int kRayThreads = 256;

struct Axis {
  double scale, support;  // n_in / n_out and 3 max(scale, 1)
  const int32_t* coef;    // DEVICE (n_out, ksize)
  int n_in, ksize;
};

struct Source {
  const uint8_t* p;
  int64_t row_stride, pix_stride, chan_stride;
};

// ksize of the definition, in the host's fp64
inline int lanczos_ksize(int n_in, int n_out) {
  const double scale = (double)n_in / (double)n_out, fs = scale < 1.0 ? 1.0 : scale;
  return 2 * (int)ceil(3.0 * fs) + 1;
}

// [first, first + count) of output index i, clamped so that whatever the arguments no tap leaves the source or the table row
__device__ __forceinline__ void axis_bounds(const Axis& a, int i, int* first, int* count) {
  const double center = ((double)i + 0.5) * a.scale;
  int lo = (int)(center - a.support + 0.5), hi = (int)(center + a.support + 0.5);
  lo = lo < 0 ? 0 : (lo > a.n_in ? a.n_in : lo);
  hi = hi > a.n_in ? a.n_in : hi;
  int n = hi - lo;
  n = n < 0 ? 0 : (n > a.ksize ? a.ksize : n);
  *first = lo, *count = n;
}

template <bool PACKED>
__device__ __forceinline__ uint32_t load_pixel(const Source& s, int64_t r, int64_t c) {
  const uint8_t* q = s.p + r * s.row_stride + c * s.pix_stride;
  if (PACKED) return *reinterpret_cast<const uint32_t*>(q);
  return (uint32_t)q[0] | ((uint32_t)q[s.chan_stride] << 8) | ((uint32_t)q[2 * s.chan_stride] << 16) | ((uint32_t)q[3 * s.chan_stride] << 24);
}

// c' = MULDIV255(c, a) on the three colour bytes
__device__ __forceinline__ uint32_t premultiply(uint32_t u) {
  const uint32_t a = u >> 24;
  uint32_t out = u & 0xff000000u;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t t = ((u >> (8 * k)) & 255u) * a + 128u;
    out |= (((t >> 8) + t) >> 8) << (8 * k);
  }
  return out;
}

__device__ __forceinline__ uint32_t unpremultiply(uint32_t u) {
  const uint32_t a = u >> 24;
  if (a == 0 || a == 255) return u;
  uint32_t out = u & 0xff000000u;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t q = 255u * ((u >> (8 * k)) & 255u) / a;
    out |= (q > 255u ? 255u : q) << (8 * k);
  }
  return out;
}

// clamp(acc >> 22, 0, 255), with the clamp applied before the shift (the same value: the shift is monotonic).  Written as shift-then-
// clamp, hipcc (ROCm 7) fuses two bands into v_ashr_pk_u8_i32 and takes the upper 16 bits of its result for zero; on gfx950 they are
// not, and stray bits were OR-ed into bands 2 and 3 of the packed pixel (tests/test_hip_blender.py holds every byte to Pillow's).
__device__ __forceinline__ uint32_t clip8(int acc) {
  const int v = acc < 0 ? 0 : (acc > (256 << kBits) - 1 ? (256 << kBits) - 1 : acc);
  return (uint32_t)v >> kBits;
}

struct Outputs {
  float* rgbs;          // (n, 3)
  uint8_t* valid_mask;  // (n) or NULL
  uint32_t* rgba;       // (n) packed or NULL
};

// ToTensor and the blend onto white of pixel p: v = u8 / 255, out = v_c v_a + (1 - v_a), every operation rounded
__device__ __forceinline__ void finish(const Outputs& o, int64_t p, uint32_t u) {
  const float a = (float)(u >> 24) / 255.0f, rest = 1.0f - a;
  float* q = o.rgbs + 3 * p;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float v = (float)((u >> (8 * k)) & 255u) / 255.0f;
    q[k] = v * a + rest;
  }
  if (o.valid_mask) o.valid_mask[p] = (u >> 24) != 0;
  if (o.rgba) o.rgba[p] = u;
}

// One resampling pass.  Output pixel (r, c) of an (n_rows, n_cols) image; VERT: taps (first + t, c), coefficients of row r (wave-
// uniform); else taps (r, first + t), coefficients of column c.  premul: the source holds straight RGBA (the first pass that runs);
// last: un-premultiply and write the outputs, else store the packed pixel to `mid`.
template <bool VERT, bool PACKED>
__global__ void __launch_bounds__(kLanes* kRows) resample_kernel(Source src, Axis axis, int n_rows, int n_cols, int premul, int last,
                                                                  uint32_t* __restrict__ mid, Outputs out) {
  const int c = blockIdx.x * kLanes + threadIdx.x;
  const int r = __builtin_amdgcn_readfirstlane(blockIdx.y * kRows + threadIdx.y);
  if (r >= n_rows || c >= n_cols) return;
  int first, count;
  axis_bounds(axis, VERT ? r : c, &first, &count);
  const int32_t* k = axis.coef + (int64_t)(VERT ? r : c) * axis.ksize;
  int acc[4] = {1 << (kBits - 1), 1 << (kBits - 1), 1 << (kBits - 1), 1 << (kBits - 1)};
  for (int t = 0; t < count; ++t) {
    uint32_t u = VERT ? load_pixel<PACKED>(src, first + t, c) : load_pixel<PACKED>(src, r, first + t);
    if (premul) u = premultiply(u);
    const int w = k[t];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] += (int)((u >> (8 * b)) & 255u) * w;
  }
  const uint32_t u = clip8(acc[0]) | (clip8(acc[1]) << 8) | (clip8(acc[2]) << 16) | (clip8(acc[3]) << 24);
  const int64_t p = (int64_t)r * n_cols + c;
  if (last)
    finish(out, p, unpremultiply(u));
  else
    mid[p] = u;
}

// Both passes skipped: the source's own bytes, as Pillow's copy
template <bool PACKED>
__global__ void __launch_bounds__(kLanes* kRows) convert_kernel(Source src, int n_rows, int n_cols, Outputs out) {
  const int c = blockIdx.x * kLanes + threadIdx.x, r = blockIdx.y * kRows + threadIdx.y;
  if (r >= n_rows || c >= n_cols) return;
  finish(out, (int64_t)r * n_cols + c, load_pixel<PACKED>(src, r, c));
}

inline dim3 grid_for(int n_rows, int n_cols) { return dim3(blocks_for(n_cols, kLanes), blocks_for(n_rows, kRows)); }

constexpr int kMaxRects = 16;
constexpr int kPerturbRows = 16;  // rows of one workgroup of perturb_kernel: kRows lanes-rows, 4 pixels each

// Everything perturb_kernel needs besides the image, by value in the kernel arguments (1.4 KB of the 4 KB a launch may carry)
struct Perturb {
  uint32_t lut[256];  // entry v: byte k = what band k's byte v becomes
  int32_t rects[kMaxRects][4];  // x0, y0, x1, y1, inclusive
  uint32_t fills[kMaxRects];    // packed, R in the low byte
  int n_rects, has_lut;
};

template <bool PACKED>
__device__ __forceinline__ void store_pixel(uint8_t* p, int64_t chan_stride, uint32_t u) {
  if (PACKED) {
    *reinterpret_cast<uint32_t*>(p) = u;
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) p[k * chan_stride] = (uint8_t)(u >> (8 * k));
}

// One pass: read a pixel, look its four bytes up, test the rectangles in order (the last that holds the pixel wins), write it.  A
// workgroup is 64 columns x 16 rows, four rows per lane, so the table is staged once per 1,024 pixels.  A pixel is read and written
// by the same lane and by no other, so dst may be src.
template <bool PACKED>
__global__ void __launch_bounds__(kLanes* kRows) perturb_kernel(Source src, uint8_t* __restrict__ dst, int n_rows, int n_cols, Perturb p) {
  __shared__ uint32_t lut[256];
  if (p.has_lut) {  // uniform over the launch
    const int t = threadIdx.y * kLanes + threadIdx.x;
    lut[t] = p.lut[t];
    __syncthreads();
  }
  const int c = blockIdx.x * kLanes + threadIdx.x;
  if (c >= n_cols) return;
  constexpr int kPer = kPerturbRows / kRows;
  const int r0 = __builtin_amdgcn_readfirstlane(blockIdx.y * kPerturbRows + threadIdx.y);  // this lane's rows: r0 + j kRows
  uint32_t u[kPer] = {};
#pragma unroll
  for (int j = 0; j < kPer; ++j)  // all four loads in flight before the first use
    if (r0 + j * kRows < n_rows) u[j] = load_pixel<PACKED>(src, r0 + j * kRows, c);
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int r = r0 + j * kRows;
    if (r >= n_rows) return;
    uint32_t v = u[j];
    if (p.has_lut)
      v = (lut[v & 255u] & 0xffu) | (lut[(v >> 8) & 255u] & 0xff00u) | (lut[(v >> 16) & 255u] & 0xff0000u) | (lut[v >> 24] & 0xff000000u);
    for (int k = 0; k < p.n_rects; ++k) {  // one 16-byte scalar load per rectangle, no branch on its outcome
      const int32_t* q = p.rects[k];
      const bool inside = (c >= q[0]) & (r >= q[1]) & (c <= q[2]) & (r <= q[3]);
      v = inside ? p.fills[k] : v;
    }
    store_pixel<PACKED>(dst + r * src.row_stride + c * src.pix_stride, src.chan_stride, v);
  }
}

struct Pinhole {
  float fx, fy, cx, cy, m[12], near, far;
};

__global__ void __launch_bounds__(kRayThreads) pinhole_rays_kernel(Pinhole k, int w, int64_t n, float4* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * kRayThreads + threadIdx.x;
  if (p >= n) return;
  int64_t r, c;
  if (n <= 0xffffffffll) {  // uniform over the launch: a 32-bit division where the index fits
    r = (uint32_t)p / (uint32_t)w, c = (uint32_t)p % (uint32_t)w;
  } else {
    r = p / w, c = p % w;
  }
  const double dx = ((double)c - (double)k.cx) / (double)k.fx, dy = -(((double)r - (double)k.cy) / (double)k.fy), dz = -1.0;
  double v[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) v[j] = (dx * (double)k.m[4 * j] + dy * (double)k.m[4 * j + 1]) + dz * (double)k.m[4 * j + 2];
  const double norm = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  out[2 * p] = make_float4(k.m[3], k.m[7], k.m[11], (float)(v[0] / norm));
  out[2 * p + 1] = make_float4((float)(v[1] / norm), (float)(v[2] / norm), k.near, k.far);
}

}  // namespace blender
}  // namespace sr

using namespace sr;
using namespace sr::blender;

extern "C" int sr_blender_colors_scratch(int src_h, int src_w, int out_h, int out_w, int64_t* bytes) {
  SR_REQUIRE(bytes, "sr_blender_colors_scratch: null pointer");
  SR_REQUIRE(src_h >= 1 && src_w >= 1 && src_h <= kMaxSide && src_w <= kMaxSide,
             "sr_blender_colors_scratch: the source sides must lie in 1..%d (got %d x %d)", kMaxSide, src_h, src_w);
  SR_REQUIRE(out_h >= 0 && out_w >= 0 && out_h <= kMaxSide && out_w <= kMaxSide,
             "sr_blender_colors_scratch: the output sides must lie in 0..%d (got %d x %d)", kMaxSide, out_h, out_w);
  ScratchCarver c(nullptr);
  if (out_h != src_h && out_w != src_w && out_h > 0 && out_w > 0) c.take<uint32_t>((int64_t)src_h * out_w, 4);  // both passes run
  *bytes = c.bytes();
  return 0;
}

extern "C" int sr_blender_colors(const uint8_t* src, int src_h, int src_w, int64_t row_stride, int64_t pix_stride, int64_t chan_stride,
                                 int out_h, int out_w, const int32_t* coef_w, int ksize_w, const int32_t* coef_h, int ksize_h,
                                 void* scratch, int64_t scratch_bytes, float* rgbs, uint8_t* valid_mask, uint8_t* rgba, int stages,
                                 void* stream) {
  int64_t need = 0;
  if (sr_blender_colors_scratch(src_h, src_w, out_h, out_w, &need)) return 1;
  SR_REQUIRE(row_stride >= 1 && pix_stride >= 1 && chan_stride >= 1,
             "sr_blender_colors: strides must be positive byte counts (got row %lld, pixel %lld, channel %lld)", (long long)row_stride,
             (long long)pix_stride, (long long)chan_stride);
  SR_REQUIRE(stages >= 0 && stages <= 1, "sr_blender_colors: stages must be 0 (everything) or 1 (stop after the first pass), got %d", stages);
  if ((int64_t)out_h * out_w == 0) return 0;
  SR_REQUIRE(src && rgbs, "sr_blender_colors: null pointer");
  SR_REQUIRE((reinterpret_cast<uintptr_t>(rgba) & 3) == 0, "sr_blender_colors: rgba must be 4-byte aligned");
  const bool horiz = out_w != src_w, vert = out_h != src_h;
  if (horiz) {
    SR_REQUIRE(coef_w, "sr_blender_colors: null coefficient table for the horizontal pass");
    SR_REQUIRE(ksize_w == lanczos_ksize(src_w, out_w), "sr_blender_colors: a table of ksize %d does not fit the resize %d -> %d (ksize %d)",
               ksize_w, src_w, out_w, lanczos_ksize(src_w, out_w));
  }
  if (vert) {
    SR_REQUIRE(coef_h, "sr_blender_colors: null coefficient table for the vertical pass");
    SR_REQUIRE(ksize_h == lanczos_ksize(src_h, out_h), "sr_blender_colors: a table of ksize %d does not fit the resize %d -> %d (ksize %d)",
               ksize_h, src_h, out_h, lanczos_ksize(src_h, out_h));
  }
  if (need) {
    SR_REQUIRE(scratch && (reinterpret_cast<uintptr_t>(scratch) & 3) == 0, "sr_blender_colors: scratch must be a 4-byte aligned pointer");
    SR_REQUIRE(scratch_bytes >= need, "sr_blender_colors: scratch holds %lld bytes, %lld are needed", (long long)scratch_bytes, (long long)need);
  }
  hipStream_t s = (hipStream_t)stream;
  const Source from{src, row_stride, pix_stride, chan_stride};
  const bool packed = pix_stride == 4 && chan_stride == 1 && (row_stride & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 3) == 0;
  const Outputs out{rgbs, valid_mask, reinterpret_cast<uint32_t*>(rgba)};
  const dim3 block(kLanes, kRows);
  auto axis = [](int n_in, int n_out, const int32_t* coef, int ksize) {
    const double scale = (double)n_in / (double)n_out;
    return Axis{scale, 3.0 * (scale < 1.0 ? 1.0 : scale), coef, n_in, ksize};
  };
  if (!horiz && !vert) {
    if (packed)
      hipLaunchKernelGGL(convert_kernel<true>, grid_for(out_h, out_w), block, 0, s, from, out_h, out_w, out);
    else
      hipLaunchKernelGGL(convert_kernel<false>, grid_for(out_h, out_w), block, 0, s, from, out_h, out_w, out);
    return check_launch("blender convert_kernel");
  }
  uint32_t* mid = ScratchCarver(scratch).take<uint32_t>((int64_t)src_h * out_w, 4);  // the one piece; unused unless both passes run
  if (horiz) {  // (src_h, out_w) from the source
    const Axis a = axis(src_w, out_w, coef_w, ksize_w);
    const int last = !vert;
    if (packed)
      hipLaunchKernelGGL((resample_kernel<false, true>), grid_for(src_h, out_w), block, 0, s, from, a, src_h, out_w, 1, last, mid, out);
    else
      hipLaunchKernelGGL((resample_kernel<false, false>), grid_for(src_h, out_w), block, 0, s, from, a, src_h, out_w, 1, last, mid, out);
    if (check_launch("blender resample_kernel (horizontal)")) return 1;
    if (!vert || stages == 1) return 0;
  }
  const Axis a = axis(src_h, out_h, coef_h, ksize_h);
  if (horiz) {  // from the packed intermediate
    const Source inter{reinterpret_cast<const uint8_t*>(mid), 4 * (int64_t)out_w, 4, 1};
    hipLaunchKernelGGL((resample_kernel<true, true>), grid_for(out_h, out_w), block, 0, s, inter, a, out_h, out_w, 0, 1, mid, out);
  } else if (packed) {
    hipLaunchKernelGGL((resample_kernel<true, true>), grid_for(out_h, out_w), block, 0, s, from, a, out_h, out_w, 1, 1, mid, out);
  } else {
    hipLaunchKernelGGL((resample_kernel<true, false>), grid_for(out_h, out_w), block, 0, s, from, a, out_h, out_w, 1, 1, mid, out);
  }
  return check_launch("blender resample_kernel (vertical)");
}

extern "C" int sr_blender_perturb(const uint8_t* src, uint8_t* dst, int h, int w, int64_t row_stride, int64_t pix_stride, int64_t chan_stride,
                                  const uint8_t* lut, const int32_t* rects, const uint8_t* fills, int n_rects, void* stream) {
  SR_REQUIRE(src && dst, "sr_blender_perturb: null image (src %p, dst %p)", (const void*)src, (const void*)dst);
  SR_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "sr_blender_perturb: the sides must lie in 1..%d (got %d x %d)", kMaxSide, h, w);
  constexpr int64_t kMaxStride = 1ll << 40;  // keeps the extent below free of overflow
  SR_REQUIRE(row_stride >= 1 && pix_stride >= 1 && chan_stride >= 1 && row_stride <= kMaxStride && pix_stride <= kMaxStride && chan_stride <= kMaxStride,
             "sr_blender_perturb: strides must be positive byte counts up to 2^40 (got row %lld, pixel %lld, channel %lld)",
             (long long)row_stride, (long long)pix_stride, (long long)chan_stride);
  SR_REQUIRE(n_rects >= 0 && n_rects <= kMaxRects, "sr_blender_perturb: n_rects must lie in 0..%d (got %d)", kMaxRects, n_rects);
  SR_REQUIRE(n_rects == 0 || (rects && fills), "sr_blender_perturb: null rects or fills with n_rects = %d", n_rects);
  const int64_t extent = (h - 1) * row_stride + (w - 1) * pix_stride + 3 * chan_stride + 1;  // bytes from the first to past the last
  const uintptr_t a = reinterpret_cast<uintptr_t>(src), b = reinterpret_cast<uintptr_t>(dst);
  SR_REQUIRE(a == b || (a < b ? b - a : a - b) >= (uintptr_t)extent,
             "sr_blender_perturb: dst must be src itself or not overlap it (the image spans %lld bytes)", (long long)extent);
  Perturb p{};
  p.n_rects = n_rects, p.has_lut = lut != nullptr;
  if (lut)
    for (int v = 0; v < 256; ++v) p.lut[v] = (uint32_t)lut[v] | ((uint32_t)lut[256 + v] << 8) | ((uint32_t)lut[512 + v] << 16) | ((uint32_t)lut[768 + v] << 24);
  for (int k = 0; k < n_rects; ++k) {
    for (int j = 0; j < 4; ++j) p.rects[k][j] = rects[4 * k + j];
    p.fills[k] = (uint32_t)fills[4 * k] | ((uint32_t)fills[4 * k + 1] << 8) | ((uint32_t)fills[4 * k + 2] << 16) | ((uint32_t)fills[4 * k + 3] << 24);
  }
  const Source from{src, row_stride, pix_stride, chan_stride};
  const bool packed = pix_stride == 4 && chan_stride == 1 && (row_stride & 3) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 3) == 0;
  const dim3 grid(blocks_for(w, kLanes), blocks_for(h, kPerturbRows)), block(kLanes, kRows);
  if (packed)
    hipLaunchKernelGGL(perturb_kernel<true>, grid, block, 0, (hipStream_t)stream, from, dst, h, w, p);
  else
    hipLaunchKernelGGL(perturb_kernel<false>, grid, block, 0, (hipStream_t)stream, from, dst, h, w, p);
  return check_launch("blender perturb_kernel");
}

extern "C" int sr_pinhole_rays(int h, int w, float fx, float fy, float cx, float cy, const float* c2w, float near, float far, float* out,
                               void* stream) {
  SR_REQUIRE(h >= 0 && w >= 0, "sr_pinhole_rays: the grid must be >= 0 x 0 (got %d x %d)", h, w);
  SR_REQUIRE(c2w, "sr_pinhole_rays: null c2w");
  SR_REQUIRE(fx != 0.f && fy != 0.f && fx == fx && fy == fy, "sr_pinhole_rays: fx and fy must be non-zero numbers (got %g, %g)", (double)fx,
             (double)fy);
  const int64_t n = (int64_t)h * w;
  if (n == 0) return 0;
  SR_REQUIRE(out && (reinterpret_cast<uintptr_t>(out) & 15) == 0, "sr_pinhole_rays: out must be a 16-byte aligned pointer");
  const int64_t blocks = (n + kRayThreads - 1) / kRayThreads;
  SR_REQUIRE(blocks <= 0x7fffffffll, "sr_pinhole_rays: %d x %d is too large", h, w);
  Pinhole k{fx, fy, cx, cy, {}, near, far};
  for (int i = 0; i < 12; ++i) k.m[i] = c2w[i];
  hipLaunchKernelGGL(pinhole_rays_kernel, dim3((unsigned)blocks), dim3(kRayThreads), 0, (hipStream_t)stream, k, w, n, reinterpret_cast<float4*>(out));
  return check_launch("pinhole_rays_kernel");
}
