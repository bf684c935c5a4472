// The per-cell decisions and the image resampling of the orthorectification, shared by the kernels of
// orthorectify.hip.  Plain fp64 C++ with contraction off and no device intrinsic, __host__ __device__ as hf_walk is: a CPU build
// computes the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace sr {

// a cell's status; kOrthoWalk exists only between the two launches (in scratch): the line of sight is still to be walked
enum : uint8_t { kOrthoEmpty = 0, kOrthoVisible = 1, kOrthoOccluded = 2, kOrthoOutside = 3, kOrthoWalk = 4 };
enum { kOrthoNearest = 0, kOrthoBilinear = 1, kOrthoBicubic = 2 };
enum { kOrthoU8 = 0, kOrthoF32 = 1 };

struct OrthoImage {  // host-filled, passed by value: pixel (row, col), channel ch at data[row row_stride + col pix_stride + ch]
  const void* data;
  int64_t row_stride, pix_stride;  // in elements
  int width, height, channels, fmt;
};

// What the projection alone decides about a cell of height hf projected to (col, row): empty, outside the image, visible because
// nothing stands above it, or to be walked.  Pixel centres sit at integers: the image covers [0, W-1] x [0, H-1].
__host__ __device__ __forceinline__ uint8_t ortho_classify(float hf, double col, double row, int width, int height, double bias, double top) {
#pragma clang fp contract(off)
  if (!isfinite(hf)) return kOrthoEmpty;
  if (!(isfinite(col) && isfinite(row)) || col < 0.0 || col > (double)(width - 1) || row < 0.0 || row > (double)(height - 1))
    return kOrthoOutside;
  return (double)hf + bias >= top ? kOrthoVisible : kOrthoWalk;
}

// pixel (y, x), channel ch as a double, indices clamped to the image (edge replicate): no read outside it, whatever y and x are
__host__ __device__ __forceinline__ double ortho_pixel(const OrthoImage& im, int y, int x, int ch) {
  y = y < 0 ? 0 : (y > im.height - 1 ? im.height - 1 : y);
  x = x < 0 ? 0 : (x > im.width - 1 ? im.width - 1 : x);
  const int64_t at = (int64_t)y * im.row_stride + (int64_t)x * im.pix_stride + ch;
  if (im.fmt == kOrthoU8) return (double)static_cast<const uint8_t*>(im.data)[at] / 255.0;
  return (double)static_cast<const float*>(im.data)[at];
}

// Keys' cubic convolution kernel with a = -0.5 at distance s >= 0
__host__ __device__ __forceinline__ double ortho_keys(double s) {
#pragma clang fp contract(off)
  const double a = -0.5;
  if (s <= 1.0) return ((a + 2.0) * s - (a + 3.0)) * s * s + 1.0;
  if (s < 2.0) return ((a * s - 5.0 * a) * s + 8.0 * a) * s - 4.0 * a;
  return 0.0;
}

// Channel ch of the image at (col, row), which lies inside [0, W-1] x [0, H-1]; fp64 throughout, rounded to fp32 once.  A NaN pixel
// under a tap propagates, also under a zero weight.
template <int MODE>
__host__ __device__ __forceinline__ float ortho_sample(const OrthoImage& im, double col, double row, int ch) {
#pragma clang fp contract(off)
  if (MODE == kOrthoNearest) return (float)ortho_pixel(im, (int)floor(row + 0.5), (int)floor(col + 0.5), ch);
  const double x0 = floor(col), y0 = floor(row);
  const double fx = col - x0, fy = row - y0;
  const int ix = (int)x0, iy = (int)y0;
  if (MODE == kOrthoBilinear) {
    const double p00 = ortho_pixel(im, iy, ix, ch), p01 = ortho_pixel(im, iy, ix + 1, ch);
    const double p10 = ortho_pixel(im, iy + 1, ix, ch), p11 = ortho_pixel(im, iy + 1, ix + 1, ch);
    const double t0 = (1.0 - fx) * p00 + fx * p01, t1 = (1.0 - fx) * p10 + fx * p11;
    return (float)(t0 * (1.0 - fy) + t1 * fy);
  }
  // taps ix - 1 .. ix + 2 at distances 1 + fx, fx, 1 - fx, 2 - fx; every row's columns first, then the rows, in increasing index order
  const double wx[4] = {ortho_keys(1.0 + fx), ortho_keys(fx), ortho_keys(1.0 - fx), ortho_keys(2.0 - fx)};
  const double wy[4] = {ortho_keys(1.0 + fy), ortho_keys(fy), ortho_keys(1.0 - fy), ortho_keys(2.0 - fy)};
  double acc = 0.0;
  for (int m = 0; m < 4; ++m) {
    double line = 0.0;
    for (int k = 0; k < 4; ++k) line = line + wx[k] * ortho_pixel(im, iy - 1 + m, ix - 1 + k, ch);
    acc = acc + wy[m] * line;
  }
  return (float)acc;
}

}  // namespace sr
