// Orthorectification of an image onto a DSM raster for gfx950: per DSM cell the pixel its surface point
// projects to through the view's RPC camera, whether the raster itself stands in the line of sight, and the image resampled there;
// several views fuse into a mean by per-cell accumulators.  Two launches, as section 7.15 found for the ray cast: the projection
// (utm_inverse, rpc_project, Newton localisation of the segment's far end, utm_forward) and the walk + sample + accumulate, handing
// over through caller-owned scratch, so the projection's registers do not set the walk's occupancy.
// All geometry and all sampling weights are fp64 with contraction off.  One lane per cell doing everything: no LDS, no atomics, no
// cross-lane traffic; views are accumulated one after another on the stream, so a mosaic is deterministic.
#include <math.h>

#include "common.h"
#include "geo_device.h"
#include "heightfield_device.h"
#include "orthorectify_device.h"
#include "rpc_device.h"

namespace sr {

struct OrthoFrame {  // the raster's place in UTM, host-filled
  double xoff, yoff;
  int zone;
};

// One lane per cell: colrow, the status the projection decides (pre) and, where a walk is due, the grid-frame (x, y) of the far end B
// of the line of sight: the view's own localisation of (col, row) at the raster's maximum, rpc_ray8's arithmetic for a ray origin.
__global__ void __launch_bounds__(256) ortho_project_kernel(const HfGrid g, const OrthoFrame f, const RpcModel m, int width, int height,
                                                           double bias, long n, double* __restrict__ colrow, double* __restrict__ seg_b,
                                                           uint8_t* __restrict__ pre) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float hf = g.hgt[i];
  const double nan = __builtin_nan("");
  double col = nan, row = nan, xb = nan, yb = nan;
  const double top = (double)*g.gmax;
  if (isfinite(hf)) {
    const int j = (int)(i / g.xsize), c = (int)(i % g.xsize);
    double lat, lon;
    utm_inverse(f.xoff + ((double)c + 0.5) * g.res, f.yoff - ((double)j + 0.5) * g.res, f.zone, lat, lon);
    rpc_project(m, lon, lat, (double)hf, col, row);
  }
  const uint8_t st = ortho_classify(hf, col, row, width, height, bias, top);
  if (st == kOrthoWalk) {
    double x, y, e, nn;
    rpc_localize(m, (col - m.col_offset) / m.col_scale, (row - m.row_offset) / m.row_scale, (top - m.alt_offset) / m.alt_scale, x, y);
    utm_forward(x * m.lat_scale + m.lat_offset, y * m.lon_scale + m.lon_offset, f.zone, e, nn);
    xb = e - f.xoff, yb = f.yoff - nn;
  }
  colrow[2 * i] = col, colrow[2 * i + 1] = row;
  seg_b[2 * i] = xb, seg_b[2 * i + 1] = yb;
  pre[i] = st;
}

// One lane per cell: the walk from (cell centre, h + bias) to B at the raster's maximum with the cell itself passed through, the
// final status, the colour of a visible cell, and its share of the accumulators.
template <int MODE>
__global__ void __launch_bounds__(256) ortho_sample_kernel(const HfGrid g, const OrthoImage im, double bias, long n,
                                                          const double* __restrict__ colrow, const double* __restrict__ seg_b,
                                                          const uint8_t* __restrict__ pre, float* __restrict__ color,
                                                          uint8_t* __restrict__ status, double* __restrict__ sum, int* __restrict__ count) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint8_t st = pre[i];
  if (st == kOrthoWalk) {
    const int j = (int)(i / g.xsize), c = (int)(i % g.xsize);
    const double xa = ((double)c + 0.5) * g.res, ya = ((double)j + 0.5) * g.res, za = (double)g.hgt[i] + bias;
    double s;
    int id;
    st = hf_walk(g, xa, ya, za, seg_b[2 * i], seg_b[2 * i + 1], (double)*g.gmax, (int)i, s, id) ? kOrthoOccluded : kOrthoVisible;
  }
  status[i] = st;
  float* out = color + i * im.channels;
  if (st != kOrthoVisible) {
    for (int ch = 0; ch < im.channels; ++ch) out[ch] = __builtin_nanf("");
    return;
  }
  const double col = colrow[2 * i], row = colrow[2 * i + 1];
  for (int ch = 0; ch < im.channels; ++ch) {
    const float v = ortho_sample<MODE>(im, col, row, ch);
    out[ch] = v;
    if (sum) sum[i * im.channels + ch] = sum[i * im.channels + ch] + (double)v;
  }
  if (count) count[i] = count[i] + 1;
}

// scratch of n cells: B's (x, y) per cell, then the projection's status bytes
static void carve(ScratchCarver& sc, int64_t n, double*& seg_b, uint8_t*& pre) {
  seg_b = sc.take<double>(2 * n, 256);
  pre = sc.take<uint8_t>(n, 256);
}

static int check_raster(const char* fn, int xsize, int ysize) {
  SR_REQUIRE(xsize >= 1 && ysize >= 1, "%s: empty raster (%d x %d)", fn, ysize, xsize);
  SR_REQUIRE((int64_t)xsize * ysize < ((int64_t)1 << 31), "%s: raster %d x %d has 2^31 cells or more", fn, ysize, xsize);
  return 0;
}

}  // namespace sr

using namespace sr;

// HOST only: bytes of caller-owned scratch sr_orthorectify needs for an (ysize, xsize) raster.
extern "C" int sr_orthorectify_scratch(int xsize, int ysize, int64_t* bytes) {
  SR_REQUIRE(bytes, "sr_orthorectify_scratch: null pointer");
  if (check_raster("sr_orthorectify_scratch", xsize, ysize)) return 1;
  ScratchCarver sc(nullptr);
  double* seg_b;
  uint8_t* pre;
  carve(sc, (int64_t)xsize * ysize, seg_b, pre);
  *bytes = sc.bytes();
  return 0;
}

// One view onto the raster (include/satrender.h states the semantics in full).  stages 0 = both launches, 1 = the projection alone
// (colrow and scratch are written), 2 = the walk + sample alone, reading the colrow and scratch a stage-1 call with the same raster,
// camera and bias left behind.
extern "C" int sr_orthorectify(const float* hgt, int xsize, int ysize, double resolution, double xoff, double yoff, int zone,
                               const float* blockmax, const float* gmax, int accelerate, const double* rpc, const void* image, int fmt,
                               int width, int height, int channels, int64_t row_stride, int64_t pix_stride, int mode, double bias,
                               int stages, void* scratch, int64_t scratch_bytes, float* color, uint8_t* status, double* colrow,
                               double* sum, int* count, void* stream) {
  const char* fn = "sr_orthorectify";
  if (check_raster(fn, xsize, ysize)) return 1;
  SR_REQUIRE(isfinite(resolution) && resolution > 0, "%s: resolution must be finite and > 0 (got %g)", fn, resolution);
  SR_REQUIRE(isfinite(xoff) && isfinite(yoff), "%s: non-finite grid offset", fn);
  SR_REQUIRE(zone >= 1 && zone <= 60, "%s: zone must be in 1..60 (got %d)", fn, zone);
  SR_REQUIRE(accelerate == 0 || accelerate == 1, "%s: accelerate must be 0 or 1 (got %d)", fn, accelerate);
  SR_REQUIRE(hgt && gmax && image && scratch && color && status && colrow, "%s: null pointer", fn);
  SR_REQUIRE(!accelerate || blockmax, "%s: the two-level walk needs blockmax (null pointer)", fn);
  SR_REQUIRE(width >= 1 && height >= 1, "%s: empty image (%d x %d)", fn, height, width);
  SR_REQUIRE(channels >= 1 && channels <= 4, "%s: channels must be in 1..4 (got %d)", fn, channels);
  SR_REQUIRE(fmt == kOrthoU8 || fmt == kOrthoF32, "%s: fmt must be 0 (uint8) or 1 (fp32) (got %d)", fn, fmt);
  SR_REQUIRE(pix_stride >= channels && row_stride >= (int64_t)(width - 1) * pix_stride + channels,
             "%s: strides (%lld, %lld) overlap for a %d x %d x %d image", fn, (long long)row_stride, (long long)pix_stride, height, width,
             channels);
  SR_REQUIRE(mode >= kOrthoNearest && mode <= kOrthoBicubic, "%s: mode must be 0 (nearest), 1 (bilinear) or 2 (bicubic) (got %d)", fn, mode);
  SR_REQUIRE(isfinite(bias) && bias >= 0, "%s: bias must be finite and >= 0 (got %g)", fn, bias);
  SR_REQUIRE(stages >= 0 && stages <= 2, "%s: stages must be 0, 1 or 2 (got %d)", fn, stages);
  SR_REQUIRE((sum != nullptr) == (count != nullptr), "%s: give both accumulators, sum and count, or neither", fn);
  RpcModel m;
  if (load_rpc(fn, rpc, m)) return 1;
  const int64_t n = (int64_t)xsize * ysize;
  ScratchCarver sc(scratch);
  double* seg_b;
  uint8_t* pre;
  carve(sc, n, seg_b, pre);
  if (require_scratch(fn, scratch_bytes, sc.bytes())) return 1;
  SR_REQUIRE(((uintptr_t)scratch & 7) == 0, "%s: scratch must be 8-byte aligned", fn);

  HfGrid g;
  g.hgt = hgt, g.blockmax = blockmax, g.gmax = gmax, g.res = resolution;
  g.xsize = xsize, g.ysize = ysize, g.bw = (xsize + kHfBlock - 1) / kHfBlock, g.accelerate = accelerate;
  const OrthoFrame f = {xoff, yoff, zone};
  const OrthoImage im = {image, row_stride, pix_stride, width, height, channels, fmt};
  const hipStream_t st = (hipStream_t)stream;
  if (stages != 2) {
    hipLaunchKernelGGL(ortho_project_kernel, dim3(blocks_for(n)), dim3(256), 0, st, g, f, m, width, height, bias, (long)n, colrow, seg_b, pre);
    if (check_launch("ortho_project_kernel")) return 2;
  }
  if (stages == 1) return 0;
  const dim3 grid(blocks_for(n)), block(256);
  if (mode == kOrthoNearest)
    hipLaunchKernelGGL(ortho_sample_kernel<kOrthoNearest>, grid, block, 0, st, g, im, bias, (long)n, colrow, seg_b, pre, color, status, sum, count);
  else if (mode == kOrthoBilinear)
    hipLaunchKernelGGL(ortho_sample_kernel<kOrthoBilinear>, grid, block, 0, st, g, im, bias, (long)n, colrow, seg_b, pre, color, status, sum, count);
  else
    hipLaunchKernelGGL(ortho_sample_kernel<kOrthoBicubic>, grid, block, 0, st, g, im, bias, (long)n, colrow, seg_b, pre, color, status, sum, count);
  return check_launch("ortho_sample_kernel");
}
