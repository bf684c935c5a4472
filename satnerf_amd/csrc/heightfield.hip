// Ray casting against a DSM raster for gfx950: the raster taken as geometry -- every finite cell a solid
// column -- and a straight segment walked through its cells in order until it enters one.  Two users share one traversal: the cast of
// camera or sun rays (sr_heightfield_cast) and the shadow mask of the raster under a sun direction (sr_heightfield_shadow).
// All geometry is fp64 with contraction off.  One lane per ray doing everything: no LDS, no atomics, no cross-lane traffic, so a result
// depends on its own ray only.  The block maxima (sr_heightfield_blockmax) are a plain max: no order problem.
#include <math.h>

#include "common.h"
#include "geo_device.h"
#include "heightfield_device.h"

namespace sr {

struct HfFrame {  // the scene frame of sr_heightfield_cast's rays, host-filled
  double cx, cy, cz, range;
  int zone;
};

// One lane per end of a ray (k = 0: near, 1: far): row i of seg = (E, N, alt) of o + d near, then of o + d far, by depth_utm_kernel's
// arithmetic (dsm.hip).  A launch of its own: the projection's registers would otherwise set the walk's occupancy.
__global__ void __launch_bounds__(256) hf_project_kernel(const HfFrame f, const float* __restrict__ rays, int ray_stride, long n,
                                                        double* __restrict__ seg) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * n) return;
  const long i = t >> 1;
  const int k = (int)(t & 1);
  const float* r = rays + i * ray_stride;
  double la, lo, al, e, nn;
  latlonalt_from_ray(r, r[6 + k], f.cx, f.cy, f.cz, f.range, la, lo, al);
  utm_forward(la, lo, f.zone, e, nn);
  double* w = seg + 6 * i + 3 * k;
  w[0] = e, w[1] = nn, w[2] = al;
}

// One lane per ray.  rays != nullptr: A, B = row i of seg (UTM) moved into the grid frame, the reported depth near + s (far - near);
// else A, B = rows of seg_a, seg_b in the grid frame and the depth is s itself.
__global__ void __launch_bounds__(256) hf_cast_kernel(const HfGrid g, double xoff, double yoff, const float* __restrict__ rays, int ray_stride,
                                                     const double* __restrict__ seg_a, const double* __restrict__ seg_b,
                                                     const double* __restrict__ seg, long n, float* __restrict__ depth,
                                                     int* __restrict__ cell, double* __restrict__ s_out) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double xa, ya, za, xb, yb, zb, near = 0.0, far = 1.0;
  bool ok = true;
  if (rays) {
    const double* u = seg + 6 * i;
    near = (double)rays[i * ray_stride + 6], far = (double)rays[i * ray_stride + 7];
    ok = isfinite(near) && isfinite(far) && far >= near;
    xa = u[0] - xoff, ya = yoff - u[1], za = u[2], xb = u[3] - xoff, yb = yoff - u[4], zb = u[5];
  } else {
    xa = seg_a[3 * i], ya = seg_a[3 * i + 1], za = seg_a[3 * i + 2];
    xb = seg_b[3 * i], yb = seg_b[3 * i + 1], zb = seg_b[3 * i + 2];
  }
  double s = __builtin_nan("");
  int id = -1;
  const bool hit = ok && hf_walk(g, xa, ya, za, xb, yb, zb, -1, s, id);
  depth[i] = hit ? (float)(near + s * (far - near)) : __builtin_nanf("");
  cell[i] = hit ? id : -1;
  if (s_out) s_out[i] = hit ? s : __builtin_nan("");
}

// One lane per cell: the segment from (cell centre, h + bias) along the sun's unit vector (ue, -un, uu in the grid frame) up to the
// raster's maximum, the start cell passed through.  1 lit, 0 shadowed, NaN where the cell is empty.
__global__ void __launch_bounds__(256) hf_shadow_kernel(const HfGrid g, double ue, double un, double uu, double bias, long n,
                                                       float* __restrict__ out) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float hf = g.hgt[i];
  if (!isfinite(hf)) {
    out[i] = __builtin_nanf("");
    return;
  }
  const int j = (int)(i / g.xsize), c = (int)(i % g.xsize);
  const double top = (double)*g.gmax;
  const double xa = ((double)c + 0.5) * g.res, ya = ((double)j + 0.5) * g.res, za = (double)hf + bias;
  if (za >= top) {  // nothing stands above the start
    out[i] = 1.f;
    return;
  }
  const double t = (top - za) / uu;
  double s;
  int id;
  out[i] = hf_walk(g, xa, ya, za, xa + t * ue, ya - t * un, top, (int)i, s, id) ? 0.f : 1.f;
}

// The maximum of the finite cells of each 16 x 16 block, one 256-thread workgroup per block and one cell per thread: xor shuffles
// within a wave, four values through LDS.  -inf where the block has no finite cell.
__global__ void __launch_bounds__(256) hf_blockmax_kernel(const float* __restrict__ hgt, int xsize, int ysize, int bw,
                                                         float* __restrict__ blockmax) {
  __shared__ float red[4];
  const int bj = blockIdx.x / bw, bc = blockIdx.x % bw;
  const int j = bj * kHfBlock + (int)threadIdx.x / kHfBlock, c = bc * kHfBlock + (int)threadIdx.x % kHfBlock;
  float v = -__builtin_inff();
  if (j < ysize && c < xsize) {
    const float h = hgt[(long)j * xsize + c];
    if (isfinite(h)) v = h;
  }
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x / 64] = v;
  __syncthreads();
  if (threadIdx.x == 0) blockmax[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// The maximum of the block maxima: one workgroup.
__global__ void __launch_bounds__(256) hf_globalmax_kernel(const float* __restrict__ blockmax, int nb, float* __restrict__ gmax) {
  __shared__ float red[4];
  float v = -__builtin_inff();
  for (int k = threadIdx.x; k < nb; k += 256) v = fmaxf(v, blockmax[k]);
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x / 64] = v;
  __syncthreads();
  if (threadIdx.x == 0) gmax[0] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// the raster checks the three entries share
static int check_raster(const char* fn, const float* hgt, int xsize, int ysize, double resolution) {
  SR_REQUIRE(xsize >= 1 && ysize >= 1, "%s: empty raster (%d x %d)", fn, ysize, xsize);
  SR_REQUIRE((int64_t)xsize * ysize < ((int64_t)1 << 31), "%s: raster %d x %d has 2^31 cells or more", fn, ysize, xsize);
  SR_REQUIRE(isfinite(resolution) && resolution > 0, "%s: resolution must be finite and > 0 (got %g)", fn, resolution);
  SR_REQUIRE(hgt, "%s: null pointer", fn);
  return 0;
}

static HfGrid make_grid(const float* hgt, int xsize, int ysize, double resolution, const float* blockmax, const float* gmax, int accelerate) {
  HfGrid g;
  g.hgt = hgt, g.blockmax = blockmax, g.gmax = gmax, g.res = resolution;
  g.xsize = xsize, g.ysize = ysize, g.bw = (xsize + kHfBlock - 1) / kHfBlock, g.accelerate = accelerate;
  return g;
}

}  // namespace sr

using namespace sr;

// The maxima of the finite cells of the raster's 16 x 16 blocks, -inf where a block has none, and their maximum: what the two-level walk
// and the shadow mask's end point read.  A max has no order problem; two launches, no atomics.
extern "C" int sr_heightfield_blockmax(const float* hgt, int xsize, int ysize, float* blockmax, float* gmax, void* stream) {
  if (check_raster("sr_heightfield_blockmax", hgt, xsize, ysize, 1.0)) return 1;
  SR_REQUIRE(blockmax && gmax, "sr_heightfield_blockmax: null pointer");
  const int bw = (xsize + kHfBlock - 1) / kHfBlock, bh = (ysize + kHfBlock - 1) / kHfBlock;
  hipLaunchKernelGGL(hf_blockmax_kernel, dim3(bw * bh), dim3(256), 0, (hipStream_t)stream, hgt, xsize, ysize, bw, blockmax);
  if (check_launch("hf_blockmax_kernel")) return 2;
  hipLaunchKernelGGL(hf_globalmax_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, blockmax, bw * bh, gmax);
  return check_launch("hf_globalmax_kernel");
}

// Per ray the first column of the raster it enters (include/satrender.h states the walk in full): the segment A -> B is clipped to the
// grid, cells are visited in order of s with crossings (k r - xA) / (xB - xA) taken from the absolute index k and never accumulated, a
// tie steps both indices, and a visited finite cell is hit at s_in when z(s_in) <= h, else at (h - zA) / (zB - zA) when z(s_out) <= h.
// Rays in the scene frame are first projected into seg by sr_depth_to_utm's arithmetic and walked along the chord; a ray with an end
// that is not finite or with far < near is a miss.  accelerate = 1 jumps blocks whose maximum lies below the segment: the same bits.
extern "C" int sr_heightfield_cast(const float* hgt, int xsize, int ysize, double resolution, const float* blockmax, const float* gmax,
                                   int accelerate, const float* rays, int ray_stride, const double* center, double range, int zone,
                                   double xoff, double yoff, const double* seg_a, const double* seg_b, int64_t n, float* depth, int* cell,
                                   double* s, double* seg, void* stream) {
  if (check_raster("sr_heightfield_cast", hgt, xsize, ysize, resolution)) return 1;
  SR_REQUIRE(accelerate == 0 || accelerate == 1, "sr_heightfield_cast: accelerate must be 0 or 1 (got %d)", accelerate);
  SR_REQUIRE(!accelerate || (blockmax && gmax), "sr_heightfield_cast: the two-level walk needs blockmax and gmax (null pointer)");
  SR_REQUIRE((rays != nullptr) != (seg_a != nullptr || seg_b != nullptr),
             "sr_heightfield_cast: give either rays or the segments seg_a and seg_b");
  HfFrame f = {0, 0, 0, 1, 1};
  if (rays) {
    SR_REQUIRE(ray_stride >= 8, "sr_heightfield_cast: ray_stride must be >= 8 (got %d)", ray_stride);
    SR_REQUIRE(zone >= 1 && zone <= 60, "sr_heightfield_cast: zone must be in 1..60 (got %d)", zone);
    SR_REQUIRE(isfinite(range) && range > 0, "sr_heightfield_cast: scene range must be finite and > 0 (got %g)", range);
    SR_REQUIRE(isfinite(xoff) && isfinite(yoff), "sr_heightfield_cast: non-finite grid offset");
    SR_REQUIRE(center, "sr_heightfield_cast: null pointer");
    SR_REQUIRE(isfinite(center[0]) && isfinite(center[1]) && isfinite(center[2]), "sr_heightfield_cast: non-finite scene center");
    f.cx = center[0], f.cy = center[1], f.cz = center[2], f.range = range, f.zone = zone;
  } else {
    SR_REQUIRE(seg_a && seg_b, "sr_heightfield_cast: null pointer");
    SR_REQUIRE(!seg, "sr_heightfield_cast: seg is an output of the ray form only");
  }
  if (n <= 0) return 0;
  SR_REQUIRE(depth && cell && (seg || !rays), "sr_heightfield_cast: null pointer");
  const HfGrid g = make_grid(hgt, xsize, ysize, resolution, blockmax, gmax, accelerate);
  if (rays) {
    hipLaunchKernelGGL(hf_project_kernel, dim3(blocks_for(2 * n)), dim3(256), 0, (hipStream_t)stream, f, rays, ray_stride, (long)n, seg);
    if (check_launch("hf_project_kernel")) return 2;
  }
  hipLaunchKernelGGL(hf_cast_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, g, xoff, yoff, rays, ray_stride, seg_a, seg_b,
                     seg, (long)n, depth, cell, s);
  return check_launch("hf_cast_kernel");
}

// The mask of the raster under the sun direction sun_d: from every finite cell the segment from (cell centre, h + bias) along the unit
// sun vector up to the raster's maximum, walked by sr_heightfield_cast's traversal with the start cell passed through (the ray leaves
// the surface it stands on); 1 lit, 0 shadowed, NaN where the cell is empty; a start at or above the maximum is lit.
extern "C" int sr_heightfield_shadow(const float* hgt, int xsize, int ysize, double resolution, const float* blockmax, const float* gmax,
                                     int accelerate, const double* sun_d, double bias, float* out, void* stream) {
  if (check_raster("sr_heightfield_shadow", hgt, xsize, ysize, resolution)) return 1;
  SR_REQUIRE(accelerate == 0 || accelerate == 1, "sr_heightfield_shadow: accelerate must be 0 or 1 (got %d)", accelerate);
  SR_REQUIRE(gmax && out && sun_d, "sr_heightfield_shadow: null pointer");
  SR_REQUIRE(!accelerate || blockmax, "sr_heightfield_shadow: the two-level walk needs blockmax (null pointer)");
  SR_REQUIRE(isfinite(bias) && bias >= 0, "sr_heightfield_shadow: bias must be finite and >= 0 (got %g)", bias);
  const double len = sqrt(sun_d[0] * sun_d[0] + sun_d[1] * sun_d[1] + sun_d[2] * sun_d[2]);
  SR_REQUIRE(isfinite(len) && len > 0 && sun_d[2] / len > 0,
             "sr_heightfield_shadow: sun_d must be finite, non-zero and above the horizon, up > 0 (got %g, %g, %g)", sun_d[0], sun_d[1],
             sun_d[2]);
  const HfGrid g = make_grid(hgt, xsize, ysize, resolution, blockmax, gmax, accelerate);
  const long n = (long)xsize * ysize;
  hipLaunchKernelGGL(hf_shadow_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, g, sun_d[0] / len, sun_d[1] / len,
                     sun_d[2] / len, bias, n, out);
  return check_launch("hf_shadow_kernel");
}
