// Nadir DSM rays for gfx950: the inverse UTM projection (eval_s2p.lonlat_from_utm, eval_s2p.py:37-44) and
// the vertical rays through the cell centres of a DSM grid -- get_rays + normalize_rays (datasets/satellite.py:18-65,218-227) with the
// RPC localisation replaced by the grid's own lon / lat.  All geometry is fp64 with contraction off; a ray is rounded to fp32 once.
// One thread per point / cell doing everything: no LDS, no atomics, no cross-lane traffic, so a result depends on its own cell only.
#include <math.h>

#include "common.h"
#include "geo_device.h"

namespace sr {

__global__ void __launch_bounds__(256) utm_inverse_kernel(const double* __restrict__ east, const double* __restrict__ north, long n, int zone,
                                                          double* __restrict__ lat, double* __restrict__ lon) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  utm_inverse(east[i], north[i], zone, lat[i], lon[i]);
}

struct OrthoGrid {  // host-filled, passed by value
  double xoff, yoff, res;
  int xsize, zone;
  double max_alt, cx, cy, cz, range;
  float far, sx, sy, sz;
};

// cell i = (row j = i / xsize, column c = i % xsize), row 0 at the top (dsm.DSM's layout).  The origin sits at max_alt on the cell
// centre's vertical and is normalised in fp64; the direction is the inward ellipsoid normal, written down analytically (the difference
// of the ECEF points at max_alt and min_alt is the same vector with ~1e-11 of cancellation error).
__global__ void __launch_bounds__(256) ortho_rays_kernel(const OrthoGrid g, long n, float* __restrict__ rays, int row_stride,
                                                        double* __restrict__ latlon) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int j = (int)(i / g.xsize), c = (int)(i % g.xsize);
  const double e = g.xoff + (c + 0.5) * g.res, nn = g.yoff - (j + 0.5) * g.res;
  double lat, lon, X, Y, Z;
  utm_inverse(e, nn, g.zone, lat, lon);
  geodetic_to_ecef(lat, lon, g.max_alt, X, Y, Z);
  const double phi = lat * (3.141592653589793 / 180.0), lam = lon * (3.141592653589793 / 180.0);
  const double cphi = cos(phi);
  float* r = rays + i * row_stride;
  r[0] = (float)((X - g.cx) / g.range), r[1] = (float)((Y - g.cy) / g.range), r[2] = (float)((Z - g.cz) / g.range);
  r[3] = (float)(-(cphi * cos(lam))), r[4] = (float)(-(cphi * sin(lam))), r[5] = (float)(-sin(phi));
  r[6] = 0.f, r[7] = g.far;
  r[8] = g.sx, r[9] = g.sy, r[10] = g.sz;
  if (latlon) latlon[2 * i] = lat, latlon[2 * i + 1] = lon;
}

}  // namespace sr

using namespace sr;

extern "C" int sr_utm_to_latlon(const double* east, const double* north, int64_t n, int zone, double* lat, double* lon, void* stream) {
  SR_REQUIRE(zone >= 1 && zone <= 60, "sr_utm_to_latlon: zone must be in 1..60 (got %d)", zone);
  if (n <= 0) return 0;
  SR_REQUIRE(east && north && lat && lon, "sr_utm_to_latlon: null pointer");
  hipLaunchKernelGGL(utm_inverse_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, east, north, (long)n, zone, lat, lon);
  return check_launch("utm_inverse_kernel");
}

extern "C" int sr_ortho_rays(double xoff, double yoff, double resolution, int xsize, int ysize, int zone, double min_alt, double max_alt,
                             const double* center, double range, const float* sun_d, float* rays, int row_stride, double* latlon,
                             void* stream) {
  SR_REQUIRE(zone >= 1 && zone <= 60, "sr_ortho_rays: zone must be in 1..60 (got %d)", zone);
  SR_REQUIRE(xsize >= 1 && ysize >= 1, "sr_ortho_rays: empty grid (%d x %d)", ysize, xsize);
  SR_REQUIRE((int64_t)xsize * ysize < ((int64_t)1 << 31), "sr_ortho_rays: grid %d x %d has 2^31 cells or more", ysize, xsize);
  SR_REQUIRE(isfinite(resolution) && resolution > 0, "sr_ortho_rays: resolution must be finite and > 0 (got %g)", resolution);
  SR_REQUIRE(isfinite(xoff) && isfinite(yoff), "sr_ortho_rays: non-finite grid offset");
  SR_REQUIRE(isfinite(min_alt) && isfinite(max_alt) && min_alt < max_alt, "sr_ortho_rays: need finite min_alt < max_alt (got %g, %g)", min_alt,
             max_alt);
  SR_REQUIRE(isfinite(range) && range > 0, "sr_ortho_rays: scene range must be finite and > 0 (got %g)", range);
  SR_REQUIRE(row_stride >= 11, "sr_ortho_rays: row_stride must be >= 11 (got %d)", row_stride);
  SR_REQUIRE(center && sun_d && rays, "sr_ortho_rays: null pointer");
  OrthoGrid g;
  g.xoff = xoff, g.yoff = yoff, g.res = resolution, g.xsize = xsize, g.zone = zone;
  g.max_alt = max_alt, g.cx = center[0], g.cy = center[1], g.cz = center[2], g.range = range;
  g.far = (float)((max_alt - min_alt) / range), g.sx = sun_d[0], g.sy = sun_d[1], g.sz = sun_d[2];
  const long n = (long)xsize * ysize;
  hipLaunchKernelGGL(ortho_rays_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, g, n, rays, row_stride, latlon);
  return check_launch("ortho_rays_kernel");
}
