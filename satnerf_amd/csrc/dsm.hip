// DSM extraction for gfx950: depth -> UTM point cloud, its bounds, and the splat rasteriser that turns the
// cloud into a DSM.  All geometry is fp64.  The rasteriser accumulates in 64-bit fixed point with integer atomics, so a raster is
// bitwise the same for any arrival (and point) order, for every sigma.
#include <math.h>

#include "block_device.h"
#include "common.h"
#include "geo_device.h"  // utm_forward (and its inverse), the ECEF <-> geodetic pair

namespace sr {

// ---- UTM zone (utm.latlon_to_zone_number / utm.latitude_to_zone_letter, the rules sat_utils.py:105-106 relies on) -------------
// Longitude is first normalised to [-180, 180) as the utm package does, so lon = +180 and lon = -180 are both zone 1.
__host__ __device__ inline int utm_zone_number(double lat, double lon) {
  double m = fmod(lon, 360.0);
  if (m < 0) m += 360.0;
  lon = fmod(m + 540.0, 360.0) - 180.0;
  if (lat >= 56 && lat < 64 && lon >= 3 && lon < 12) return 32;  // Norway
  if (lat >= 72 && lat <= 84 && lon >= 0) {                       // Svalbard
    if (lon < 9) return 31;
    if (lon < 21) return 33;
    if (lon < 33) return 35;
    if (lon < 42) return 37;
  }
  const int z = (int)((lon + 180) / 6) + 1;
  return z > 60 ? 60 : z;  // lon just below 180 may round (lon + 180) up to 360
}
// band letter for -80 <= lat <= 84, 0 otherwise (84 itself is X)
__host__ __device__ inline int utm_zone_letter(double lat) {
  if (!(lat >= -80 && lat <= 84)) return 0;
  return "CDEFGHJKLMNPQRSTUVWXX"[(int)(lat + 80) >> 3];
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) utm_kernel(const double* __restrict__ lat, const double* __restrict__ lon, long n, int zone,
                                                  double* __restrict__ east, double* __restrict__ north) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  utm_forward(lat[i], lon[i], zone, east[i], north[i]);
}

// zone_out = {zone number, band letter} of ray 0's point (sat_utils.py:105-106); number 0 when that point is not finite or its
// latitude is outside [-80, 84].  A caller-given zone (> 0) replaces the number; the letter still comes from ray 0.
__global__ void depth_zone_kernel(const float* __restrict__ rays, const float* __restrict__ depth, double cx, double cy, double cz,
                                  double range, int zone, int* __restrict__ zone_out) {
  double la, lo, al;
  latlonalt_from_ray(rays, depth[0], cx, cy, cz, range, la, lo, al);
  const int letter = isfinite(lo) ? utm_zone_letter(la) : 0;
  zone_out[0] = zone > 0 ? zone : (letter ? utm_zone_number(la, lo) : 0);
  zone_out[1] = letter;
}

// one thread per ray: point -> (lat, lon, alt) by the arithmetic of latlonalt_kernel -> UTM.  Zone 0 (no usable first point)
// gives NaN eastings / northings, which every later stage skips.
__global__ void __launch_bounds__(256) depth_utm_kernel(const float* __restrict__ rays, int ray_stride, const float* __restrict__ depth,
                                                        long n, double cx, double cy, double cz, double range,
                                                        const int* __restrict__ zone_in, double* __restrict__ east,
                                                        double* __restrict__ north, double* __restrict__ alt) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double la, lo, al;
  latlonalt_from_ray(rays + i * ray_stride, depth[i], cx, cy, cz, range, la, lo, al);
  const int zone = zone_in[0];
  double e = __builtin_nan(""), nn = __builtin_nan("");
  if (zone > 0) utm_forward(la, lo, zone, e, nn);
  east[i] = e, north[i] = nn, alt[i] = al;
}

// A point takes part in bounds and raster when east, north and alt are finite and |alt| <= 2^20 m (the fixed-point range below).
constexpr double kMaxAbsAlt = 1048576.0;
__device__ __forceinline__ bool usable(double e, double nn, double al) {
  return isfinite(e) && isfinite(nn) && isfinite(al) && fabs(al) <= kMaxAbsAlt;
}

// bounds as order_key keys (block_device.h): min / max are exact integer atomics (order-independent)
__global__ void bounds_init_kernel(unsigned long long* keys) {
  keys[0] = ~0ull, keys[1] = 0, keys[2] = ~0ull, keys[3] = 0;  // min, max, min, max
}

// grid-stride min/max over usable points, reduced across the wave by shuffles, then one atomic per wave per value
__global__ void __launch_bounds__(256) bounds_kernel(const double* __restrict__ east, const double* __restrict__ north,
                                                     const double* __restrict__ alt, long n, unsigned long long* __restrict__ keys) {
  unsigned long long k[4] = {~0ull, 0, ~0ull, 0};
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const double e = east[i], nn = north[i];
    if (!usable(e, nn, alt[i])) continue;
    const unsigned long long ke = order_key(e), kn = order_key(nn);
    k[0] = ke < k[0] ? ke : k[0], k[1] = ke > k[1] ? ke : k[1];
    k[2] = kn < k[2] ? kn : k[2], k[3] = kn > k[3] ? kn : k[3];
  }
  wave_minmax(k);
  if ((threadIdx.x & 63) == 0) {
    atomicMin(keys + 0, k[0]), atomicMax(keys + 1, k[1]);
    atomicMin(keys + 2, k[2]), atomicMax(keys + 3, k[3]);
  }
}

// keys -> doubles in place; an untouched sentinel (no usable point) decodes to NaN
__global__ void bounds_final_kernel(unsigned long long* keys) {
  double* out = reinterpret_cast<double*>(keys);
  for (int v = 0; v < 4; ++v) {
    const unsigned long long k = keys[v];
    out[v] = (k == ~0ull || k == 0) ? __builtin_nan("") : from_key(k);
  }
}

// Fixed point of the accumulators: Sum w at 2^32 per unit weight (uint64), Sum w*alt at 2^24 per metre (int64, two's complement in
// a uint64 atomic).  Quantum 6e-8 m per contribution; overflow would need > 2^19 contributions at |alt| = 2^20 m in one cell.
constexpr double kWScale = 4294967296.0;  // 2^32
constexpr double kAScale = 16777216.0;    // 2^24

// one thread per point.  Cell of a point: c = floor((e - xoff) / r), j = floor((yoff - n) / r); points outside the grid are dropped.
// It adds to every in-grid cell (j + dj, c + dc), |dj|, |dc| <= radius, with w = 1 (sigma = inf) or exp(-d^2 / (2 sigma^2)), d = the
// distance in cells from the point to the target cell's centre.
__global__ void __launch_bounds__(256) splat_kernel(const double* __restrict__ east, const double* __restrict__ north,
                                                    const double* __restrict__ alt, long n, double xoff, double yoff, double res,
                                                    int xsize, int ysize, int radius, double sigma, unsigned long long* __restrict__ acc) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double e = east[i], nn = north[i], al = alt[i];
  if (!usable(e, nn, al)) return;
  const double u = (e - xoff) / res, v = (yoff - nn) / res;
  if (!(u >= 0 && u < xsize && v >= 0 && v < ysize)) return;
  const int c = (int)floor(u), j = (int)floor(v);
  const bool flat = isinf(sigma);
  const double inv2s2 = flat ? 0.0 : 1.0 / (2 * sigma * sigma);
  const unsigned long long wa_flat = (unsigned long long)llrint(al * kAScale);
  for (int dj = -radius; dj <= radius; ++dj) {
    const int jj = j + dj;
    if (jj < 0 || jj >= ysize) continue;
    for (int dc = -radius; dc <= radius; ++dc) {
      const int cc = c + dc;
      if (cc < 0 || cc >= xsize) continue;
      unsigned long long wq = (unsigned long long)kWScale, waq = wa_flat;
      if (!flat) {
        const double du = u - (cc + 0.5), dv = v - (jj + 0.5);
        const double w = exp(-(du * du + dv * dv) * inv2s2);
        wq = (unsigned long long)llrint(w * kWScale);
        waq = (unsigned long long)llrint(w * al * kAScale);
      }
      unsigned long long* cell = acc + 2 * ((long)jj * xsize + cc);
      atomicAdd(cell, wq);
      atomicAdd(cell + 1, waq);
    }
  }
}

// dsm = Sum w*alt / Sum w (NaN where Sum w = 0), weight = Sum w, both fp32
__global__ void __launch_bounds__(256) dsm_finalize_kernel(const unsigned long long* __restrict__ acc, long cells, float* __restrict__ dsm,
                                                           float* __restrict__ weight) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= cells) return;
  const unsigned long long sw = acc[2 * i];
  const long long swa = (long long)acc[2 * i + 1];
  const double w = (double)sw / kWScale;
  dsm[i] = sw ? (float)(((double)swa / kAScale) / w) : __builtin_nanf("");
  weight[i] = (float)w;
}

}  // namespace sr

using namespace sr;

extern "C" int sr_utm_zone(double lat, double lon, int* zone, int* letter) {
  SR_REQUIRE(zone && letter, "sr_utm_zone: null pointer");
  SR_REQUIRE(isfinite(lon) && lat >= -80 && lat <= 84, "sr_utm_zone: need -80 <= lat <= 84 and a finite lon (got %g, %g)", lat, lon);
  *zone = utm_zone_number(lat, lon);
  *letter = utm_zone_letter(lat);
  return 0;
}

extern "C" int sr_utm_from_latlon(const double* lat, const double* lon, int64_t n, int zone, double* east, double* north, void* stream) {
  SR_REQUIRE(zone >= 1 && zone <= 60, "sr_utm_from_latlon: zone must be in 1..60 (got %d)", zone);
  if (n <= 0) return 0;
  SR_REQUIRE(lat && lon && east && north, "sr_utm_from_latlon: null pointer");
  hipLaunchKernelGGL(utm_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, lat, lon, (long)n, zone, east, north);
  return check_launch("utm_kernel");
}

extern "C" int sr_depth_to_utm(const float* rays, int ray_stride, const float* depth, int64_t n_rays, const double* center, double range,
                               int zone, double* east, double* north, double* alt, int* zone_out, void* stream) {
  SR_REQUIRE(zone >= 0 && zone <= 60, "sr_depth_to_utm: zone must be 0 (from the first point) or 1..60 (got %d)", zone);
  if (n_rays <= 0) return 0;
  SR_REQUIRE(rays && depth && center && east && north && alt && zone_out, "sr_depth_to_utm: null pointer");
  SR_REQUIRE(ray_stride >= 6, "sr_depth_to_utm: ray_stride must be >= 6 (got %d)", ray_stride);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(depth_zone_kernel, dim3(1), dim3(1), 0, s, rays, depth, center[0], center[1], center[2], range, zone, zone_out);
  if (check_launch("depth_zone_kernel")) return 2;
  hipLaunchKernelGGL(depth_utm_kernel, dim3(blocks_for(n_rays)), dim3(256), 0, s, rays, ray_stride, depth, (long)n_rays, center[0], center[1],
                     center[2], range, zone_out, east, north, alt);
  return check_launch("depth_utm_kernel");
}

extern "C" int sr_dsm_bounds(const double* east, const double* north, const double* alt, int64_t n, double* bounds, void* stream) {
  SR_REQUIRE(bounds, "sr_dsm_bounds: null pointer");
  SR_REQUIRE(n <= 0 || (east && north && alt), "sr_dsm_bounds: null pointer");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(bounds);
  hipLaunchKernelGGL(bounds_init_kernel, dim3(1), dim3(1), 0, s, keys);
  if (check_launch("bounds_init_kernel")) return 2;
  if (n > 0) {
    const unsigned blocks = blocks_for(n) < 1024 ? blocks_for(n) : 1024;
    hipLaunchKernelGGL(bounds_kernel, dim3(blocks), dim3(256), 0, s, east, north, alt, (long)n, keys);
    if (check_launch("bounds_kernel")) return 2;
  }
  hipLaunchKernelGGL(bounds_final_kernel, dim3(1), dim3(1), 0, s, keys);
  return check_launch("bounds_final_kernel");
}

extern "C" int sr_dsm_rasterize(const double* east, const double* north, const double* alt, int64_t n, double xoff, double yoff,
                                double resolution, int xsize, int ysize, int radius, double sigma, uint64_t* acc, float* dsm, float* weight,
                                void* stream) {
  SR_REQUIRE(acc && dsm && weight, "sr_dsm_rasterize: null pointer");
  SR_REQUIRE(n <= 0 || (east && north && alt), "sr_dsm_rasterize: null pointer");
  SR_REQUIRE(xsize >= 1 && ysize >= 1, "sr_dsm_rasterize: empty grid (%d x %d)", ysize, xsize);
  SR_REQUIRE(radius >= 0 && radius <= 4, "sr_dsm_rasterize: radius must be in 0..4 (got %d)", radius);
  SR_REQUIRE(isfinite(resolution) && resolution > 0, "sr_dsm_rasterize: resolution must be finite and > 0 (got %g)", resolution);
  SR_REQUIRE(isfinite(xoff) && isfinite(yoff), "sr_dsm_rasterize: non-finite grid offset");
  SR_REQUIRE(sigma > 0, "sr_dsm_rasterize: sigma must be > 0 or inf (got %g)", sigma);
  hipStream_t s = (hipStream_t)stream;
  const int64_t cells = (int64_t)xsize * ysize;
  if (hipMemsetAsync(acc, 0, (size_t)cells * 2 * sizeof(uint64_t), s) != hipSuccess) {
    set_error("sr_dsm_rasterize: hipMemsetAsync of the accumulators failed");
    return 2;
  }
  if (n > 0) {
    hipLaunchKernelGGL(splat_kernel, dim3(blocks_for(n)), dim3(256), 0, s, east, north, alt, (long)n, xoff, yoff, resolution, xsize, ysize,
                       radius, sigma, reinterpret_cast<unsigned long long*>(acc));
    if (check_launch("splat_kernel")) return 2;
  }
  hipLaunchKernelGGL(dsm_finalize_kernel, dim3(blocks_for(cells)), dim3(256), 0, s, reinterpret_cast<const unsigned long long*>(acc),
                     (long)cells, dsm, weight);
  return check_launch("dsm_finalize_kernel");
}
