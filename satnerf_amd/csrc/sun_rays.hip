// Geometric sun visibility for gfx950: the ray from a rendered surface point towards the sun, in the scene's
// normalised ECEF frame, and the per-pixel relighting with the transparency the density leaves along it.  The reference's solar
// correction pass (rendering.py:102-108) adds the east / north / up vector of rays[:, 8:11] to an ECEF origin and starts at the camera
// ray's origin; here the vector is turned into the local tangent frame of the surface point and the ray starts at that point.
// All geometry is fp64 with contraction off; a ray is rounded to fp32 once.  One thread per ray doing everything: no LDS, no atomics,
// no cross-lane traffic, so a result depends on its own ray only.
#include <math.h>

#include "common.h"
#include "geo_device.h"

namespace sr {

struct SunFrame {  // host-filled, passed by value
  double cx, cy, cz, range, max_alt, bias_abs, bias_rel;
  float sx, sy, sz;
  int call_sun;  // 1: (sx, sy, sz) is the call's sun vector; 0: each ray carries its own in columns 8..10
};

// Row i of `out`: [P(3) dir(3) near far sun(3)], or the zero-length row [o(3) d(3) 0 0 sun(3)] of an invalid ray (valid[i] = 0).
// lat / lon / alt are latlonalt_from_ray's, i.e. sr_latlonalt_from_depth's bits.
__global__ void __launch_bounds__(256) sun_rays_kernel(const SunFrame g, const float* __restrict__ rays, int ray_stride,
                                                      const float* __restrict__ depth, long n, float* __restrict__ out, int out_stride,
                                                      unsigned char* __restrict__ valid, double* __restrict__ latlonalt) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* r = rays + i * ray_stride;
  const float o0 = r[0], o1 = r[1], o2 = r[2], d0 = r[3], d1 = r[4], d2 = r[5], near0 = r[6], far0 = r[7];
  const float s0 = g.call_sun ? g.sx : r[8], s1 = g.call_sun ? g.sy : r[9], s2 = g.call_sun ? g.sz : r[10];
  const float tf = depth[i];
  const double t = (double)tf;
  const double px = (double)o0 + (double)d0 * t, py = (double)o1 + (double)d1 * t, pz = (double)o2 + (double)d2 * t;
  double lat, lon, alt;
  latlonalt_from_ray(r, tf, g.cx, g.cy, g.cz, g.range, lat, lon, alt);
  if (latlonalt) latlonalt[i] = lat, latlonalt[n + i] = lon, latlonalt[2 * n + i] = alt;
  const double ex = px * g.range + g.cx, ey = py * g.range + g.cy, ez = pz * g.range + g.cz;
  const double se = (double)s0, sn = (double)s1, su = (double)s2;
  const double len = sqrt(se * se + sn * sn + su * su);
  const double he = se / len, hn = sn / len, hu = su / len;
  const bool ok = isfinite(tf) && isfinite(ex) && isfinite(ey) && isfinite(ez) && isfinite(len) && len > 0 && hu > 0;
  float* w = out + i * out_stride;
  w[8] = s0, w[9] = s1, w[10] = s2;
  valid[i] = ok ? 1 : 0;
  if (!ok) {
    w[0] = o0, w[1] = o1, w[2] = o2, w[3] = d0, w[4] = d1, w[5] = d2, w[6] = 0.f, w[7] = 0.f;
    return;
  }
  const double phi = lat * (3.141592653589793 / 180.0), lam = lon * (3.141592653589793 / 180.0);
  const double sphi = sin(phi), cphi = cos(phi), slam = sin(lam), clam = cos(lam);
  // east (-sin lam, cos lam, 0), north (-sin phi cos lam, -sin phi sin lam, cos phi), up (cos phi cos lam, cos phi sin lam, sin phi)
  const double dx = he * -slam + hn * -(sphi * clam) + hu * (cphi * clam);
  const double dy = he * clam + hn * -(sphi * slam) + hu * (cphi * slam);
  const double dz = hn * cphi + hu * sphi;
  const double L = (g.max_alt - alt) / (hu * g.range);  // where the ray reaches max_alt on the local tangent plane
  const double nr = g.bias_abs + g.bias_rel * ((double)far0 - (double)near0);
  const double fr = L > nr ? L : nr;
  w[0] = (float)px, w[1] = (float)py, w[2] = (float)pz;
  w[3] = (float)dx, w[4] = (float)dy, w[5] = (float)dz;
  w[6] = (float)nr, w[7] = (float)fr;
}

// rgb = clamp(albedo * (v + (1 - v) * sky), 0, 1) per channel in fp32, one rounding per operation; a NaN stays a NaN.
__global__ void __launch_bounds__(256) sun_shade_kernel(const float* __restrict__ albedo, int albedo_stride, const float* __restrict__ sky,
                                                       int sky_stride, const float* __restrict__ vis, long n, float* __restrict__ rgb,
                                                       int rgb_stride) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = vis[i];
  const float q = 1.f - v;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float k = q * sky[i * sky_stride + c];
    const float irr = v + k;
    const float x = albedo[i * albedo_stride + c] * irr;
    rgb[i * rgb_stride + c] = x != x ? x : fminf(fmaxf(x, 0.f), 1.f);  // fminf / fmaxf alone would drop the NaN
  }
}

}  // namespace sr

using namespace sr;

extern "C" int sr_sun_rays(const float* rays, int ray_stride, const float* depth, int64_t n, const double* center, double range, double max_alt,
                           const float* sun_d, double bias_abs, double bias_rel, float* out, int out_stride, uint8_t* valid,
                           double* latlonalt, void* stream) {
  SR_REQUIRE(ray_stride >= 11, "sr_sun_rays: ray_stride must be >= 11 (got %d)", ray_stride);
  SR_REQUIRE(out_stride >= 11, "sr_sun_rays: out_stride must be >= 11 (got %d)", out_stride);
  SR_REQUIRE(isfinite(range) && range > 0, "sr_sun_rays: scene range must be finite and > 0 (got %g)", range);
  SR_REQUIRE(isfinite(max_alt), "sr_sun_rays: max_alt must be finite (got %g)", max_alt);
  SR_REQUIRE(isfinite(bias_abs) && bias_abs >= 0 && isfinite(bias_rel) && bias_rel >= 0,
             "sr_sun_rays: bias_abs and bias_rel must be finite and >= 0 (got %g, %g)", bias_abs, bias_rel);
  SR_REQUIRE(center, "sr_sun_rays: null pointer");
  SR_REQUIRE(isfinite(center[0]) && isfinite(center[1]) && isfinite(center[2]), "sr_sun_rays: non-finite scene center");
  SunFrame g;
  g.cx = center[0], g.cy = center[1], g.cz = center[2], g.range = range, g.max_alt = max_alt, g.bias_abs = bias_abs, g.bias_rel = bias_rel;
  g.sx = g.sy = g.sz = 0.f, g.call_sun = sun_d != nullptr;
  if (sun_d) {
    g.sx = sun_d[0], g.sy = sun_d[1], g.sz = sun_d[2];
    SR_REQUIRE(isfinite(g.sx) && isfinite(g.sy) && isfinite(g.sz) && (g.sx != 0 || g.sy != 0 || g.sz != 0) && g.sz > 0,
               "sr_sun_rays: sun_d must be finite, non-zero and above the horizon, up > 0 (got %g, %g, %g)", g.sx, g.sy, g.sz);
  }
  if (n <= 0) return 0;
  SR_REQUIRE(rays && depth && out && valid, "sr_sun_rays: null pointer");
  hipLaunchKernelGGL(sun_rays_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, g, rays, ray_stride, depth, (long)n, out,
                     out_stride, valid, latlonalt);
  return check_launch("sun_rays_kernel");
}

extern "C" int sr_sun_shade(const float* albedo, int albedo_stride, const float* sky, int sky_stride, const float* vis, int64_t n, float* rgb,
                            int rgb_stride, void* stream) {
  SR_REQUIRE(albedo_stride >= 3 && sky_stride >= 3 && rgb_stride >= 3, "sr_sun_shade: strides must be >= 3 (got %d, %d, %d)", albedo_stride,
             sky_stride, rgb_stride);
  if (n <= 0) return 0;
  SR_REQUIRE(albedo && sky && vis && rgb, "sr_sun_shade: null pointer");
  hipLaunchKernelGGL(sun_shade_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, albedo, albedo_stride, sky, sky_stride, vis,
                     (long)n, rgb, rgb_stride);
  return check_launch("sun_shade_kernel");
}
