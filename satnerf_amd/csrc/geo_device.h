// Geodesy shared by the depth -> lat/lon/alt kernel (ray_ops.hip), the DSM kernels (dsm.hip) and the tie-point reprojection
// (depth_supervision.hip), fp64 throughout.
#pragma once
#include <hip/hip_runtime.h>

namespace sr {

// ECEF (x, y, zz) -> geodetic lat, lon (degrees), alt (m): sat_utils.ecef_to_latlon_custom (sat_utils.py:76-95).  Shared by
// latlonalt_from_ray and the tie-point reprojection (depth_supervision.hip).
__device__ __forceinline__ void ecef_to_geodetic(double x, double y, double zz, double& lat, double& lon, double& alt) {
#pragma clang fp contract(off)
  const double a = 6378137.0, e = 8.1819190842622e-2;
  const double asq = a * a, esq = e * e;
  const double b = sqrt(asq * (1 - esq));
  const double bsq = b * b;
  const double ep = sqrt((asq - bsq) / bsq);
  const double p = sqrt(x * x + y * y);
  const double th = atan2(a * zz, b * p);
  const double lo = atan2(y, x);
  const double sth = sin(th), cth = cos(th);
  const double la = atan2(zz + (ep * ep) * b * (sth * sth * sth), p - esq * a * (cth * cth * cth));
  const double sla = sin(la);
  const double N = a / sqrt(1 - esq * (sla * sla));
  alt = p / cos(la) - N;
  lon = lo * 180 / 3.141592653589793;
  lat = la * 180 / 3.141592653589793;
}

// scene point (o + d*depth) * range + center -> ECEF -> geodetic (datasets/satellite.py:246-275 + sat_utils.py:76-95).
// Contraction stays off: sr_latlonalt_from_depth's output is pinned bit for bit (tests/test_hip_dsm.py).
__device__ __forceinline__ void latlonalt_from_ray(const float* __restrict__ r, float depth, double cx, double cy, double cz, double range,
                                                   double& lat, double& lon, double& alt) {
#pragma clang fp contract(off)
  const double d = (double)depth;
  const double x = ((double)r[0] + (double)r[3] * d) * range + cx;
  const double y = ((double)r[1] + (double)r[4] * d) * range + cy;
  const double zz = ((double)r[2] + (double)r[5] * d) * range + cz;
  ecef_to_geodetic(x, y, zz, lat, lon, alt);
}

}  // namespace sr
