// Geodesy shared by the depth -> lat/lon/alt kernel (ray_ops.hip), the DSM kernels (dsm.hip), the RPC ray generation (rpc_device.h),
// the tie-point reprojection (depth_supervision.hip) and the nadir DSM rays (ortho.hip), fp64 throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

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

// geodetic lat, lon (degrees), alt (m) -> ECEF: sat_utils.latlon_to_ecef_custom (sat_utils.py:59-74)
__device__ __forceinline__ void geodetic_to_ecef(double lat, double lon, double alt, double& X, double& Y, double& Z) {
#pragma clang fp contract(off)
  const double rad_lat = lat * (3.141592653589793 / 180.0), rad_lon = lon * (3.141592653589793 / 180.0);
  const double a = 6378137.0, f = 1 / 298.257223563;
  const double e2 = 1 - (1 - f) * (1 - f);
  const double v = a / sqrt(1 - e2 * sin(rad_lat) * sin(rad_lat));
  X = (v + alt) * cos(rad_lat) * cos(rad_lon);
  Y = (v + alt) * cos(rad_lat) * sin(rad_lon);
  Z = (v * (1 - e2) + alt) * sin(rad_lat);
}

// ---- transverse Mercator, Krueger's series to order n^6 (Karney 2011, eqs. 7-9, 11, 35), WGS84 ---------------------------------
// UTM scale k0 = 0.9996, false easting 500 km, false northing 0 in BOTH hemispheres: the reference's "+proj=utm +zone=<n><L>"
// carries no +south, so southern points get negative northings.  Series truncation error < 5e-9 m within 3900 km of the
// central meridian (Karney 2011, section 4), i.e. far below the fp64 rounding of the inputs here.
__device__ inline void utm_forward(double lat_deg, double lon_deg, int zone, double& east, double& north) {
  const double kDeg = 3.141592653589793 / 180;
  const double a = 6378137.0, f = 1 / 298.257223563;
  const double e = sqrt(f * (2 - f));
  const double n = f / (2 - f), n2 = n * n, n3 = n2 * n, n4 = n3 * n, n5 = n4 * n, n6 = n5 * n;
  const double A = a / (1 + n) * (1 + n2 / 4 + n4 / 64 + n6 / 256);
  const double alpha[6] = {
      n / 2 - 2 * n2 / 3 + 5 * n3 / 16 + 41 * n4 / 180 - 127 * n5 / 288 + 7891 * n6 / 37800,
      13 * n2 / 48 - 3 * n3 / 5 + 557 * n4 / 1440 + 281 * n5 / 630 - 1983433 * n6 / 1935360,
      61 * n3 / 240 - 103 * n4 / 140 + 15061 * n5 / 26880 + 167603 * n6 / 181440,
      49561 * n4 / 161280 - 179 * n5 / 168 + 6601661 * n6 / 7257600,
      34729 * n5 / 80640 - 3418889 * n6 / 1995840,
      212378941 * n6 / 319334400};
  double dl = lon_deg - (6.0 * zone - 183.0);  // longitude from the central meridian, wrapped to [-180, 180)
  if (dl >= 180) dl -= 360;
  if (dl < -180) dl += 360;
  const double lam = dl * kDeg, phi = lat_deg * kDeg;
  const double tau = tan(phi);
  const double sig = sinh(e * atanh(e * tau / sqrt(1 + tau * tau)));
  const double taup = tau * sqrt(1 + sig * sig) - sig * sqrt(1 + tau * tau);  // tangent of the conformal latitude
  const double cl = cos(lam);
  const double xip = atan2(taup, cl);
  const double etap = asinh(sin(lam) / sqrt(taup * taup + cl * cl));
  double xi = xip, eta = etap;
  for (int j = 1; j <= 6; ++j) {
    xi += alpha[j - 1] * sin(2 * j * xip) * cosh(2 * j * etap);
    eta += alpha[j - 1] * cos(2 * j * xip) * sinh(2 * j * etap);
  }
  east = 500000.0 + 0.9996 * A * eta;
  north = 0.9996 * A * xi;
}

// The inverse series (Karney 2011, eqs. 11, 15, 19-21): UTM (east, north) metres in `zone` -> lat, lon degrees, same constants and
// false northing 0 as utm_forward.  tau' -> tau by a FIXED six Newton steps on tau'(tau) (Karney eqs. 19-21; converged to an ulp after
// three for |lat| < 89.9), so a lane's result never depends on its neighbours in the wave.  Non-finite input -> NaN.  lon is not
// wrapped: it is the central meridian plus an angle in (-180, 180].
__device__ __forceinline__ void utm_inverse(double east, double north, int zone, double& lat_deg, double& lon_deg) {
#pragma clang fp contract(off)
  constexpr double kRad = 180 / 3.141592653589793;
  constexpr double a = 6378137.0, f = 1 / 298.257223563, e2 = f * (2 - f);
  constexpr double n = f / (2 - f), n2 = n * n, n3 = n2 * n, n4 = n3 * n, n5 = n4 * n, n6 = n5 * n;
  constexpr double k = 0.9996 * (a / (1 + n) * (1 + n2 / 4 + n4 / 64 + n6 / 256));
  static constexpr double beta[6] = {  // a table in constant memory: the series loop below stays rolled
      n / 2 - 2 * n2 / 3 + 37 * n3 / 96 - n4 / 360 - 81 * n5 / 512 + 96199 * n6 / 604800,
      n2 / 48 + n3 / 15 - 437 * n4 / 1440 + 46 * n5 / 105 - 1118711 * n6 / 3870720,
      17 * n3 / 480 - 37 * n4 / 840 - 209 * n5 / 4480 + 5569 * n6 / 90720,
      4397 * n4 / 161280 - 11 * n5 / 504 - 830251 * n6 / 7257600,
      4583 * n5 / 161280 - 108847 * n6 / 3991680,
      20648693 * n6 / 638668800};
  const double e = sqrt(e2);
  if (!(isfinite(east) && isfinite(north))) {
    lat_deg = lon_deg = __builtin_nan("");
    return;
  }
  const double xi = north / k, eta = (east - 500000.0) / k;
  double xip = xi, etap = eta;
#pragma unroll 1
  for (int j = 1; j <= 6; ++j) {
    xip -= beta[j - 1] * sin(2 * j * xi) * cosh(2 * j * eta);
    etap -= beta[j - 1] * cos(2 * j * xi) * sinh(2 * j * eta);
  }
  const double she = sinh(etap), cxi = cos(xip);
  const double taup = sin(xip) / sqrt(she * she + cxi * cxi);  // tangent of the conformal latitude
  const double lam = atan2(she, cxi);
  double tau = taup;
#pragma unroll 1
  for (int it = 0; it < 6; ++it) {
    const double h = sqrt(1 + tau * tau);
    const double sig = sinh(e * atanh(e * tau / h));
    const double tp = tau * sqrt(1 + sig * sig) - sig * h;
    tau += (taup - tp) / sqrt(1 + tp * tp) * (1 + (1 - e2) * tau * tau) / ((1 - e2) * h);
  }
  lat_deg = atan(tau) * kRad;
  lon_deg = lam * kRad + (6.0 * zone - 183.0);
}

}  // namespace sr
