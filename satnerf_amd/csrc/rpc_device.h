// RPC00B camera arithmetic shared by the ray generation of whole images (rpc_rays.hip) and of tie-point keypoints
// (depth_supervision.hip), fp64 throughout with contraction off: sr_rpc_rays' output is unchanged by the move into this header.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include "common.h"
#include "geo_device.h"

namespace sr {

struct RpcModel {  // host-filled, passed by value (90 doubles)
  double row_num[20], row_den[20], col_num[20], col_den[20];
  double row_offset, col_offset, lat_offset, lon_offset, alt_offset, row_scale, col_scale, lat_scale, lon_scale, alt_scale;
};

// the 90 host doubles of entry point fn -> m; 1 + sr_last_error on a null pointer or a zero scale
inline int load_rpc(const char* fn, const double* rpc, RpcModel& m) {
  SR_REQUIRE(rpc, "%s: null rpc", fn);
  static_assert(sizeof(RpcModel) == 90 * sizeof(double), "RpcModel layout = the 90 host doubles");
  memcpy(&m, rpc, sizeof(m));
  SR_REQUIRE(m.row_scale != 0 && m.col_scale != 0 && m.lat_scale != 0 && m.lon_scale != 0 && m.alt_scale != 0, "%s: zero RPC scale", fn);
  return 0;
}

// an image's sun direction (datasets/satellite.py:199-211) from its elevation and azimuth in degrees: fp64 on the host, rounded once
inline void sun_direction(double el_deg, double az_deg, float sun[3]) {
  const double el = el_deg * (3.141592653589793 / 180.0), az = az_deg * (3.141592653589793 / 180.0);
  sun[0] = (float)(sin(az) * cos(el)), sun[1] = (float)(cos(az) * cos(el)), sun[2] = (float)sin(el);
}

__device__ __forceinline__ double rpc_poly(const double* c, double x, double y, double z) {  // x = lat, y = lon, z = alt (normalised)
#pragma clang fp contract(off)
  return c[0] + c[1] * y + c[2] * x + c[3] * z + c[4] * y * x + c[5] * y * z + c[6] * x * z + c[7] * y * y + c[8] * x * x + c[9] * z * z +
         c[10] * x * y * z + c[11] * y * y * y + c[12] * y * x * x + c[13] * y * z * z + c[14] * y * y * x + c[15] * x * x * x +
         c[16] * x * z * z + c[17] * y * y * z + c[18] * x * x * z + c[19] * z * z * z;
}

// image (normalised col, row) at normalised altitude z -> normalised (lat x, lon y)
__device__ inline void rpc_localize(const RpcModel& m, double nc, double nr, double z, double& x, double& y) {
#pragma clang fp contract(off)
  x = 0.0, y = 0.0;
  const double eps = 1e-6;
  for (int it = 0; it < 100; ++it) {
    const double c0 = rpc_poly(m.col_num, x, y, z) / rpc_poly(m.col_den, x, y, z);
    const double r0 = rpc_poly(m.row_num, x, y, z) / rpc_poly(m.row_den, x, y, z);
    const double ec = nc - c0, er = nr - r0;
    if (ec * ec + er * er < 1e-18) break;
    const double cx = rpc_poly(m.col_num, x + eps, y, z) / rpc_poly(m.col_den, x + eps, y, z);
    const double rx = rpc_poly(m.row_num, x + eps, y, z) / rpc_poly(m.row_den, x + eps, y, z);
    const double cy = rpc_poly(m.col_num, x, y + eps, z) / rpc_poly(m.col_den, x, y + eps, z);
    const double ry = rpc_poly(m.row_num, x, y + eps, z) / rpc_poly(m.row_den, x, y + eps, z);
    const double j11 = (cx - c0) / eps, j12 = (cy - c0) / eps, j21 = (rx - r0) / eps, j22 = (ry - r0) / eps;
    const double det = j11 * j22 - j12 * j21;
    x = x + (ec * j22 - er * j12) / det;
    y = y + (er * j11 - ec * j21) / det;
  }
}

// ground (lon, lat degrees, alt m) -> image (col, row): rpcm.RPCModel.projection, the forward RPC00B model
__device__ __forceinline__ void rpc_project(const RpcModel& m, double lon, double lat, double alt, double& col, double& row) {
#pragma clang fp contract(off)
  const double x = (lat - m.lat_offset) / m.lat_scale, y = (lon - m.lon_offset) / m.lon_scale, z = (alt - m.alt_offset) / m.alt_scale;
  col = rpc_poly(m.col_num, x, y, z) / rpc_poly(m.col_den, x, y, z) * m.col_scale + m.col_offset;
  row = rpc_poly(m.row_num, x, y, z) / rpc_poly(m.row_den, x, y, z) * m.row_scale + m.row_offset;
}

// get_rays (datasets/satellite.py:18-65) of one image point (col, row): localised at max_alt (ray origin) and min_alt, converted to
// ECEF, r8 = the fp32 row [o(3) d(3) near = 0 far]
__device__ __forceinline__ void rpc_ray8(const RpcModel& m, double col, double row, double min_alt, double max_alt, float r8[8]) {
#pragma clang fp contract(off)
  const double nc = (col - m.col_offset) / m.col_scale, nr = (row - m.row_offset) / m.row_scale;
  double P[2][3];
#pragma unroll
  for (int k = 0; k < 2; ++k) {  // k = 0: max_alt (closest to the camera = origin), k = 1: min_alt
    const double alt = k == 0 ? max_alt : min_alt;
    double x, y;
    rpc_localize(m, nc, nr, (alt - m.alt_offset) / m.alt_scale, x, y);
    geodetic_to_ecef(x * m.lat_scale + m.lat_offset, y * m.lon_scale + m.lon_offset, alt, P[k][0], P[k][1], P[k][2]);
  }
  const double d0 = P[1][0] - P[0][0], d1 = P[1][1] - P[0][1], d2 = P[1][2] - P[0][2];
  const double far = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  r8[0] = (float)P[0][0], r8[1] = (float)P[0][1], r8[2] = (float)P[0][2];
  r8[3] = (float)(d0 / far), r8[4] = (float)(d1 / far), r8[5] = (float)(d2 / far), r8[6] = 0.f, r8[7] = (float)far;
}

// normalize_rays in the tensor's own fp32 (datasets/satellite.py:218-227) + the image's sun direction (:199-211): o = 11 floats
__device__ __forceinline__ void normalize_ray11(const float r8[8], float cx, float cy, float cz, float range, float sx, float sy, float sz,
                                                float* __restrict__ o) {
#pragma clang fp contract(off)
  o[0] = (r8[0] - cx) / range, o[1] = (r8[1] - cy) / range, o[2] = (r8[2] - cz) / range;
  o[3] = r8[3], o[4] = r8[4], o[5] = r8[5];
  o[6] = r8[6] / range, o[7] = r8[7] / range;
  o[8] = sx, o[9] = sy, o[10] = sz;
}

}  // namespace sr
