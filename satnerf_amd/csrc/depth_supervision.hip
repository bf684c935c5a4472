// Depth-supervision data from tie points on the GPU: the sparse rays, depth targets and keypoint weights
// SatelliteDataset_depth builds (datasets/satellite_depth.py:51-129) with rpcm on the host in the reference.
//
// Per image, two launches with the image's RPC00B camera passed by value: rays_at_kernel (get_rays + normalize_rays + sun at
// sub-pixel keypoints: rpc_device.h's rpc_ray8, the per-pixel body of sr_rpc_rays) and reproj_kernel (tie point ECEF -> geodetic ->
// RPC projection -> pixel distance, fp64, stored fp32 as the reference's error matrix is).  Then, once for the dataset:
// scatter_kernel records per (point, camera) the LAST observation with an integer atomicMax on its index (numpy's assignment keeps
// the last of repeated indices), point_sum_kernel adds each point's errors over the cameras in camera order in fp64, finalize_kernel
// adds the per-workgroup partials of the mean in a fixed order, weights_kernel evaluates exp(-(e / e_mean)^2) in fp32, and
// depths_kernel writes [target, weight] per observation.  Every grid depends on the sizes alone: bitwise repeatable on any CU count,
// no float atomics, no host synchronisation.
#include <limits.h>
#include <math.h>

#include "block_device.h"
#include "common.h"
#include "geo_device.h"
#include "rpc_device.h"

namespace sr {
namespace dsup {

constexpr int kThreads = 256;
constexpr int kMaxPartials = 2048;  // workgroups (= partial slots) of the per-point sum: grid-strided beyond that

inline long point_partials(int64_t n_pts) { return partial_slots(n_pts, kThreads, kMaxPartials); }

// scratch: winner (n_pts, n_cams) ints, rounded to 256 bytes | part P doubles (base == nullptr: sizes only)
struct Scratch { int* winner; double* part; int64_t bytes; };
inline Scratch scratch_layout(void* base, int64_t n_pts, int n_cams) {
  ScratchCarver c(base);
  int* winner = c.take<int>(n_pts * n_cams, 256);
  double* part = c.take<double>(point_partials(n_pts), 8);
  return {winner, part, c.bytes()};
}

// get_rays + normalize_rays + sun (datasets/satellite_depth.py:64-75) at n keypoints colrow = (col, row) fp64 pairs
__global__ void __launch_bounds__(kThreads) rays_at_kernel(const RpcModel m, const double* __restrict__ colrow, long n, double min_alt,
                                                           double max_alt, float cx, float cy, float cz, float range, float sx, float sy,
                                                           float sz, float* __restrict__ rays11) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  float r8[8];
  rpc_ray8(m, colrow[2 * i], colrow[2 * i + 1], min_alt, max_alt, r8);
  normalize_ray11(r8, cx, cy, cz, range, sx, sy, sz, rays11 + i * 11);
}

// satellite_depth.py:116-122: |pts2d - rpc.projection(ecef_to_latlon_custom(pts3d[idx]))| in fp64, rounded to fp32 once
__global__ void __launch_bounds__(kThreads) reproj_kernel(const RpcModel m, const double* __restrict__ colrow, const int64_t* __restrict__ idx,
                                                          long n, const double* __restrict__ pts3d, int64_t n_pts, float* __restrict__ err) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t p = idx[i];
  if (p < 0 || p >= n_pts) {  // the host checks the indices; a bad one reads nothing
    err[i] = __builtin_nanf("");
    return;
  }
  double lat, lon, alt, col, row;
  ecef_to_geodetic(pts3d[3 * p], pts3d[3 * p + 1], pts3d[3 * p + 2], lat, lon, alt);
  rpc_project(m, lon, lat, alt, col, row);
  const double dc = colrow[2 * i] - col, dr = colrow[2 * i + 1] - row;
  err[i] = (float)sqrt(dc * dc + dr * dr);  // np.linalg.norm(axis=1) of a (K, 2) fp64 array: sqrt(dc^2 + dr^2)
}

// reprojection_errors[idx, t] = errs (satellite_depth.py:123): the winner of (point, camera) is the observation with the largest
// index (+ 1; 0 = none), i.e. the last one in JSON order, whatever order the atomics land in
__global__ void __launch_bounds__(kThreads) scatter_kernel(const int64_t* __restrict__ idx, const int64_t* __restrict__ cam, long n,
                                                           int64_t n_pts, int n_cams, int* __restrict__ winner) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t p = idx[i], t = cam[i];
  if (p < 0 || p >= n_pts || t < 0 || t >= n_cams) return;
  atomicMax(winner + p * n_cams + t, (int)(i + 1));
}

// e[p] = sum over cameras t = 0, 1, ... of the winning fp32 error (fp64 accumulation, one rounding to fp32; satellite_depth.py:125),
// and each workgroup's fp64 partial of sum_p e[p] (of the fp32 values) for the mean (:126).  Points p = g * 256 + t + k * (P * 256).
__global__ void __launch_bounds__(kThreads) point_sum_kernel(const int* __restrict__ winner, const float* __restrict__ err, int64_t n_pts,
                                                             int n_cams, float* __restrict__ e, double* __restrict__ part) {
#pragma clang fp contract(off)
  const int64_t P = gridDim.x;
  double s[1] = {0.0};
  for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < n_pts; p += P * kThreads) {
    double acc = 0.0;
    const int* wrow = winner + p * n_cams;
    for (int t = 0; t < n_cams; ++t) {
      const int k = wrow[t];
      if (k > 0) acc += (double)err[k - 1];
    }
    const float ef = (float)acc;
    e[p] = ef;
    s[0] += (double)ef;
  }
  block_sum(s);
  if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}

// e_mean = (sum of the P partials: strided_sum, then block_sum's fixed tree) / n_pts, rounded to fp32.  One workgroup.
__global__ void __launch_bounds__(kThreads) finalize_kernel(const double* __restrict__ part, int P, int64_t n_pts, float* __restrict__ e_mean) {
#pragma clang fp contract(off)
  double s[1];
  strided_sum(part, P, s);
  block_sum(s);
  if (threadIdx.x == 0) e_mean[0] = (float)(s[0] / (double)n_pts);
}

// weights = np.exp(-(e / e_mean) ** 2) on fp32 arrays (satellite_depth.py:127)
__global__ void __launch_bounds__(kThreads) weights_kernel(const float* __restrict__ e, int64_t n_pts, const float* __restrict__ e_mean,
                                                           float* __restrict__ w) {
#pragma clang fp contract(off)
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= n_pts) return;
  const float q = e[p] / e_mean[0];
  w[p] = expf(-(q * q));
}

// depths = [|normalised fp32 tie point - ray origin|, w[idx]] (satellite_depth.py:77-91): the fp64 ECEF point is cast to fp32 first,
// then -= center, /= range and the norm in fp32, as the reference's tensor ops
__global__ void __launch_bounds__(kThreads) depths_kernel(const float* __restrict__ rays11, const double* __restrict__ pts3d,
                                                          const int64_t* __restrict__ idx, long n, int64_t n_pts, float cx, float cy,
                                                          float cz, float range, const float* __restrict__ w, float* __restrict__ depths) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t p = idx[i];
  if (p < 0 || p >= n_pts) {
    depths[2 * i] = depths[2 * i + 1] = __builtin_nanf("");
    return;
  }
  const float* o = rays11 + i * 11;
  const float q0 = ((float)pts3d[3 * p] - cx) / range, q1 = ((float)pts3d[3 * p + 1] - cy) / range, q2 = ((float)pts3d[3 * p + 2] - cz) / range;
  const float d0 = q0 - o[0], d1 = q1 - o[1], d2 = q2 - o[2];
  depths[2 * i] = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
  depths[2 * i + 1] = w ? w[p] : 0.f;
}

}  // namespace dsup
}  // namespace sr

using namespace sr;
using namespace sr::dsup;

extern "C" int sr_rpc_rays_at(const double* rpc, const double* colrow, int64_t n, double min_alt, double max_alt, const double* center,
                              double range, double sun_elevation_deg, double sun_azimuth_deg, float* rays11, void* stream) {
  SR_REQUIRE(center && (n == 0 || (colrow && rays11)), "sr_rpc_rays_at: null pointer");
  SR_REQUIRE(n >= 0 && n < ((int64_t)1 << 40), "sr_rpc_rays_at: n must be in 0..2^40 (got %lld)", (long long)n);
  SR_REQUIRE(range > 0, "sr_rpc_rays_at: scene range must be positive");
  RpcModel m;
  if (load_rpc("sr_rpc_rays_at", rpc, m)) return 1;
  if (n == 0) return 0;
  float sun[3];
  sun_direction(sun_elevation_deg, sun_azimuth_deg, sun);
  hipLaunchKernelGGL(rays_at_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream, m, colrow, (long)n, min_alt, max_alt,
                     (float)center[0], (float)center[1], (float)center[2], (float)range, sun[0], sun[1], sun[2], rays11);
  return check_launch("rays_at_kernel");
}

extern "C" int sr_reprojection_errors(const double* rpc, const double* colrow, const int64_t* pts3d_idx, int64_t n, const double* pts3d,
                                      int64_t n_pts, float* err, void* stream) {
  SR_REQUIRE(n == 0 || (colrow && pts3d_idx && pts3d && err), "sr_reprojection_errors: null pointer");
  SR_REQUIRE(n >= 0 && n < ((int64_t)1 << 40) && n_pts >= 0, "sr_reprojection_errors: bad sizes n %lld, n_pts %lld", (long long)n,
             (long long)n_pts);
  RpcModel m;
  if (load_rpc("sr_reprojection_errors", rpc, m)) return 1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(reproj_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream, m, colrow, pts3d_idx, (long)n, pts3d, n_pts, err);
  return check_launch("reproj_kernel");
}

extern "C" int sr_keypoint_weights_scratch(int64_t n_pts, int n_cams, int64_t* bytes) {
  SR_REQUIRE(bytes, "sr_keypoint_weights_scratch: null pointer");
  SR_REQUIRE(n_pts >= 1 && n_cams >= 1 && n_pts <= ((int64_t)1 << 36) / n_cams,
             "sr_keypoint_weights_scratch: need n_pts >= 1, n_cams >= 1 and n_pts * n_cams <= 2^36 (got %lld x %d)", (long long)n_pts, n_cams);
  *bytes = scratch_layout(nullptr, n_pts, n_cams).bytes;
  return 0;
}

extern "C" int sr_keypoint_weights(const int64_t* pts3d_idx, const int64_t* cam, const float* err, int64_t n, int64_t n_pts, int n_cams,
                                   void* scratch, int64_t scratch_bytes, float* e, float* w, float* e_mean, void* stream) {
  int64_t need = 0;
  if (sr_keypoint_weights_scratch(n_pts, n_cams, &need)) return 1;
  SR_REQUIRE(scratch && e && w && e_mean && (n == 0 || (pts3d_idx && cam && err)), "sr_keypoint_weights: null pointer");
  SR_REQUIRE(n >= 0 && n < INT_MAX, "sr_keypoint_weights: n must be in 0..%d (got %lld)", INT_MAX - 1, (long long)n);
  if (require_scratch("sr_keypoint_weights", scratch_bytes, need)) return 1;
  hipStream_t s = (hipStream_t)stream;
  const Scratch sc = scratch_layout(scratch, n_pts, n_cams);
  const long P = point_partials(n_pts);
  SR_REQUIRE(hipMemsetAsync(sc.winner, 0, (size_t)n_pts * n_cams * sizeof(int), s) == hipSuccess, "sr_keypoint_weights: hipMemsetAsync failed");
  if (n > 0) {
    hipLaunchKernelGGL(scatter_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, pts3d_idx, cam, (long)n, n_pts, n_cams, sc.winner);
    if (check_launch("scatter_kernel")) return 2;
  }
  hipLaunchKernelGGL(point_sum_kernel, dim3((unsigned)P), dim3(kThreads), 0, s, (const int*)sc.winner, err, n_pts, n_cams, e, sc.part);
  if (check_launch("point_sum_kernel")) return 2;
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(kThreads), 0, s, (const double*)sc.part, (int)P, n_pts, e_mean);
  if (check_launch("finalize_kernel")) return 2;
  hipLaunchKernelGGL(weights_kernel, dim3(blocks_for(n_pts)), dim3(kThreads), 0, s, (const float*)e, n_pts, (const float*)e_mean, w);
  return check_launch("weights_kernel");
}

extern "C" int sr_tie_point_depths(const float* rays11, const double* pts3d, const int64_t* pts3d_idx, int64_t n, int64_t n_pts,
                                   const double* center, double range, const float* w, float* depths, void* stream) {
  SR_REQUIRE(center && (n == 0 || (rays11 && pts3d && pts3d_idx && depths)), "sr_tie_point_depths: null pointer");
  SR_REQUIRE(n >= 0 && n < ((int64_t)1 << 40) && n_pts >= 0, "sr_tie_point_depths: bad sizes n %lld, n_pts %lld", (long long)n,
             (long long)n_pts);
  SR_REQUIRE(range > 0, "sr_tie_point_depths: scene range must be positive");
  if (n == 0) return 0;
  hipLaunchKernelGGL(depths_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream, rays11, pts3d, pts3d_idx, (long)n, n_pts,
                     (float)center[0], (float)center[1], (float)center[2], (float)range, w, depths);
  return check_launch("depths_kernel");
}
