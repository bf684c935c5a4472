// RPC ray generation on the GPU: the (H*W, 11) ray block of one satellite image from its RPC00B camera.
//
// Replaces datasets/satellite.py:18-65 (get_rays: rpcm.RPCModel.localization of every pixel at max_alt and min_alt ->
// sat_utils.latlon_to_ecef_custom (sat_utils.py:59-74) -> origin / unit direction / near = 0 / far), :218-227 (normalize_rays) and
// :229-244 (per-image sun direction) -- numpy on the host in the reference, cached per image as a torch-saved (H*W, 8) fp32 tensor.
// One thread per pixel, everything up to the fp32 cast in fp64: the 20-term RPC00B cubics (term order of rpcm's apply_poly),
// Newton iteration on the normalised projection with a finite-difference Jacobian until the squared pixel error is < 1e-18
// (rpcm's tolerance), then the same fp32 arithmetic as the reference's in-place tensor ops for the normalisation.
#include <math.h>
#include <string.h>

#include "common.h"
#include "rpc_device.h"

namespace sr {

__global__ void __launch_bounds__(256) rpc_rays_kernel(const RpcModel m, int width, long n, double min_alt, double max_alt, float cx, float cy,
                                                      float cz, float range, float sx, float sy, float sz, float* __restrict__ rays11,
                                                      float* __restrict__ rays8) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float r8[8];
  rpc_ray8(m, (double)(i % width), (double)(i / width), min_alt, max_alt, r8);  // np.meshgrid(arange(w), arange(h)) flattened, :193-194
  if (rays8) {
#pragma unroll
    for (int c = 0; c < 8; ++c) rays8[i * 8 + c] = r8[c];  // the reference's <cache_dir>/<img_id>.data content
  }
  if (rays11) normalize_ray11(r8, cx, cy, cz, range, sx, sy, sz, rays11 + i * 11);
}

}  // namespace sr

using namespace sr;

extern "C" int sr_rpc_rays(const double* rpc, int width, int height, double min_alt, double max_alt, const double* center, double range,
                           double sun_elevation_deg, double sun_azimuth_deg, float* rays11, float* rays8, void* stream) {
  SR_REQUIRE(rpc && center, "sr_rpc_rays: null pointer");
  SR_REQUIRE(rays11 || rays8, "sr_rpc_rays: no output requested");
  SR_REQUIRE(width >= 1 && height >= 1, "sr_rpc_rays: bad image size %d x %d", width, height);
  SR_REQUIRE(range > 0, "sr_rpc_rays: scene range must be positive");
  RpcModel m;
  static_assert(sizeof(RpcModel) == 90 * sizeof(double), "RpcModel layout = the 90 host doubles");
  memcpy(&m, rpc, sizeof(m));
  SR_REQUIRE(m.row_scale != 0 && m.col_scale != 0 && m.lat_scale != 0 && m.lon_scale != 0 && m.alt_scale != 0, "sr_rpc_rays: zero RPC scale");
  const double el = sun_elevation_deg * (3.141592653589793 / 180.0), az = sun_azimuth_deg * (3.141592653589793 / 180.0);
  const long n = (long)width * height;
  hipLaunchKernelGGL(rpc_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m, width, n, min_alt, max_alt,
                     (float)center[0], (float)center[1], (float)center[2], (float)range, (float)(sin(az) * cos(el)), (float)(cos(az) * cos(el)),
                     (float)sin(el), rays11, rays8);
  return check_launch("rpc_rays_kernel");
}
