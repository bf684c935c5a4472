// RPC ray generation on the GPU: the (H*W, 11) ray block of one satellite image from its RPC00B camera.
//
// Replaces datasets/satellite.py:18-65 (get_rays: rpcm.RPCModel.localization of every pixel at max_alt and min_alt ->
// sat_utils.latlon_to_ecef_custom (sat_utils.py:59-74) -> origin / unit direction / near = 0 / far), :218-227 (normalize_rays) and
// :229-244 (per-image sun direction) -- numpy on the host in the reference, cached per image as a torch-saved (H*W, 8) fp32 tensor.
// One thread per pixel, everything up to the fp32 cast in fp64: the 20-term RPC00B cubics (term order of rpcm's apply_poly),
// Newton iteration on the normalised projection with a finite-difference Jacobian until the squared pixel error is < 1e-18
// (rpcm's tolerance), then the same fp32 arithmetic as the reference's in-place tensor ops for the normalisation.
#include <math.h>

#include "block_device.h"
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

// ---- ECEF bounds of one image's rays: SatelliteDataset.init_scaling_params (datasets/satellite.py:139-151) ----
// The bounds are held as fp32 order_key keys (block_device.h): min / max become exact integer atomics, so the result does not depend
// on the arrival order.
__global__ void scene_bounds_init_kernel(unsigned* keys, unsigned long long* n_bad) {
  for (int v = 0; v < 6; ++v) keys[v] = (v & 1) ? kKeyNegInf : kKeyPosInf;  // min, max per axis
  *n_bad = 0;
}

// one thread per pixel, as rpc_rays_kernel (the fp64 Newton iteration fills the register file, so nothing is carried across pixels):
// the near point o and the far point o + far * d (fp32, separate multiply and add, as the reference's tensor ops, :149-150).  A pixel
// with a non-finite coordinate counts in n_bad and touches no bound.  Lanes past n hold the neutral elements and still take part in
// the shuffles; at most one atomic per wave and value.
__global__ void __launch_bounds__(256) rpc_scene_bounds_kernel(const RpcModel m, int width, long n, double min_alt, double max_alt,
                                                              unsigned* __restrict__ keys, unsigned long long* __restrict__ n_bad) {
#pragma clang fp contract(off)
  unsigned k[6] = {kKeyPosInf, kKeyNegInf, kKeyPosInf, kKeyNegInf, kKeyPosInf, kKeyNegInf};
  unsigned bad = 0;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    float r8[8];
    rpc_ray8(m, (double)(i % width), (double)(i / width), min_alt, max_alt, r8);
    float fp[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float t = r8[7] * r8[3 + a];
      fp[a] = r8[a] + t;
      ok = ok && isfinite(r8[a]) && isfinite(fp[a]);
    }
    if (ok) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const unsigned kn = order_key(r8[a]), kf = order_key(fp[a]);
        k[2 * a] = kn < kf ? kn : kf;
        k[2 * a + 1] = kn < kf ? kf : kn;
      }
    } else {
      bad = 1;
    }
  }
  for (int off = 32; off >= 1; off >>= 1) {
    wave_minmax_step(k, off);
    bad += __shfl_xor(bad, off);
  }
  if ((threadIdx.x & 63) == 0) {
    // a stored key only ever moves towards its extreme, so a wave whose value does not beat the one it reads (however stale) cannot
    // change the result and skips the atomic: 4 M pixels otherwise queue 390 k atomics on one cache line (4.5 ms instead of 1.1)
#pragma unroll
    for (int v = 0; v < 6; ++v) {
      const unsigned cur = __hip_atomic_load(keys + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (v & 1) {
        if (k[v] > cur) atomicMax(keys + v, k[v]);
      } else {
        if (k[v] < cur) atomicMin(keys + v, k[v]);
      }
    }
    if (bad) atomicAdd(n_bad, (unsigned long long)bad);
  }
}

// keys -> floats in place; an untouched sentinel decodes to +inf (min) / -inf (max)
__global__ void scene_bounds_final_kernel(unsigned* keys) {
  float* out = reinterpret_cast<float*>(keys);
  for (int v = 0; v < 6; ++v) out[v] = from_key(keys[v]);
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
  if (load_rpc("sr_rpc_rays", rpc, m)) return 1;
  float sun[3];
  sun_direction(sun_elevation_deg, sun_azimuth_deg, sun);
  const long n = (long)width * height;
  hipLaunchKernelGGL(rpc_rays_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, m, width, n, min_alt, max_alt, (float)center[0],
                     (float)center[1], (float)center[2], (float)range, sun[0], sun[1], sun[2], rays11, rays8);
  return check_launch("rpc_rays_kernel");
}

extern "C" int sr_rpc_scene_bounds(const double* rpc, int width, int height, double min_alt, double max_alt, float* bounds6, int64_t* n_bad,
                                   void* stream) {
  SR_REQUIRE(rpc && bounds6 && n_bad, "sr_rpc_scene_bounds: null pointer");
  SR_REQUIRE(width >= 1 && height >= 1, "sr_rpc_scene_bounds: bad image size %d x %d", width, height);
  RpcModel m;
  if (load_rpc("sr_rpc_scene_bounds", rpc, m)) return 1;
  hipStream_t s = (hipStream_t)stream;
  unsigned* keys = reinterpret_cast<unsigned*>(bounds6);
  unsigned long long* bad = reinterpret_cast<unsigned long long*>(n_bad);
  const long n = (long)width * height;
  hipLaunchKernelGGL(scene_bounds_init_kernel, dim3(1), dim3(1), 0, s, keys, bad);
  if (check_launch("scene_bounds_init_kernel")) return 2;
  hipLaunchKernelGGL(rpc_scene_bounds_kernel, dim3(blocks_for(n)), dim3(256), 0, s, m, width, n, min_alt, max_alt, keys, bad);
  if (check_launch("rpc_scene_bounds_kernel")) return 2;
  hipLaunchKernelGGL(scene_bounds_final_kernel, dim3(1), dim3(1), 0, s, keys);
  return check_launch("scene_bounds_final_kernel");
}
