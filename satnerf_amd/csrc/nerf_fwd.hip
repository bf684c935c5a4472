// C ABI of the fused classic-NeRF forward (nerf_fwd.inc): argument checks + the two launches.
#include "nerf_fwd.inc"

using namespace sr;

constexpr int kNerfMaxSamples = kNerfPoints;  // a workgroup composites whole rays: one ray's samples must fit its 256 points

extern "C" int64_t sr_nerf_stream_elems(int feat) { return feat == kFeat ? NerfStream::total_pieces() * 512 : -1; }

extern "C" int sr_nerf_render_max_samples(void) { return kNerfMaxSamples; }

extern "C" int sr_nerf_mlp_fwd(const float* xyz, int xyz_stride, const float* dirs, int dir_stride, int row_div, int64_t n_points, int feat,
                               const uint16_t* stream_hi, float* rgb, float* sigma, void* stream) {
  SR_REQUIRE(feat == kFeat, "sr_nerf_mlp_fwd: feat=%d unsupported (the fused classic NeRF is built for %d)", feat, kFeat);
  SR_REQUIRE(xyz_stride >= 3 && dir_stride >= 3 && row_div >= 1, "sr_nerf_mlp_fwd: bad layout (xyz stride %d, dir stride %d, row_div %d)", xyz_stride,
             dir_stride, row_div);
  if (n_points <= 0) return 0;
  SR_REQUIRE(xyz && dirs && stream_hi && rgb && sigma, "sr_nerf_mlp_fwd: null pointer");
  NerfParams p{};
  p.stream = (const char*)stream_hi;
  p.xyz = xyz, p.dirs = dirs, p.xyz_stride = xyz_stride, p.dir_stride = dir_stride, p.row_div = row_div, p.n_points = n_points;
  p.rgb = rgb, p.sigma = sigma;
  return nerf_launch<false>(p, (hipStream_t)stream);
}

extern "C" int sr_nerf_render_fwd(const float* rays, int ray_stride, int64_t n_rays, int n_samples, const float* u, const float* z_in,
                                  const float* noise, float noise_std, int feat, const uint16_t* stream_hi, float* z_out, float* rgb, float* depth,
                                  float* weights, float* transparency, void* stream) {
  SR_REQUIRE(feat == kFeat, "sr_nerf_render_fwd: feat=%d unsupported (the fused classic NeRF is built for %d)", feat, kFeat);
  SR_REQUIRE(ray_stride >= 8, "sr_nerf_render_fwd: ray_stride=%d, classic rays have 8 columns", ray_stride);
  SR_REQUIRE(n_samples >= 2 && n_samples <= kNerfMaxSamples, "sr_nerf_render_fwd: n_samples=%d must lie in 2..%d (sr_nerf_render_max_samples)", n_samples,
             kNerfMaxSamples);
  if (n_rays <= 0) return 0;
  SR_REQUIRE((u != nullptr) != (z_in != nullptr), "sr_nerf_render_fwd: exactly one of u (stratified depths) and z_in (given depths) is required");
  SR_REQUIRE(rays && stream_hi && weights && transparency, "sr_nerf_render_fwd: null pointer (rays, stream, weights and transparency are required)");
  NerfParams p{};
  p.stream = (const char*)stream_hi;
  p.rays = rays, p.ray_stride = ray_stride, p.n_samples = n_samples, p.rays_per_block = kNerfPoints / n_samples, p.n_rays = n_rays;
  p.u = u, p.z_in = z_in, p.noise = noise, p.noise_std = noise_std;
  p.z_out = z_out, p.r_rgb = rgb, p.depth = depth, p.weights = weights, p.transp = transparency;
  return nerf_launch<true>(p, (hipStream_t)stream);
}
