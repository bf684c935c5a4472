// Kernel parameter blocks shared by the API translation unit and the kernel instantiations (independent of the trunk width:
// they stay outside the per-width inline namespace of mlp_layout.h).
#pragma once
#include <stdlib.h>

#include "common.h"

namespace sr {

// waves per workgroup of the fused forward kernels, each wave one 32-point tile: the kernels take (or static_assert) their NW from
// these, sr_render_points_per_block answers from them
constexpr int kFwdWaves256 = 8;     // width 256, bf16 / fp16 operands: two waves per SIMD
constexpr int kFwdWavesParity = 4;  // width 256, parity mode: one wave per SIMD with the 512-register file
constexpr int kFwdWaves512 = 4;     // width 512: likewise

// SATNERF_FWD_V1=1: every forward launch of the process runs the compiler-scheduled kernel (A/B against the generated cores)
inline bool fwd_v1_forced() {
  static const bool v1 = [] { const char* e = getenv("SATNERF_FWD_V1"); return e && e[0] == '1'; }();
  return v1;
}

// the fused render pass around the MLP (csrc/mlp_fwd.inc REND): stratified sampling in the prologue, the sky head and the
// sigma->alpha compositing of the workgroup's rays in the epilogue.  rays == NULL: plain MLP launch.
struct RenderParams {
  const float* rays;       // (N, ray_stride >= 11): o(3) d(3) near far sun(3)
  int ray_stride;
  const float* z_in;       // (N,S) given depths (fine pass), or NULL: stratified from u / the in-kernel RNG
  const float* u;          // (N,S) jitter, or NULL: Philox(seed, step_counter[0])
  unsigned long long seed;
  float* step_counter;
  int tick;
  const float* noise;      // (N,S) or NULL
  float noise_std;
  int sky_hidden;
  const float *w1, *b1, *w2, *b2;
  float* z_out;            // (N,S) or NULL
  float* sky;              // (N,3)
  float* weights;          // (N,S)
  float* transp;           // (N,S)
  float* depth;            // (N)
  float* rgb;              // (N,3)
  long n_rays;
  long bank_chunks;        // > 0: rays / ts hold bank_chunks x n_rays rows, this launch renders chunk step_counter[0] % bank_chunks
};

// the training epilogue of the fused render pass (sr_satnerf_render_train): with target != NULL the compositing of a ray is followed, in
// the same wave, by the colour loss and the closed-form compositing backward (ray_device.h render_loss_ray) -- the launch then writes what
// the dX kernel consumes instead of weights / transparency
struct TrainParams {
  const float* target;     // (N,3) ground-truth colours, or NULL: plain render
  const float* sched;      // device-side schedule block ([2] != 0: SNerfLoss warm-up epochs) or NULL
  float beta_min;
  float* loss_parts;       // one partial sum per workgroup
  float* rgb;              // (N,3) rendered colour (logging) or NULL
  float* d_sigma;          // (N,S)
  float* d_albedo;         // (N,S,3)
  float* d_sun;            // (N,S)
  float* g_beta;           // (N,S)
  float* d_sky;            // (N,3)
  // the batch sampler inside the launch (include/satrender.h sr_train_args): rays / ts / target are the resident bank, ray r reads row
  // gather_idx[cursor[0] * n_rays + r]; the compositing wave copies the row out for the later launches of the step
  const long long* gather_idx;
  float* cursor;
  unsigned batches;
  float* out_rays;         // (N,11)
  float* out_rgbs;         // (N,3)
  long long* out_ts;       // (N)
};

struct FwdParams {
  sr_mlp_inputs in;
  RenderParams rend;
  TrainParams train;
  const char* stream_hi;
  const char* stream_lo;
  const float4* l0;
  float* albedo;
  float* sigma;
  float* sun_v;
  float* beta;
  uint4* acts;
  int tau;
};

// ---- the launchers of the per-variant translation units, declared here alone; mlp_api.hip's table kFwdUnits is what chooses among them.
// p = bf16 operands, h = fp16 (SR_MODE_F16), p3 = parity (SR_MODE_BF16X3); a1 / a2 = aux steps (mlp_layout.h aux_steps(tau))
using FwdLaunch = int (*)(const FwdParams&, int save_fmt, hipStream_t);  // a unit's whole kernel (mlp_fwd*_{p1,p3,h1}a*.hip)
using FwdGeomLaunch = int (*)(const FwdParams&, hipStream_t);           // its trunk-and-sigma build (mlp_fwdg_*.hip, mlp_fwd512g_g*.hip)
int launch_fwd_p1a1(const FwdParams&, int, hipStream_t);
int launch_fwd_p1a2(const FwdParams&, int, hipStream_t);
int launch_fwd_h1a1(const FwdParams&, int, hipStream_t);
int launch_fwd_h1a2(const FwdParams&, int, hipStream_t);
int launch_fwd_p3a1(const FwdParams&, int, hipStream_t);
int launch_fwd_p3a2(const FwdParams&, int, hipStream_t);
int launch_fwd512_p1a1(const FwdParams&, int, hipStream_t);
int launch_fwd512_p1a2(const FwdParams&, int, hipStream_t);
int launch_fwd512_h1a1(const FwdParams&, int, hipStream_t);
int launch_fwd512_h1a2(const FwdParams&, int, hipStream_t);
int launch_fwd_geom_p1a1(const FwdParams&, hipStream_t);
int launch_fwd_geom_p1a2(const FwdParams&, hipStream_t);
int launch_fwd_geom_h1a1(const FwdParams&, hipStream_t);
int launch_fwd_geom_h1a2(const FwdParams&, hipStream_t);
int launch_fwd512_geom_p1a1(const FwdParams&, hipStream_t);
int launch_fwd512_geom_p1a2(const FwdParams&, hipStream_t);
int launch_fwd512_geom_h1a1(const FwdParams&, hipStream_t);
int launch_fwd512_geom_h1a2(const FwdParams&, hipStream_t);
long fwd512_stream_pieces_a1();  // FwdStream<AUXS>::total_pieces() of the 512-wide layout (mlp_fwd512_p1a*.hip)
long fwd512_stream_pieces_a2();

struct BwdParams {
  const float* g_albedo;  // upstream gradients of the per-point outputs (any may be null = 0)
  const float* g_sigma;
  const float* g_sun;
  const float* g_beta;
  const float* albedo;    // forward outputs (activation derivatives of the heads)
  const float* sigma;
  const float* sun_v;
  const float* beta;
  const uint4* acts;      // saved activations, act_ksteps(auxs) fragments per 32-point tile
  uint4* dpre;            // out: pre-activation gradients, kDpFrags fragments per tile
  uint4* emax;            // out (SR_FMT8): the table of exponent maxima behind the workspace's last tile (mlp_layout.h), one entry per 4 tiles
  float* d_t;             // out: (P, tau) gradient of the embedding vector per point (may be null)
  const char* stream;     // transposed weight stream (bf16)
  long n_points;
  int tau;
  int auxs;
};

}  // namespace sr
