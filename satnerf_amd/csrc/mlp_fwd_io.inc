// The shell of the generated-core forward kernels (mlp_fwd2.inc, mlp_fwd3.inc, mlp_fwd512g.inc), everything around their instruction
// streams that is not a kernel's own geometry:
//   aux_values         the fp32 slot values of a lane's aux fragment(s), in front of the stream
//   write_outputs      the output activations / the one-launch render and training epilogue behind the stream
//   core_timing_store  the SR_CORE_TIMING experiment's three floats
//   fwd_route          host (with mlp_params.h fwd_v1_forced): generated core, compiler-scheduled kernel (mlp_fwd.inc) or error, for the three launch_fwd*_any
// The rest of the shell is in mlp_fwd.inc, beside the compiler-scheduled kernel that shares it (point_setup, aux_ws_bf16,
// launch_fwd_kernel), and in mlp_device.h (uniform64).  NW = waves per workgroup (a workgroup's NW * 32 consecutive points are whole
// rays under REND).
#pragma once
#include <stdlib.h>

#include "mlp_fwd.inc"

namespace sr {

// Where a forward launch runs.  The generated core takes inference and its one native save format, while the stream's 32-bit workspace
// offsets reach the whole workspace (tail waves included); everything else is the compiler-scheduled kernel's, which has no training
// epilogue.  Today's callers (native format, units per tile, may a render launch save):
//   launch_fwd_any     256, bf16 / f16   SR_FMT8    act8_units   yes (the one-launch training forward)
//   launch_fwd3_any    256, parity       SR_FMT16   act_ksteps   no  (falls back; launch_fwd refuses a render launch that saves)
//   launch_fwd512_any  512, bf16 / f16   SR_FMT8    act8_units   yes
//   save_fmt   render launch   workspace   SATNERF_FWD_V1 | route
//   0          any             -           unset          | Core
//   native     no              < 4 GiB     unset          | Core
//   native     yes             < 4 GiB     unset          | Core if a render launch may save, else Scheduled
//   native     any             >= 4 GiB    unset          | Scheduled
//   other      any             any         unset          | Scheduled
//   any        any             any         1              | Scheduled
//   ... and Scheduled with train.target set                | Refused (error set; the parity mode has no training launch, mlp_api.hip)
enum class FwdRoute { Core, Scheduled, Refused };
inline FwdRoute fwd_route(const FwdParams& p, int save_fmt, int native_fmt, int units_per_tile, bool rend_may_save) {
  const unsigned long ws_bytes = (unsigned long)ws_tiles(p.in.n_points) * units_per_tile * 1024ul;
  const bool rend = p.rend.rays != nullptr;
  if (!fwd_v1_forced() && (save_fmt == 0 || (save_fmt == native_fmt && (rend_may_save || !rend) && ws_bytes < (1ul << 32)))) return FwdRoute::Core;
  if (p.train.target != nullptr) {
    set_error("sr_satnerf_render_train: no fused training forward for this configuration (SATNERF_FWD_V1, a 16-bit workspace or >= 4 GiB of it): use the separate launches");
    return FwdRoute::Refused;
  }
  return FwdRoute::Scheduled;
}

inline namespace SR_FEAT_NS {

// this lane's fp32 values of the aux fragment(s): slots [sun(3), 1, xyz(3), 0 | t(0..7) | t(8..15) | t(16..23)], av[a][j] = slot
// 16 a + 8 h + j.  The shells pack their operand formats from these (tests/test_hip_fwd_reference.py pins the layout).
// h is derived here, with its range stated: handed in as a plain int the helper is simplified before it is inlined without knowing
// that h is 0 or 1, and the callers' fc_net.0 table reads behind it then came out with one address add each (+128..256 instructions).
template <int AUXS>
__device__ __forceinline__ void aux_values(const FwdParams& prm, const PointIn& in, int lane, float (&av)[AUXS][8]) {
  const int h = lane >> 5;
  __builtin_assume(h == 0 || h == 1);
  const float *sn = in.sn, *te = in.te;
  const float x = in.x, y = in.y, zc = in.zc;
#pragma unroll
  for (int a = 0; a < AUXS; ++a)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int q = 16 * a + 8 * h + j;  // aux slot
      float val = 0.f;
      if (q >= 8) { const int ti = q - 8; val = ti < prm.tau ? te[ti < prm.tau ? ti : 0] : 0.f; }
      av[a][j] = val;
    }
  if (h == 0) { av[0][0] = sn[0], av[0][1] = sn[1], av[0][2] = sn[2], av[0][3] = 1.f, av[0][4] = x, av[0][5] = y, av[0][6] = zc, av[0][7] = 0.f; }
}

#ifdef SR_CORE_TIMING  // experiments (tools/ab_core.sh -DSR_CORE_TIMING): shader cycles of the core / the prologue per wave instead of sigma / sun_v
__device__ __forceinline__ void core_timing_store(const FwdParams& prm, long tile, int lane, uint64_t t_kernel0, uint64_t t_core0, uint64_t r_core0) {
  const uint64_t t_core1 = __builtin_amdgcn_s_memtime();
  const uint64_t r_core1 = __builtin_amdgcn_s_memrealtime();
  if (lane == 0 && prm.sigma && prm.sun_v) {
    prm.sigma[tile] = (float)(t_core1 - t_core0);
    prm.sun_v[tile] = (float)(t_core0 - t_kernel0);
    if (prm.beta) prm.beta[tile] = (float)(r_core1 - r_core0);  // constant 100 MHz ticks
  }
}
#endif

// acc = the 5-row head accumulator (rows 0..2 albedo logits, 3 sun visibility logit on lanes < 32; row 0 = beta on lanes >= 32),
// sig = sigma pre-activation.  REND: r_z .. = kRendFloats * NW * 32 floats of LDS (depth, sigma, sun, albedo, beta per point).
// prm.train.target != NULL (the training forward, n_samples <= 64): wave w renders ray w, w + NW, ... of the workgroup AND takes the colour loss
// and the compositing backward of that ray (render_loss_ray): the launch writes d_sigma / d_albedo / d_sun / g_beta / d_sky and one loss
// partial per workgroup instead of weights / transparency -- what sr_ray_setup + this kernel + sr_render_loss did in three launches.
// GEOM (the geometry cores, gen/fwd_core.py heads=False): `acc` is not read and sigma is the one per-point value.  REND then keeps
// kRendFloatsGeom floats per point in LDS (depth, sigma) and each wave composites its rays sigma-only -- composite_ray with no albedo is
// the reduction of the full render's depth / weights / transparency, in the same order -- with no sky head and no colour.
constexpr int kRendFloats = 7, kRendFloatsGeom = 2;
template <bool REND, int NW, bool GEOM = false>
__device__ __forceinline__ void write_outputs(const FwdParams& prm, const PointIn& in, const f32x16& acc, float sig, float* r_z, int wave, int lane) {
  constexpr int P = NW * 32;
  float *r_sigma = r_z + P, *r_sun = r_z + 2 * P, *r_albedo = r_z + 3 * P, *r_beta = r_z + 6 * P;
  const int h = lane >> 5, pl = lane & 31;
  const long pt = in.pt, r = in.r, rg = in.rg;
  const bool valid = in.valid;
  if constexpr (GEOM && REND) {
    const float sg = softplus_f(sig);
    if (h == 0) {
      r_sigma[wave * 32 + pl] = sg;
      if (valid && prm.sigma) prm.sigma[pt] = sg;
    }
    __syncthreads();
    const int S = prm.in.n_samples;
    const int rays_here = P / S;  // host contract: S divides P
    for (int lr = wave; lr < rays_here; lr += NW) {
      const long ray = (long)blockIdx.x * rays_here + lr;
      if (ray >= prm.rend.n_rays) break;
      composite_ray(r_z + lr * S, r_sigma + lr * S, prm.rend.noise ? prm.rend.noise + ray * S : nullptr, prm.rend.noise_std, nullptr, nullptr, 0.f,
                    0.f, 0.f, S, lane, 1, prm.rend.weights + ray * S, prm.rend.transp + ray * S, prm.rend.depth ? prm.rend.depth + ray : nullptr,
                    nullptr);
    }
  } else if constexpr (GEOM) {
    if (valid && h == 0 && prm.sigma) prm.sigma[pt] = softplus_f(sig);
  } else if constexpr (REND) {
    const float sg = softplus_f(sig);
    if (h == 0) {
      r_sigma[wave * 32 + pl] = sg;
      const float al0 = sigmoid_f(acc[0]) * 1.002f - 0.001f, al1 = sigmoid_f(acc[1]) * 1.002f - 0.001f, al2 = sigmoid_f(acc[2]) * 1.002f - 0.001f;
      const float sv = sigmoid_f(acc[3]);
      float* la = r_albedo + (wave * 32 + pl) * 3;
      la[0] = al0, la[1] = al1, la[2] = al2;
      r_sun[wave * 32 + pl] = sv;
      if (valid) {
        if (prm.sigma) prm.sigma[pt] = sg;
        if (prm.albedo) {
          float* a = prm.albedo + pt * 3;
          a[0] = al0, a[1] = al1, a[2] = al2;
        }
        if (prm.sun_v) prm.sun_v[pt] = sv;
      }
    } else {
      const float bt = softplus_f(acc[0]);
      r_beta[wave * 32 + pl] = bt;
      if (valid && prm.beta) prm.beta[pt] = bt;
    }
    __syncthreads();
    const int S = prm.in.n_samples;
    const int rays_here = P / S;  // host contract: S divides P
    const bool train = prm.train.target != nullptr;
    const bool warm = prm.train.sched != nullptr && prm.train.sched[2] != 0.f;  // (include/satrender.h `sched`: [2] = SNerfLoss warm-up)
    float loss_part = 0.f;
    for (int lr = wave; lr < rays_here; lr += NW) {
      const long ray = (long)blockIdx.x * rays_here + lr;
      if (ray >= prm.rend.n_rays) break;
      const bool gathered = prm.train.gather_idx != nullptr;
      const long ray_g = gathered ? (long)prm.train.gather_idx[in.first + ray] : ray + (rg - r);
      const float* rr = prm.rend.rays + ray_g * prm.rend.ray_stride;
      if (gathered) {  // the batch row, for the step's later launches (what sr_gather_batch wrote)
        if (lane < 11) prm.train.out_rays[ray * 11 + lane] = rr[lane];
        else if (lane < 14) prm.train.out_rgbs[ray * 3 + (lane - 11)] = prm.train.target[ray_g * 3 + (lane - 11)];
        else if (lane == 14) prm.train.out_ts[ray] = prm.in.ts[ray_g];
      }
      float k0, k1, k2;
      sky_ray(rr[8], rr[9], rr[10], prm.rend.sky_hidden, prm.rend.w1, prm.rend.b1, prm.rend.w2, prm.rend.b2, lane, k0, k1, k2);
      if (lane == 0 && prm.rend.sky) prm.rend.sky[ray * 3] = k0, prm.rend.sky[ray * 3 + 1] = k1, prm.rend.sky[ray * 3 + 2] = k2;
      if (train) {
        loss_part += render_loss_ray(r_z + lr * S, r_sigma + lr * S, prm.rend.noise ? prm.rend.noise + ray * S : nullptr, prm.rend.noise_std,
                                     r_albedo + lr * S * 3, r_sun + lr * S, r_beta + lr * S, k0, k1, k2, prm.train.target + (gathered ? ray_g : ray) * 3, ray,
                                     prm.rend.n_rays, S, lane, prm.train.beta_min, warm, prm.train.rgb ? prm.train.rgb + ray * 3 : nullptr,
                                     prm.train.d_sigma + ray * S, prm.train.d_albedo + ray * S * 3, prm.train.d_sun + ray * S,
                                     prm.train.g_beta + ray * S, prm.train.d_sky + ray * 3);
        continue;
      }
      composite_ray(r_z + lr * S, r_sigma + lr * S, prm.rend.noise ? prm.rend.noise + ray * S : nullptr, prm.rend.noise_std,
                    r_albedo + lr * S * 3, r_sun + lr * S, k0, k1, k2, S, lane, 1, prm.rend.weights + ray * S, prm.rend.transp + ray * S,
                    prm.rend.depth ? prm.rend.depth + ray : nullptr, prm.rend.rgb ? prm.rend.rgb + ray * 3 : nullptr);
    }
    if (train) {  // the workgroup's share of the batch-mean loss: the waves' sums meet in the (now free) first floats of r_z
      __syncthreads();
      if (lane == 0) r_z[wave] = loss_part;
      __syncthreads();
      if (threadIdx.x == 0) {
        float sum = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) sum += r_z[w];
        prm.train.loss_parts[blockIdx.x] = sum;
        // the launch's counters move on now: every wave of every workgroup that has arrived read them at its start
        if (prm.rend.tick) tick_at_exit(prm.rend.step_counter, in.step_read);
        if (prm.train.gather_idx != nullptr) tick_at_exit(prm.train.cursor, in.cursor_read, prm.train.batches);
      }
    }
  } else if (valid) {
    if (h == 0) {
      if (prm.sigma) prm.sigma[pt] = softplus_f(sig);
      if (prm.albedo) {
        float* a = prm.albedo + pt * 3;
        a[0] = sigmoid_f(acc[0]) * 1.002f - 0.001f;  // models/satnerf.py:195, rgb_padding = 0.001
        a[1] = sigmoid_f(acc[1]) * 1.002f - 0.001f;
        a[2] = sigmoid_f(acc[2]) * 1.002f - 0.001f;
      }
      if (prm.sun_v) prm.sun_v[pt] = sigmoid_f(acc[3]);
    } else if (prm.beta) {
      prm.beta[pt] = softplus_f(acc[0]);
    }
  }
}

}  // inline namespace SR_FEAT_NS
}  // namespace sr
