// Fused Sat-NeRF MLP forward in the PARITY arithmetic (bf16x3: hi + lo planes, three MFMAs per k-step, <= 1e-4 of the reference),
// width 256, inference and the one-launch render pass, second generation: as mlp_fwd2.inc the 4,218-MFMA core between fc_net.0 and
// the output activations is ONE hand-placed instruction stream (csrc/gen/fwd_core3.py -> mlp_fwd3_core_a*.inc).  A wave owns 32 sample
// points, runs alone on its SIMD with the unified 512-register file (hi planes + accumulators in VGPRs, lo planes + A fragments + head
// accumulator in AGPRs), 4 waves per workgroup; LDS ring of 64 units (hi + lo KiB of one k-step) fed by LDS-DMA rows of 4 units.
// Replaces (as mlp_fwd.inc): models/satnerf.py:20-40 + SatNeRF.forward models/satnerf.py:156-208 + Siren models/nerf.py:23-33, and with
// REND rendering.py:62-81 + models/satnerf.py:42-79.  Included after mlp_fwd.inc by the p3 translation units.  SAVE = SR_FMT16 is the
// training forward of the parity mode: the unorm16 phases / bf16 feats of mlp_layout.h's 16-bit workspaces are written by the stream.
#pragma once
#include "mlp_fwd_io.inc"

namespace sr {
inline namespace SR_FEAT_NS {

#if SR_FEAT == 256

typedef unsigned int u32x16_3 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x32_3 __attribute__((ext_vector_type(32)));

constexpr int kRing3 = 64;  // ring units of 2 KiB (gen/fwd_core3.py R)
#ifndef SR_CORE3_A1  // timing experiments compile other generator outputs
#define SR_CORE3_A1 "mlp_fwd3_core_a1.inc"
#define SR_CORE3_A2 "mlp_fwd3_core_a2.inc"
#define SR_CORE3_A1S16 "mlp_fwd3_core_a1s16.inc"
#define SR_CORE3_A2S16 "mlp_fwd3_core_a2s16.inc"
#endif

__device__ __forceinline__ u32x32_3 cat8(const uint4* f) {
  u32x32_3 v;
#pragma unroll
  for (int i = 0; i < 8; ++i) v[4 * i] = f[i].x, v[4 * i + 1] = f[i].y, v[4 * i + 2] = f[i].z, v[4 * i + 3] = f[i].w;
  return v;
}

template <int AUXS, bool REND, int SAVE = 0>
__global__ void __launch_bounds__(256) satnerf_fwd3_kernel(const FwdParams prm) {
  constexpr int NW = kFwdWavesParity;  // (gen/fwd_core3.py feeds the ring in rows of 4)
  constexpr int AK = act_ksteps(AUXS);  // workspace fragments per tile (SAVE)
  static_assert(SAVE == 0 || SAVE == SR_FMT16, "the parity mode saves 16-bit workspaces");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem;
  float4* l0w = reinterpret_cast<float4*>(smem + kRing3 * 2048);
  float* r_z = reinterpret_cast<float*>(smem + kRing3 * 2048 + kFeat * sizeof(float4));

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5;
#ifdef SR_CORE_TIMING
  const uint64_t t_kernel0 = __builtin_amdgcn_s_memtime();
#endif

  for (int i = tid; i < kFeat; i += NW * 64) l0w[i] = prm.l0[i];

  // this lane's sample point (mlp_fwd_io.inc)
  const PointIn in = point_setup<REND, NW>(prm, r_z, wave, lane);
  const long tile = in.tile;
  const float x = in.x, y = in.y, zc = in.zc;

  // aux fragment(s), hi and lo planes (mlp_fwd_io.inc aux_values: the slots)
  u32x16_3 auxv = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};  // [hi a0, hi a1, lo a0, lo a1]
  {
    float av[AUXS][8];
    aux_values<AUXS>(prm, in, lane, av);
#pragma unroll
    for (int a = 0; a < AUXS; ++a)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t hw, lw;
        split_bf16x2(av[a][2 * q], av[a][2 * q + 1], hw, lw);
        auxv[4 * a + q] = hw, auxv[8 + 4 * a + q] = lw;
      }
  }
  uint4* save = SAVE ? prm.acts + (tile * AK) * 64 + lane : nullptr;
  if constexpr (SAVE != 0) {
#pragma unroll
    for (int a = 0; a < AUXS; ++a) ws_store(save + a * 64, make_uint4(auxv[4 * a], auxv[4 * a + 1], auxv[4 * a + 2], auxv[4 * a + 3]));
  }

  __syncthreads();  // l0w visible; every global load of the prologue has been waited for (the core's LDS-DMA counts start clean)

  // ---- fc_net.0 (K = 3) on VALU, fp32, w0 = 30 folded into l0 ------------------------------------------
  Frags<3, kKS> cur;
#pragma unroll
  for (int s = 0; s < kKS; s += 2) {
    f32x16 pre;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int ss = s + (g >> 3), j = g & 7;
      const float4 w = l0w[(ss * 2 + h) * 8 + j];
      pre[g] = __builtin_fmaf(w.x, x, __builtin_fmaf(w.y, y, __builtin_fmaf(w.z, zc, w.w)));
    }
    pack_tile<3, ACT_SIN, SAVE>(pre, cur.hi[s], cur.hi[s + 1], cur.lo[s], cur.lo[s + 1], save_at<SAVE>(save, AUXS, s));
  }

  // ---- the core: fc_net.2 .. fc_net.14, feats / sigma, the three heads -----------------------------------
  u32x32_3 xh0 = cat8(cur.hi), xh1 = cat8(cur.hi + 8), xl0 = cat8(cur.lo), xl1 = cat8(cur.lo + 8);
  const uint32_t ring_addr = lds_addr_of(ring);
  const uint32_t vl0 = ring_addr + (uint32_t)lane * 16u, vl1 = vl0 + 65536u;
  uint32_t voff = (uint32_t)wave * 1024u + (uint32_t)lane * 16u;
  const uint32_t wb = __builtin_amdgcn_readfirstlane(ring_addr + (uint32_t)wave * 2048u);
  const uint64_t sh = uniform64(prm.stream_hi), sl = uniform64(prm.stream_lo);
  f32x16 acc;
  float sig;
  uint32_t m0save;
#ifdef SR_CORE_TIMING
  const uint64_t t_core0 = __builtin_amdgcn_s_memtime();
  const uint64_t r_core0 = __builtin_amdgcn_s_memrealtime();
#endif
  // SAVE: this lane's workspace offset (tile base + lane * 16; the stream advances it fragment by fragment)
  uint32_t soff = (uint32_t)((unsigned long)tile * AK * 1024ul) + (uint32_t)lane * 16u;
  const uint64_t ab = uniform64(prm.acts);
#define SR_CORE3_OUTS                                                                                                                  \
  "+{v[0:31]}"(xh0), "+{v[32:63]}"(xh1), "+{v[64:95]}"(xl0), "+{v[96:127]}"(xl1), "+{v[144:159]}"(auxv), "={v[128:143]}"(acc),        \
      "={v168}"(sig), "+{v171}"(voff), [m0save] "=&s"(m0save)
#define SR_CORE3_INS "{v169}"(vl0), "{v170}"(vl1), [sh] "s"(sh), [sl] "s"(sl), [wb] "s"(wb), [wave] "s"(wave)
  if constexpr (AUXS == 1 && SAVE == 0) {
    asm volatile(
#include SR_CORE3_A1
        : SR_CORE3_OUTS
        : SR_CORE3_INS
        :
#include "mlp_fwd3_core_clobbers.inc"
    );
  } else if constexpr (SAVE == 0) {
    asm volatile(
#include SR_CORE3_A2
        : SR_CORE3_OUTS
        : SR_CORE3_INS
        :
#include "mlp_fwd3_core_clobbers.inc"
    );
  } else if constexpr (AUXS == 1) {
    asm volatile(
#include SR_CORE3_A1S16
        : SR_CORE3_OUTS, "+{v188}"(soff)
        : SR_CORE3_INS, [ab] "s"(ab)
        :
#include "mlp_fwd3_core_clobbers_s16.inc"
    );
  } else {
    asm volatile(
#include SR_CORE3_A2S16
        : SR_CORE3_OUTS, "+{v188}"(soff)
        : SR_CORE3_INS, [ab] "s"(ab)
        :
#include "mlp_fwd3_core_clobbers_s16.inc"
    );
  }
#undef SR_CORE3_OUTS
#undef SR_CORE3_INS

#ifdef SR_CORE_TIMING
  core_timing_store(prm, tile, lane, t_kernel0, t_core0, r_core0);
  return;
#endif
  write_outputs<REND, NW>(prm, in, acc, sig, r_z, wave, lane);
}

template <int AUXS, bool REND, int SAVE = 0>
int launch_fwd3(const FwdParams& p, hipStream_t st) {
  return launch_fwd_kernel(satnerf_fwd3_kernel<AUXS, REND, SAVE>, "satnerf_fwd3_kernel", kFwdWavesParity, (size_t)kRing3 * 2048 + kFeat * sizeof(float4),
                           REND ? kRendFloats : 0, p, st);
}

// entry of the (3, AUXS) translation units: the generated core for inference, the render pass and the 16-bit training forward unless
// SATNERF_FWD_V1=1 selects the hipcc-scheduled kernel (A/B; it also keeps what the stream's 32-bit workspace offsets cannot address,
// and a render launch with a workspace: mlp_fwd_io.inc fwd_route)
template <int AUXS>
int launch_fwd3_any(const FwdParams& p, int save_fmt, hipStream_t st) {
  const FwdRoute route = fwd_route(p, save_fmt, SR_FMT16, act_ksteps(AUXS), false);
  if (route != FwdRoute::Core) return route == FwdRoute::Refused ? 1 : launch_fwd<3, AUXS>(p, save_fmt, st);
  if (save_fmt == SR_FMT16) return launch_fwd3<AUXS, false, SR_FMT16>(p, st);
  return p.rend.rays != nullptr ? launch_fwd3<AUXS, true>(p, st) : launch_fwd3<AUXS, false>(p, st);
}

#endif  // SR_FEAT == 256

}  // inline namespace SR_FEAT_NS
}  // namespace sr
