// Fused Sat-NeRF MLP forward at WIDTH 512 (opt.py:50's default fc_units, what run_all.sh trains sat-nerf with), single-pass bf16 / fp16
// operands, inference and the one-launch render pass, second generation: the 5,370-MFMA core between fc_net.0 and the output
// activations is ONE hand-placed instruction stream (csrc/gen/fwd_core512.py -> mlp_fwd512_core_a*.inc).  One activation vector of a
// 32-point wave is 128 registers, so the wave runs alone on its SIMD with the unified 512-register file (X + accumulators in VGPRs;
// Y, the A-fragment ring and the head accumulator in AGPRs), 4 waves per workgroup, LDS ring of 144 pieces fed by rows of 4.
// Replaces (as mlp_fwd.inc): models/satnerf.py:20-40 + SatNeRF.forward models/satnerf.py:156-208 + Siren models/nerf.py:23-33, and with
// REND rendering.py:62-81 + models/satnerf.py:42-79.  Included after mlp_fwd.inc by the 512-wide translation units.  SAVE = SR_FMT8 is
// the training forward: the PHASE8 / MX8 encoding of mlp_layout.h's 8-bit workspaces and their stores are part of the stream.
#pragma once
#include "mlp_fwd_io.inc"

namespace sr {
inline namespace SR_FEAT_NS {

#if SR_FEAT == 512

typedef unsigned int u32x8_5 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x32_5 __attribute__((ext_vector_type(32)));

constexpr int kRing5 = 144;  // ring pieces of 1 KiB (gen/fwd_core512.py R)
#ifndef SR_CORE5_A1  // timing experiments compile other generator outputs
#define SR_CORE5_A1 "mlp_fwd512_core_a1.inc"
#define SR_CORE5_A2 "mlp_fwd512_core_a2.inc"
#define SR_CORE5_A1S8 "mlp_fwd512_core_a1s8.inc"
#define SR_CORE5_A2S8 "mlp_fwd512_core_a2s8.inc"
#endif
#define SR_CORE5_A1G "mlp_fwd512_core_a1g.inc"  // the geometry cores (gen/fwd_core512.py heads=False): trunk + sigma
#define SR_CORE5_A2G "mlp_fwd512_core_a2g.inc"
#ifdef SR_F16
#define SR_CORE5_MACROS ".macro MF d, a, b, c\n v_mfma_f32_32x32x16_f16 \\d, \\a, \\b, \\c\n.endm\n.macro PK d, a, b\n v_cvt_pk_f16_f32 \\d, \\a, \\b\n.endm\n"
#else
#define SR_CORE5_MACROS ".macro MF d, a, b, c\n v_mfma_f32_32x32x16_bf16 \\d, \\a, \\b, \\c\n.endm\n.macro PK d, a, b\n v_cvt_pk_bf16_f32 \\d, \\a, \\b\n.endm\n"
#endif

__device__ __forceinline__ u32x32_5 cat8_5(const uint4* f) {
  u32x32_5 v;
#pragma unroll
  for (int i = 0; i < 8; ++i) v[4 * i] = f[i].x, v[4 * i + 1] = f[i].y, v[4 * i + 2] = f[i].z, v[4 * i + 3] = f[i].w;
  return v;
}

// GEOM: the geometry core (as in mlp_fwd2.inc): trunk and sigma tile of the same packed stream, `acc` is then only the register operand
// the stream uses as an accumulator
template <int AUXS, bool REND, int SAVE = 0, bool GEOM = false>
__global__ void __launch_bounds__(256) satnerf_fwd512g_kernel(const FwdParams prm) {
  constexpr int NW = kFwdWaves512;  // (gen/fwd_core512.py feeds the ring in rows of 4)
  constexpr int AK = act8_units(AUXS);  // workspace units per tile (SAVE)
  static_assert(SAVE == 0 || SAVE == SR_FMT8, "the generated core saves in the 8-bit format only");
  static_assert(!GEOM || SAVE == 0, "the geometry core saves nothing");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem;
  float4* l0w = reinterpret_cast<float4*>(smem + kRing5 * 1024);
  float* r_z = reinterpret_cast<float*>(smem + kRing5 * 1024 + kFeat * sizeof(float4));

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

  // aux fragment(s) in the operand format, and their workspace copy (mlp_fwd_io.inc aux_values: the slots)
  u32x8_5 auxv = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  {
    float av[AUXS][8];
    aux_values<AUXS>(prm, in, lane, av);
#pragma unroll
    for (int a = 0; a < AUXS; ++a)
#pragma unroll
      for (int q = 0; q < 4; ++q) auxv[4 * a + q] = pack_op2(av[a][2 * q], av[a][2 * q + 1]);
    if constexpr (SAVE != 0) {
      uint4* save_aux = prm.acts + (tile * AK) * 64 + lane;
#pragma unroll
      for (int a = 0; a < AUXS; ++a) ws_store(save_aux + a * 64, aux_ws_bf16(av[a]));
    }
  }
  uint4* save = SAVE ? prm.acts + (tile * AK) * 64 + lane : nullptr;

  __syncthreads();  // l0w visible; every global load of the prologue has been waited for (the core's LDS-DMA counts start clean)

  // ---- fc_net.0 (K = 3) on VALU, fp32, w0 = 30 folded into l0 ------------------------------------------
  Frags<1, kKS> cur;
#pragma unroll
  for (int s = 0; s < kKS; s += 2) {
    f32x16 pre;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int ss = s + (g >> 3), j = g & 7;
      const float4 w = l0w[(ss * 2 + h) * 8 + j];
      pre[g] = __builtin_fmaf(w.x, x, __builtin_fmaf(w.y, y, __builtin_fmaf(w.z, zc, w.w)));
    }
    uint4 dl0, dl1;
    pack_tile<1, ACT_SIN, SAVE>(pre, cur.hi[s], cur.hi[s + 1], dl0, dl1, save_at<SAVE>(save, AUXS, s));
  }

  // ---- the core: fc_net.2 .. fc_net.14, feats / sigma, the three heads -----------------------------------
  u32x32_5 x0 = cat8_5(cur.hi), x1 = cat8_5(cur.hi + 8), x2 = cat8_5(cur.hi + 16), x3 = cat8_5(cur.hi + 24);
  const uint32_t ring_addr = lds_addr_of(ring);
  const uint32_t vl0 = ring_addr + (uint32_t)lane * 16u, vl1 = vl0 + 65536u, vl2 = vl0 + 131072u;
  uint32_t voff = (uint32_t)wave * 1024u + (uint32_t)lane * 16u;
  const uint32_t wb = __builtin_amdgcn_readfirstlane(ring_addr + (uint32_t)wave * 1024u);
  const uint64_t sb = uniform64(prm.stream_hi);
  f32x16 acc;
  float sig;
  uint32_t m0save;
#ifdef SR_CORE_TIMING
  const uint64_t t_core0 = __builtin_amdgcn_s_memtime();
  const uint64_t r_core0 = __builtin_amdgcn_s_memrealtime();
#endif
  // SAVE: this lane's workspace offset (tile base + lane * 16; the stream advances it unit by unit) and the PHASE8 / MX8 constants
  uint32_t soff = (uint32_t)((unsigned long)tile * AK * 1024ul) + (uint32_t)lane * 16u;
  const float kmagic = 49152.0f, k128 = 128.0f;
  const uint64_t ab = uniform64(prm.acts);
#define SR_CORE5_OUTS                                                                                                                  \
  "+{v[0:31]}"(x0), "+{v[32:63]}"(x1), "+{v[64:95]}"(x2), "+{v[96:127]}"(x3), "+{v[144:151]}"(auxv), "={v[128:143]}"(acc),            \
      "={v168}"(sig), "+{v172}"(voff), [m0save] "=&s"(m0save)
#define SR_CORE5_INS "{v169}"(vl0), "{v170}"(vl1), "{v171}"(vl2), [sb] "s"(sb), [wb] "s"(wb), [wave] "s"(wave)
  if constexpr (GEOM && AUXS == 1) {
    asm volatile(SR_CORE5_MACROS
#include SR_CORE5_A1G
                 ".purgem MF\n.purgem PK\n"
                 : SR_CORE5_OUTS
                 : SR_CORE5_INS
                 :
#include "mlp_fwd512_core_clobbers.inc"
    );
  } else if constexpr (GEOM) {
    asm volatile(SR_CORE5_MACROS
#include SR_CORE5_A2G
                 ".purgem MF\n.purgem PK\n"
                 : SR_CORE5_OUTS
                 : SR_CORE5_INS
                 :
#include "mlp_fwd512_core_clobbers.inc"
    );
  } else if constexpr (AUXS == 1 && SAVE == 0) {
    asm volatile(SR_CORE5_MACROS
#include SR_CORE5_A1
                 ".purgem MF\n.purgem PK\n"
                 : SR_CORE5_OUTS
                 : SR_CORE5_INS
                 :
#include "mlp_fwd512_core_clobbers.inc"
    );
  } else if constexpr (SAVE == 0) {
    asm volatile(SR_CORE5_MACROS
#include SR_CORE5_A2
                 ".purgem MF\n.purgem PK\n"
                 : SR_CORE5_OUTS
                 : SR_CORE5_INS
                 :
#include "mlp_fwd512_core_clobbers.inc"
    );
  } else if constexpr (AUXS == 1) {
    asm volatile(SR_CORE5_MACROS
#include SR_CORE5_A1S8
                 ".purgem MF\n.purgem PK\n"
                 : SR_CORE5_OUTS, "+{v182}"(soff)
                 : SR_CORE5_INS, "{v183}"(kmagic), "{v192}"(k128), [ab] "s"(ab)
                 :
#include "mlp_fwd512_core_clobbers_s8.inc"
    );
  } else {
    asm volatile(SR_CORE5_MACROS
#include SR_CORE5_A2S8
                 ".purgem MF\n.purgem PK\n"
                 : SR_CORE5_OUTS, "+{v182}"(soff)
                 : SR_CORE5_INS, "{v183}"(kmagic), "{v192}"(k128), [ab] "s"(ab)
                 :
#include "mlp_fwd512_core_clobbers_s8.inc"
    );
  }
#undef SR_CORE5_OUTS
#undef SR_CORE5_INS

#ifdef SR_CORE_TIMING
  core_timing_store(prm, tile, lane, t_kernel0, t_core0, r_core0);
  return;
#endif
  write_outputs<REND, NW, GEOM>(prm, in, acc, sig, r_z, wave, lane);
}

template <int AUXS, bool REND, int SAVE = 0, bool GEOM = false>
int launch_fwd512g(const FwdParams& p, hipStream_t st) {
  return launch_fwd_kernel(satnerf_fwd512g_kernel<AUXS, REND, SAVE, GEOM>, GEOM ? "satnerf_fwd512g_kernel (geometry)" : "satnerf_fwd512g_kernel",
                           kFwdWaves512, (size_t)kRing5 * 1024 + kFeat * sizeof(float4), !REND ? 0 : GEOM ? kRendFloatsGeom : kRendFloats, p, st);
}

// entry of the 512-wide translation units: the generated core for inference, the render pass and the 8-bit training forward unless
// SATNERF_FWD_V1=1 selects the hipcc-scheduled kernel (A/B; it also keeps what the stream's 32-bit workspace offsets cannot address:
// mlp_fwd_io.inc fwd_route)
template <int AUXS>
int launch_fwd512_any(const FwdParams& p, int save_fmt, hipStream_t st) {
  const FwdRoute route = fwd_route(p, save_fmt, SR_FMT8, act8_units(AUXS), true);
  if (route != FwdRoute::Core) return route == FwdRoute::Refused ? 1 : launch_fwd<1, AUXS>(p, save_fmt, st);
  if (save_fmt == SR_FMT8) return p.rend.rays != nullptr ? launch_fwd512g<AUXS, true, SR_FMT8>(p, st) : launch_fwd512g<AUXS, false, SR_FMT8>(p, st);
  return p.rend.rays != nullptr ? launch_fwd512g<AUXS, true>(p, st) : launch_fwd512g<AUXS, false>(p, st);
}

// entry of the 512-wide geometry translation units (mlp_fwd512g_g*.hip), as mlp_fwd2.inc launch_fwd_geom
template <int AUXS>
int launch_fwd512_geom(const FwdParams& p, hipStream_t st, int (*full)(const FwdParams&, int, hipStream_t)) {
  if (fwd_route(p, 0, SR_FMT8, act8_units(AUXS), true) != FwdRoute::Core) return full(p, 0, st);
  return p.rend.rays != nullptr ? launch_fwd512g<AUXS, true, 0, true>(p, st) : launch_fwd512g<AUXS, false, 0, true>(p, st);
}

#endif  // SR_FEAT == 512

}  // inline namespace SR_FEAT_NS
}  // namespace sr
