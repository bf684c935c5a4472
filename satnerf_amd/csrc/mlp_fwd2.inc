// Fused Sat-NeRF MLP forward, second generation (width 256, single-pass bf16 / fp16 operands, inference and the one-launch render
// pass): the same decomposition as mlp_fwd.inc -- a wave owns 32 sample points and carries their activations in registers through the
// whole network, weights stream L2 -> LDS by LDS-DMA -- but the 1,406-MFMA core between fc_net.0 and the output activations is ONE
// hand-placed instruction stream (csrc/gen/fwd_core.py -> mlp_fwd_core_a*.inc) instead of hipcc's schedule of C++ templates:
//   * profiles/r03_coissue.txt: on gfx950 v_mfma_f32_32x32x16 and the SIREN epilogue (v_sin + v_cvt_pk) co-issue completely from one
//     wave when placed by hand (32.3-32.8 cycles per MFMA with the A fragment from LDS); hipcc's stream of the same work ran at ~75;
//   * LDS ring = flat ring of 128 pieces fed in rows of 8 (one 1-KiB request per wave), rendezvous per two chunks with exact vmcnt
//     counts; A fragments five MFMAs ahead; the epilogue of tile t-1 sits in the gaps of tile t's MFMAs, also across layers.
//   * fc_net.0 (K = 3, fp32 coordinates) is part of the stream: the prologue splits the coordinates and the fc_net.0 table three ways
//     into bf16 (24 bits) and writes the table's 16 A fragments into ring pieces 0..15 (gen/fwd_core.py l0_terms / l0_pieces); as VALU
//     work it was 128 LDS table reads + 650 instructions per wave with nothing to overlap (14.6 k cycles of the kernel's 112 k).
// Replaces (as mlp_fwd.inc): models/satnerf.py:20-40 + SatNeRF.forward models/satnerf.py:156-208 + Siren models/nerf.py:23-33, and with
// REND rendering.py:62-81 + models/satnerf.py:42-79.  Included after mlp_fwd.inc by the p1 / h1 translation units.
#pragma once
#include "mlp_fwd_io.inc"

namespace sr {
inline namespace SR_FEAT_NS {

#if SR_FEAT == 256

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x16 __attribute__((ext_vector_type(16)));

constexpr int kRing2 = 128;  // ring pieces (gen/fwd_core.py R)
#ifndef SR_CORE_A1  // timing experiments compile other generator outputs (tools/ab_core.sh)
#define SR_CORE_A1 "mlp_fwd_core_a1.inc"
#define SR_CORE_A2 "mlp_fwd_core_a2.inc"
#define SR_CORE_A1S8 "mlp_fwd_core_a1s8.inc"
#define SR_CORE_A2S8 "mlp_fwd_core_a2s8.inc"
#endif
#define SR_CORE_A1G "mlp_fwd_core_a1g.inc"  // the geometry cores (gen/fwd_core.py heads=False): trunk + sigma
#define SR_CORE_A2G "mlp_fwd_core_a2g.inc"
#define SR_CORE_MF0 ".macro MF0 d, a, b, c\n v_mfma_f32_32x32x16_bf16 \\d, \\a, \\b, \\c\n.endm\n"  // fc_net.0's split operands: bf16 in every mode
#ifdef SR_F16
#define SR_CORE_MACROS ".macro MF d, a, b, c\n v_mfma_f32_32x32x16_f16 \\d, \\a, \\b, \\c\n.endm\n.macro PK d, a, b\n v_cvt_pk_f16_f32 \\d, \\a, \\b\n.endm\n" SR_CORE_MF0
#else
#define SR_CORE_MACROS ".macro MF d, a, b, c\n v_mfma_f32_32x32x16_bf16 \\d, \\a, \\b, \\c\n.endm\n.macro PK d, a, b\n v_cvt_pk_bf16_f32 \\d, \\a, \\b\n.endm\n" SR_CORE_MF0
#endif

// v = h + m + l to 24 bits, each term a bf16 value (RNE of the remainder; the remainders are exact in fp32)
__device__ __forceinline__ void split3(float v, float& h, float& m, float& l) {
#pragma clang fp contract(off)
  h = bf16_lo_to_f32(pack_bf16x2(v, 0.f));
  const float r = v - h;
  m = bf16_lo_to_f32(pack_bf16x2(r, 0.f));
  l = bf16_lo_to_f32(pack_bf16x2(r - m, 0.f));
}

// SAVE: 0 = inference, SR_FMT8 = the training forward (activations saved in the 8-bit workspaces of mlp_layout.h: the PHASE8 / MX8
// encoding and the non-temporal stores are part of the generated stream)
// GEOM: the geometry core -- fc_net.0 .. fc_net.14 and the sigma tile of the SAME packed stream (the feats rows are jumped over), no head
// accumulator; with REND the depth-only render pass (models/satnerf.py:183-185 sigma_only + :52-67), mlp_fwd_io.inc write_outputs
template <int AUXS, bool REND, int SAVE = 0, bool GEOM = false>
__global__ void __launch_bounds__(512) satnerf_fwd2_kernel(const FwdParams prm) {
  constexpr int NW = kFwdWaves256;  // (gen/fwd_core.py feeds the ring in rows of 8)
  constexpr int AK = act8_units(AUXS);  // workspace units per tile (SAVE)
  static_assert(SAVE == 0 || SAVE == SR_FMT8, "the generated core saves in the 8-bit format only");
  static_assert(!GEOM || SAVE == 0, "the geometry core saves nothing");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem;
  float* r_z = reinterpret_cast<float*>(smem + kRing2 * 1024);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, pl = lane & 31;
#ifdef SR_CORE_TIMING
  const uint64_t t_kernel0 = __builtin_amdgcn_s_memtime();
#endif

  // fc_net.0's A fragments -> ring pieces 0..15 (gen/fwd_core.py l0_pieces): wave w writes the two k-steps of output tile w; lane =
  // 32 * (k >> 3) + row, row r of the tile is slot 16 (2 w + (g >> 3)) + 8 hh + (g & 7), g = (r & 3) + 4 (r >> 3), hh = (r >> 2) & 1
  {
    const int g = (pl & 3) + 4 * (pl >> 3), hh = (pl >> 2) & 1;
    const float4 w = prm.l0[16 * (2 * wave + (g >> 3)) + 8 * hh + (g & 7)];
    float xh, xm, xl, yh, ym, yl, zh, zm, zl, bh, bm, bl;
    split3(w.x, xh, xm, xl), split3(w.y, yh, ym, yl), split3(w.z, zh, zm, zl), split3(w.w, bh, bm, bl);
    uint4 k0, k1;
    if (h == 0) {
      k0 = make_uint4(pack_bf16x2(xh, xh), pack_bf16x2(xm, xh), pack_bf16x2(yh, yh), pack_bf16x2(ym, yh));
      k1 = make_uint4(pack_bf16x2(xm, xl), pack_bf16x2(ym, yl), pack_bf16x2(zm, zl), 0u);
    } else {
      k0 = make_uint4(pack_bf16x2(zh, zh), pack_bf16x2(zm, zh), pack_bf16x2(bh, bm), pack_bf16x2(bl, 0.f));
      k1 = make_uint4(0u, 0u, 0u, 0u);
    }
    *reinterpret_cast<uint4*>(ring + (2 * wave) * 1024 + lane * 16) = k0;
    *reinterpret_cast<uint4*>(ring + (2 * wave + 1) * 1024 + lane * 16) = k1;
  }

  // this lane's sample point (mlp_fwd_io.inc)
  const PointIn in = point_setup<REND, NW>(prm, r_z, wave, lane);
  const long tile = in.tile;
  const float x = in.x, y = in.y, zc = in.zc;

  // aux fragment(s) in the operand format, and their workspace copy (mlp_fwd_io.inc aux_values: the slots)
  uint4 auxf[AUXS];
  uint4* save = SAVE ? prm.acts + (tile * AK) * 64 + lane : nullptr;
  {
    float av[AUXS][8];
    aux_values<AUXS>(prm, in, lane, av);
#pragma unroll
    for (int a = 0; a < AUXS; ++a) {
      auxf[a] = make_uint4(pack_op2(av[a][0], av[a][1]), pack_op2(av[a][2], av[a][3]), pack_op2(av[a][4], av[a][5]), pack_op2(av[a][6], av[a][7]));
      if constexpr (SAVE != 0) ws_store(save + a * 64, aux_ws_bf16(av[a]));
    }
  }

  __syncthreads();  // fc_net.0's ring pieces visible; every global load of the prologue has been waited for (the core's LDS-DMA counts start clean)

  // ---- fc_net.0's B fragments: the sample position split three ways (gen/fwd_core.py l0_terms), w0 = 30 / 2 pi folded into the table;
  //      the PHASE8 bytes of its pre-activations are saved by the stream like every other layer's ------------------------------------
  u32x4 l0b0, l0b1;
  {
    float xh, xm, xl, yh, ym, yl, zh, zm, zl;
    split3(x, xh, xm, xl), split3(y, yh, ym, yl), split3(zc, zh, zm, zl);
    if (h == 0) {
      l0b0 = u32x4{pack_bf16x2(xh, xm), pack_bf16x2(xh, xl), pack_bf16x2(yh, ym), pack_bf16x2(yh, yl)};
      l0b1 = u32x4{pack_bf16x2(xm, xh), pack_bf16x2(ym, yh), pack_bf16x2(zm, zh), 0u};
    } else {
      l0b0 = u32x4{pack_bf16x2(zh, zm), pack_bf16x2(zh, zl), pack_bf16x2(1.f, 1.f), pack_bf16x2(1.f, 0.f)};
      l0b1 = u32x4{0u, 0u, 0u, 0u};
    }
  }

  // ---- the core: fc_net.2 .. fc_net.14, feats / sigma, the three heads -----------------------------------
  const u32x4 a0 = __builtin_bit_cast(u32x4, auxf[0]);
  const uint32_t ring_addr = lds_addr_of(ring);
  const uint32_t vl0 = ring_addr + (uint32_t)lane * 16u, vl1 = vl0 + 65536u;
  uint32_t voff = (uint32_t)wave * 1024u + (uint32_t)lane * 16u;
  const uint32_t wb = __builtin_amdgcn_readfirstlane(ring_addr + (uint32_t)wave * 1024u);
  const uint64_t sb = uniform64(prm.stream_hi);  // ring piece p is stream piece p - 16: the first requested row is row 2, at source offset 0
  f32x16 acc;
  float sig;
  uint32_t m0save;
#ifdef SR_CORE_TIMING  // experiments: shader cycles of the prologue / core per wave instead of sigma / sun_v (tools/ab_core.sh -DSR_CORE_TIMING)
  const uint64_t t_core0 = __builtin_amdgcn_s_memtime();
  const uint64_t r_core0 = __builtin_amdgcn_s_memrealtime();
#endif
  // SAVE: this lane's workspace offset (tile base + lane * 16; the stream advances it unit by unit) and the PHASE8 constant
  uint32_t soff = (uint32_t)((unsigned long)tile * AK * 1024ul) + (uint32_t)lane * 16u;
  const float kmagic = 49152.0f, k128 = 128.0f;
  const uint64_t ab = uniform64(prm.acts);
#define SR_CORE_OUTS "={v[192:207]}"(acc), "={v208}"(sig), "+{v211}"(voff), [m0save] "=&s"(m0save)
#define SR_CORE_INS "{v[232:235]}"(l0b0), "{v[236:239]}"(l0b1), "{v209}"(vl0), "{v210}"(vl1), [sb] "s"(sb), [wb] "s"(wb), [wave] "s"(wave)
  if constexpr (GEOM && AUXS == 1) {
    asm volatile(SR_CORE_MACROS
#include SR_CORE_A1G
                 ".purgem MF\n.purgem PK\n.purgem MF0\n"
                 : "={v208}"(sig), "+{v211}"(voff), [m0save] "=&s"(m0save)
                 : "{v[184:187]}"(a0), SR_CORE_INS
                 :
#include "mlp_fwd_core_clobbers.inc"
    );
  } else if constexpr (GEOM) {
    const u32x4 a1 = __builtin_bit_cast(u32x4, auxf[AUXS - 1]);
    asm volatile(SR_CORE_MACROS
#include SR_CORE_A2G
                 ".purgem MF\n.purgem PK\n.purgem MF0\n"
                 : "={v208}"(sig), "+{v211}"(voff), [m0save] "=&s"(m0save)
                 : "{v[184:187]}"(a0), "{v[188:191]}"(a1), SR_CORE_INS
                 :
#include "mlp_fwd_core_clobbers.inc"
    );
  } else if constexpr (AUXS == 1 && SAVE == 0) {
    asm volatile(SR_CORE_MACROS
#include SR_CORE_A1
                 ".purgem MF\n.purgem PK\n.purgem MF0\n"
                 : SR_CORE_OUTS
                 : "{v[184:187]}"(a0), SR_CORE_INS
                 :
#include "mlp_fwd_core_clobbers.inc"
    );
  } else if constexpr (AUXS == 2 && SAVE == 0) {
    const u32x4 a1 = __builtin_bit_cast(u32x4, auxf[AUXS - 1]);
    asm volatile(SR_CORE_MACROS
#include SR_CORE_A2
                 ".purgem MF\n.purgem PK\n.purgem MF0\n"
                 : SR_CORE_OUTS
                 : "{v[184:187]}"(a0), "{v[188:191]}"(a1), SR_CORE_INS
                 :
#include "mlp_fwd_core_clobbers.inc"
    );
  } else if constexpr (AUXS == 1) {
    asm volatile(SR_CORE_MACROS
#include SR_CORE_A1S8
                 ".purgem MF\n.purgem PK\n.purgem MF0\n"
                 : SR_CORE_OUTS, "+{v221}"(soff)
                 : "{v[184:187]}"(a0), SR_CORE_INS, "{v220}"(kmagic), "{v228}"(k128), [ab] "s"(ab)
                 :
#include "mlp_fwd_core_clobbers_s8.inc"
    );
  } else {
    const u32x4 a1 = __builtin_bit_cast(u32x4, auxf[AUXS - 1]);
    asm volatile(SR_CORE_MACROS
#include SR_CORE_A2S8
                 ".purgem MF\n.purgem PK\n.purgem MF0\n"
                 : SR_CORE_OUTS, "+{v221}"(soff)
                 : "{v[184:187]}"(a0), "{v[188:191]}"(a1), SR_CORE_INS, "{v220}"(kmagic), "{v228}"(k128), [ab] "s"(ab)
                 :
#include "mlp_fwd_core_clobbers_s8.inc"
    );
  }
#undef SR_CORE_OUTS
#undef SR_CORE_INS

#ifdef SR_CORE_TIMING
  core_timing_store(prm, tile, lane, t_kernel0, t_core0, r_core0);
  return;
#endif
  write_outputs<REND, NW, GEOM>(prm, in, acc, sig, r_z, wave, lane);
}

template <int AUXS, bool REND, int SAVE = 0, bool GEOM = false>
int launch_fwd2(const FwdParams& p, hipStream_t st) {
  return launch_fwd_kernel(satnerf_fwd2_kernel<AUXS, REND, SAVE, GEOM>, GEOM ? "satnerf_fwd2_kernel (geometry)" : "satnerf_fwd2_kernel", kFwdWaves256,
                           (size_t)kRing2 * 1024, !REND ? 0 : GEOM ? kRendFloatsGeom : kRendFloats, p, st);
}

// entry of the (1, AUXS) translation units: the generated core for inference and for the 8-bit training forward, unless
// SATNERF_FWD_V1=1 selects the r02 kernels (A/B); 16-bit workspaces stay on mlp_fwd.inc (mlp_fwd_io.inc fwd_route)
template <int AUXS>
int launch_fwd_any(const FwdParams& p, int save_fmt, hipStream_t st) {
  const FwdRoute route = fwd_route(p, save_fmt, SR_FMT8, act8_units(AUXS), true);
  if (route != FwdRoute::Core) return route == FwdRoute::Refused ? 1 : launch_fwd<1, AUXS>(p, save_fmt, st);
  if (save_fmt == SR_FMT8) return p.rend.rays != nullptr ? launch_fwd2<AUXS, true, SR_FMT8>(p, st) : launch_fwd2<AUXS, false, SR_FMT8>(p, st);
  return p.rend.rays != nullptr ? launch_fwd2<AUXS, true>(p, st) : launch_fwd2<AUXS, false>(p, st);
}

// entry of the geometry translation units (mlp_fwdg_*.hip): a launch that wants sigma alone (p.albedo / sun_v / beta and rend.rgb / sky
// null).  fwd_route decides as for every inference launch; off the Core route `full` -- the (1, AUXS) unit's entry -- runs the request
// with the unused outputs null: correct, and no faster.
template <int AUXS>
int launch_fwd_geom(const FwdParams& p, hipStream_t st, int (*full)(const FwdParams&, int, hipStream_t)) {
  if (fwd_route(p, 0, SR_FMT8, act8_units(AUXS), true) != FwdRoute::Core) return full(p, 0, st);
  return p.rend.rays != nullptr ? launch_fwd2<AUXS, true, 0, true>(p, st) : launch_fwd2<AUXS, false, 0, true>(p, st);
}

#endif  // SR_FEAT == 256

}  // inline namespace SR_FEAT_NS
}  // namespace sr
