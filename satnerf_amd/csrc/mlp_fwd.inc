// Fused Sat-NeRF MLP forward for gfx950: one launch evaluates fc_net (8 SIREN layers), the sigma,
// albedo, sun-visibility and uncertainty heads for every sample point of a ray batch.
//
// Replaces: models/satnerf.py:20-40 (repeat_interleave + point-chunk loop) and SatNeRF.forward
// models/satnerf.py:156-208 with Siren models/nerf.py:23-33 -- about 80 ATen kernels per 5120 points
// in the reference.  See mlp_layout.h for the orientation / slot permutation / stream format.
//
// Workgroup = NW waves; each wave owns 32 consecutive sample points and carries their activations in
// registers through the whole network (B fragments).  The weight stream is pulled L2 -> LDS with
// global_load_lds (1 KiB per wave-instruction) into a 4-slot ring, 3 chunks ahead of the consumer,
// with counted vmcnt waits and one raw s_barrier per chunk (a chunk = one 32-row output tile).
//   SR_MODE_BF16   : 8 waves (2 per SIMD, <=256 VGPR), one MFMA per k-step.
//   SR_MODE_BF16X3 : 4 waves (1 per SIMD, <=512 VGPR), hi*hi + lo*hi + hi*lo per k-step.
#pragma once
#include <type_traits>
#include <utility>

#include "common.h"
#include "mlp_layout.h"
#include "ray_device.h"
#include "mlp_params.h"
#define SR_DMA_BRANCH 1  // ragged last DMA round: branched here, predicated in the dX kernel (A/B: profiles/r02_ab_variants.txt)
#include "mlp_device.h"
#include "codec8.h"

namespace sr {
inline namespace SR_FEAT_NS {

// acc += A(chunk pieces [0,NP)) x B(fragments P0 .. P0+NP-1), where fragment index >= KS means aux[index-KS].
// A fragments are fetched from LDS in batches of BATCH ds_read_b128 issued back to back, one batch ahead of the MFMAs
// that consume them; sched_barrier(0) pins that order (left alone, hipcc sinks each read next to its MFMA and the
// chain becomes one LDS round trip per MFMA pair).
template <int NPASS, int NP, int P0, int KS, int AUXS, int BATCH>
__device__ __forceinline__ void mma_chunk(f32x16& acc, const char* slot, const Frags<NPASS, KS>& in,
                                          const Frags<NPASS, AUXS>& aux, int lane) {
  constexpr int PB = Mode<NPASS>::PIECE_BYTES;
  constexpr int NB = (NP + BATCH - 1) / BATCH;
  uint4 ah[NP], al[NPASS == 3 ? NP : 1];
  auto load_batch = [&](int b) {
#pragma unroll
    for (int i = b * BATCH; i < (b + 1) * BATCH && i < NP; ++i) {
      ah[i] = *reinterpret_cast<const uint4*>(slot + i * PB + lane * 16);
      if constexpr (NPASS == 3) al[i] = *reinterpret_cast<const uint4*>(slot + i * PB + 1024 + lane * 16);
    }
  };
  load_batch(0);
  SR_SCHED_BARRIER();
#ifdef SR_ACC2
  f32x16 acc2 = {0};  // second, independent accumulation chain (odd pieces): halves the MFMA->MFMA dependency depth
#endif
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (b + 1 < NB) load_batch(b + 1);
    SR_SCHED_BARRIER();
#pragma unroll
    for (int i = b * BATCH; i < (b + 1) * BATCH && i < NP; ++i) {
      const int f = P0 + i;
      const uint4 bh = f < KS ? in.hi[f < KS ? f : 0] : aux.hi[f < KS ? 0 : f - KS];
#ifdef SR_ACC2
      if (i & 1) {  // constant after unrolling: no lvalue select (that would put both accumulators on the stack)
        if constexpr (NPASS == 3) {
          const uint4 bl = f < KS ? in.lo[f < KS ? f : 0] : aux.lo[f < KS ? 0 : f - KS];
          acc2 = mfma(al[i], bh, acc2);
          acc2 = mfma(ah[i], bl, acc2);
        }
        acc2 = mfma(ah[i], bh, acc2);
        continue;
      }
#endif
      if constexpr (NPASS == 3) {
        const uint4 bl = f < KS ? in.lo[f < KS ? f : 0] : aux.lo[f < KS ? 0 : f - KS];
        acc = mfma(al[i], bh, acc);  // small terms first
        acc = mfma(ah[i], bl, acc);
      }
      acc = mfma(ah[i], bh, acc);
    }
    SR_SCHED_BARRIER();
  }
#ifdef SR_ACC2
  acc += acc2;
#endif
}

// ---- epilogues: 16 accumulator values of one tile -> two B fragments of the next stage ---------------
enum { ACT_SIN = 0, ACT_ID = 1 };

// SAVE: 0 = inference, SR_FMT16 / SR_FMT8 = training workspace format (mlp_layout.h).  Returns the MX8 scale byte of the
// tile (SR_FMT8 identity stages), 0 otherwise.
template <int NPASS, int ACT, int SAVE>
__device__ __forceinline__ uint32_t pack_tile(const f32x16& acc, uint4& h0, uint4& h1, uint4& l0, uint4& l1, uint4* save0) {
  float v[16];
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    // parity mode: the hardware sine of the EXACT fraction (v_fract is exact in fp32).  Measured against the degree-11 polynomial
    // (sin_rev_precise) it replaced: the same 1.6e-6 / 1.2e-6 / 1.5e-6 of the reference on rgb / depth / weights, kernel 346 -> 298 us
    // (profiles/r03_ab_variants.txt)
    if (ACT == ACT_SIN) v[g] = NPASS == 3 ? sin_rev_fast(__builtin_amdgcn_fractf(acc[g])) : sin_rev_fast(acc[g]);
    else v[g] = acc[g];
  }
  uint32_t hw[8], lw[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    if constexpr (NPASS == 3) split_bf16x2(v[2 * q], v[2 * q + 1], hw[q], lw[q]);
    else hw[q] = pack_op2(v[2 * q], v[2 * q + 1]);
  }
  h0 = make_uint4(hw[0], hw[1], hw[2], hw[3]);
  h1 = make_uint4(hw[4], hw[5], hw[6], hw[7]);
  if constexpr (NPASS == 3) {
    l0 = make_uint4(lw[0], lw[1], lw[2], lw[3]);
    l1 = make_uint4(lw[4], lw[5], lw[6], lw[7]);
  }
  if constexpr (SAVE == SR_FMT8) {
    // one byte per value: the phase of a sin stage's pre-activation, micro-scaled int8 for an identity stage (codec8.h)
    if constexpr (ACT == ACT_SIN) {
      ws_store(save0, phase8_encode(acc));
    } else {
      const uint32_t e = mx8_exponent(acc, hw[0]);  // `after` = hw[0], packed from acc[0], acc[1] by ordinary instructions: the MFMA -> VALU wait states are in place for all 16 registers (codec8.h contract)
      ws_store(save0, mx8_encode(acc, e));
      return e;
    }
  } else if constexpr (SAVE == SR_FMT16) {
    // training: sin stages save the PHASE of the pre-activation as unorm16 (sin and cos are both
    // recovered to ~5e-5 in the backward pass); identity stages save the bf16 value.
    if (ACT == ACT_SIN) {
      uint32_t pw[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        auto pk = __builtin_amdgcn_cvt_pknorm_u16(__builtin_amdgcn_fractf(acc[2 * q]), __builtin_amdgcn_fractf(acc[2 * q + 1]));
        pw[q] = __builtin_bit_cast(uint32_t, pk);
      }
      ws_store(save0, make_uint4(pw[0], pw[1], pw[2], pw[3]));
      ws_store(save0 + 64, make_uint4(pw[4], pw[5], pw[6], pw[7]));
    } else {
#ifdef SR_F16  // the 16-bit workspaces are operands of the bf16 backward kernels: identity stages are saved as bf16, not as the fp16 MFMA operand
      ws_store(save0, make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])));
      ws_store(save0 + 64, make_uint4(pack_bf16x2(v[8], v[9]), pack_bf16x2(v[10], v[11]), pack_bf16x2(v[12], v[13]), pack_bf16x2(v[14], v[15])));
#else
      ws_store(save0, h0);
      ws_store(save0 + 64, h1);
#endif
    }
  }
  return 0u;
}

// workspace address of the fragment pair starting at logical fragment `frag` (aux excluded) of this lane's tile
template <int SAVE>
__device__ __forceinline__ uint4* save_at(uint4* tile_base, int auxs, int frag) {
  if constexpr (SAVE == SR_FMT8) return tile_base + (auxs + (frag >> 1)) * 64;
  else if constexpr (SAVE == SR_FMT16) return tile_base + (auxs + frag) * 64;
  else return nullptr;
}

// Entry protocol of chunk G (compile-time global chunk index).
//   KG == 1: rendezvous per chunk -- wait for chunk G's DMA, barrier, refill the slot consumed one chunk ago with chunk G + kD
//            (4-slot ring).  Used when the kernel also streams activations to HBM (counted vmcnt must skip those stores) and in
//            BF16X3 mode (34-KiB slots).
//   KG  > 1: rendezvous per GROUP of KG chunks with a 2*KG-slot ring: at a group start every wave waits for ALL its DMA
//            (nothing else is in flight in inference mode), barrier, then the whole next group is requested; chunks inside a
//            group run with no synchronisation, so the two waves of a SIMD keep the matrix pipe fed while the other one is in
//            its epilogue.  PMC before: 46 % of wave time parked at waitcnt/barrier with 88 rendezvous per launch.
template <int KG>
constexpr int ring_slots() { return KG == 1 ? kNSLOT : 2 * KG; }

template <int NPASS, int AUXS, int KG, int G>
__device__ __forceinline__ void chunk_enter(char* ring, const char* shi, const char* slo, int wave, int lane) {
  using FS = FwdStream<AUXS>;
  constexpr int SLOT_BYTES = FS::SLOTP * Mode<NPASS>::PIECE_BYTES;
  if constexpr (KG == 1) {
    constexpr int later = [] {  // loads certainly issued after chunk G's: chunks G+1 .. G+kD-1
      int n = 0;
      for (int c = 1; c < kD; ++c) n += min_loads<NPASS>(FS::np(G + c));
      return n;
    }();
    wait_then_barrier<later>();
    if constexpr (G + kD < FS::NCH) {
      constexpr long off = FS::offset_pieces(G + kD) * 1024L;  // must be a constant expression: evaluated at run time otherwise
      constexpr int slot = (G + kD) % kNSLOT;
      issue_chunk<NPASS, FS::np(G + kD)>(shi, slo, off, ring + slot * SLOT_BYTES, wave, lane);
    }
  } else if constexpr (G % KG == 0) {
    wait_then_barrier<0>();
    static_for<KG>([&](auto ic) {
      constexpr int c = G + KG + decltype(ic)::value;
      if constexpr (c < FS::NCH) {
        constexpr long off = FS::offset_pieces(c) * 1024L;
        issue_chunk<NPASS, FS::np(c)>(shi, slo, off, ring + (c % (2 * KG)) * SLOT_BYTES, wave, lane);
      }
    });
  }
}

// A generic dense stage: MT output tiles, each one chunk of KS+AUXS pieces; tile results packed into `out`
// (fragments O0 + 2t, O0 + 2t + 1).  G0 = global chunk index of the stage's first chunk.
// `save_tile` = this lane's workspace tile, SF0 = logical fragment of the stage's first output; returns the MX8 scale bytes
// of the stage's tiles (SR_FMT8 identity stage: byte t = tile t, MT <= 8).
template <int NPASS, int AUXS, int KG, int KS, int MT, int ACT, int SAVE, int G0, int NOUT, int SF0, int O0 = 0>
__device__ __forceinline__ uint4 dense_stage(const Frags<NPASS, KS>& in, const Frags<NPASS, AUXS>& aux,
                                             Frags<NPASS, NOUT>& out, char* ring, const char* shi, const char* slo,
                                             int wave, int lane, uint4* save_tile) {
  using FS = FwdStream<AUXS>;
  constexpr int SLOT_BYTES = FS::SLOTP * Mode<NPASS>::PIECE_BYTES;
  static_assert(KS + AUXS <= FS::SLOTP, "tile must fit one ring slot");
  // software pipeline: tile t's MFMAs are issued first, THEN tile t-1's epilogue (sin / pack, VALU) in the same scheduling
  // region, so the epilogue runs under the matrix pipe instead of in front of the next barrier (SR_NO_EPI_PIPE: A/B switch)
  f32x16 acc[2];
  uint32_t eb[4] = {0u, 0u, 0u, 0u};
  auto epilogue = [&](auto tc) {
    constexpr int t = decltype(tc)::value, o = O0 + 2 * t;
    uint4 dl0, dl1;
    uint4* sp = save_at<SAVE>(save_tile, AUXS, SF0 + 2 * t);
    uint32_t e;
    if constexpr (NPASS == 3) e = pack_tile<NPASS, ACT, SAVE>(acc[t & 1], out.hi[o], out.hi[o + 1], out.lo[o], out.lo[o + 1], sp);
    else e = pack_tile<NPASS, ACT, SAVE>(acc[t & 1], out.hi[o], out.hi[o + 1], dl0, dl1, sp);
    if constexpr (SAVE == SR_FMT8 && ACT == ACT_ID) eb[t >> 2] |= e << (8 * (t & 3));
  };
  static_for<MT>([&](auto tc) {
    constexpr int t = decltype(tc)::value, g = G0 + t;
    static_assert(FS::np(g) == KS + AUXS, "stream geometry mismatch");
    chunk_enter<NPASS, AUXS, KG, g>(ring, shi, slo, wave, lane);
    acc[t & 1] = f32x16{0};
    mma_chunk<NPASS, KS + AUXS, 0, KS, AUXS, kBatchHead>(acc[t & 1], ring + (g % ring_slots<KG>()) * SLOT_BYTES, in, aux, lane);
#ifdef SR_NO_EPI_PIPE
    epilogue(tc);
#else
    if constexpr (t > 0) epilogue(std::integral_constant<int, t - 1>{});
#endif
  });
#ifndef SR_NO_EPI_PIPE
  epilogue(std::integral_constant<int, MT - 1>{});
#endif
  return make_uint4(eb[0], eb[1], eb[2], eb[3]);
}

// ---- a lane's sample point: shared by every forward kernel (this file's and the generated-core ones) --------------------------------
struct PointIn {
  long tile, pt, r, rg;  // 32-point tile of the wave, global point index, ray of the point, row of the per-ray input arrays
  bool valid;            // pt < n_points (tail lanes compute the last point again and store nothing)
  float x, y, zc;        // sample position
  const float* sn;       // sun direction of the ray
  const float* te;       // embedding vector of the ray
  long first = 0;        // (in-launch sampler) position of the batch's first row index in gather_idx
  uint32_t step_read = 0u, cursor_read = 0u;  // what the launch found in its counters (training launches advance them at their end)
};

// REND: r_z = the workgroup's per-point depths in LDS (NW * 32 floats), written here for the compositing epilogue
template <bool REND, int NW>
__device__ __forceinline__ PointIn point_setup(const FwdParams& prm, float* r_z, int wave, int lane) {
  const int h = lane >> 5, pl = lane & 31;
  PointIn p;
  p.tile = (long)blockIdx.x * NW + wave;
  p.pt = p.tile * 32 + pl;
  p.valid = p.pt < prm.in.n_points;
  const long pt = p.pt, ptc = p.valid ? p.pt : prm.in.n_points - 1;
  const bool valid = p.valid;
  const long r = ptc / prm.in.n_samples;
  long rg = r;
  uint32_t rng_step = 0u;
  if constexpr (REND) {
    const bool draw = prm.rend.z_in == nullptr && prm.rend.u == nullptr;
    // (a launch that ticks reads the counter whatever the source of its depths: a training launch with `u` / `z_in` supplied would otherwise
    //  write next_step(0) back at its exit and reset Adam's step count, ADVICE r05)
    if ((draw || prm.rend.bank_chunks > 0 || prm.rend.tick != 0) && prm.rend.step_counter) rng_step = (uint32_t)prm.rend.step_counter[0];
    // training launches advance their counters when they END (write_outputs: tick_at_exit), the others here
    const bool train = prm.train.target != nullptr;
    p.step_read = rng_step;
    if (prm.rend.tick && !train) tick_when_all_read(prm.rend.step_counter, rng_step, 0u, prm.rend.bank_chunks > 0 ? (uint32_t)prm.rend.bank_chunks : 1u);
    if (prm.rend.tick == 2) rng_step = next_step(rng_step);  // "tick first": this launch opens the step, its jitter is the advanced step's
    if (prm.rend.bank_chunks > 0) rg += (long)(rng_step % (uint32_t)prm.rend.bank_chunks) * prm.rend.n_rays;
    if (prm.train.gather_idx != nullptr) {  // the batch sampler: batch cursor[0] of the epoch's shuffled rows (the cursor moves on at the exit)
      p.cursor_read = (uint32_t)prm.train.cursor[0];
      p.first = (long)p.cursor_read * prm.rend.n_rays;
      rg = prm.train.gather_idx[p.first + r];
    }
  }
  float x, y, zc;
  {
#pragma clang fp contract(off)  // rendering.py:81 is an unfused mul then add
    const float* o = prm.in.org + rg * prm.in.org_stride;
    x = o[0], y = o[1], zc = o[2];
    if constexpr (REND) {
      const int S = prm.in.n_samples;
      const int j = (int)(ptc - r * S);
      float zz;
      if (prm.rend.z_in) {
        zz = prm.rend.z_in[ptc];
      } else {
        const float* ray = prm.rend.rays + rg * prm.rend.ray_stride;
        // (the jitter is keyed by the ray's place in the launch's batch: a sampled batch draws what the gathered batch would)
        zz = stratified_z(ray[6], ray[7], j, S, prm.rend.u ? prm.rend.u[ptc] : philox_uniform(prm.rend.seed, prm.train.gather_idx ? r : rg, j, rng_step));
      }
      if (h == 0) {
        r_z[wave * 32 + pl] = zz;
        if (valid && prm.rend.z_out) prm.rend.z_out[pt] = zz;
      }
      const float* d = prm.in.dir + rg * prm.in.dir_stride;
      const float mx = d[0] * zz, my = d[1] * zz, mz = d[2] * zz;
      x = x + mx, y = y + my, zc = zc + mz;
    } else if (prm.in.dir != nullptr && prm.in.z != nullptr) {
      const float* d = prm.in.dir + r * prm.in.dir_stride;
      const float zz = prm.in.z[ptc];
      const float mx = d[0] * zz, my = d[1] * zz, mz = d[2] * zz;
      x = x + mx, y = y + my, zc = zc + mz;
    }
  }
  p.x = x, p.y = y, p.zc = zc, p.r = r, p.rg = rg;
  p.sn = prm.in.sun + rg * prm.in.sun_stride;
  p.te = prm.in.temb + (prm.in.ts ? prm.in.ts[rg] : rg) * prm.tau;
  return p;

}

// the workspace copy of one aux fragment: bf16 whatever the forward's single-pass operand format, it is an operand of the (bf16) backward kernels
__device__ __forceinline__ uint4 aux_ws_bf16(const float (&v)[8]) {
  return make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
}

template <int NPASS, int AUXS, int SAVE, int KG, bool REND = false>
__global__ void __launch_bounds__(Mode<NPASS>::NW * 64) satnerf_fwd_kernel(const FwdParams prm) {
  using FS = FwdStream<AUXS>;
  constexpr int NW = Mode<NPASS>::NW;
  static_assert(NW == (kFeat != 256 ? kFwdWaves512 : NPASS == 1 ? kFwdWaves256 : kFwdWavesParity), "sr_render_points_per_block (mlp_params.h)");
  constexpr int SLOT_BYTES = FS::SLOTP * Mode<NPASS>::PIECE_BYTES;
  constexpr int AK = SAVE == SR_FMT8 ? act8_units(AUXS) : act_ksteps(AUXS);  // workspace units per tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem;
  constexpr int NS = ring_slots<KG>();
  float4* l0w = reinterpret_cast<float4*>(smem + NS * SLOT_BYTES);
  // REND: per-point values of the workgroup's NW * 32 consecutive points = whole rays, handed to the compositing epilogue
  constexpr int P = NW * 32;
  float* r_z = reinterpret_cast<float*>(smem + NS * SLOT_BYTES + kFeat * sizeof(float4));
  float *r_sigma = r_z + P, *r_sun = r_z + 2 * P, *r_albedo = r_z + 3 * P;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, pl = lane & 31;
  const char* shi = prm.stream_hi;
  const char* slo = prm.stream_lo;

  // prologue: start the weight stream, stage fc_net.0 into LDS
#pragma unroll
  for (int g = 0; g < (KG == 1 ? kD : KG); ++g) issue_chunk<NPASS, FS::SLOTP>(shi, slo, (long)g * FS::SLOTP * 1024, ring + g * SLOT_BYTES, wave, lane);
  for (int i = tid; i < kFeat; i += NW * 64) l0w[i] = prm.l0[i];

  // this lane's sample point
  const PointIn in = point_setup<REND, NW>(prm, r_z, wave, lane);
  const long tile = in.tile, pt = in.pt, r = in.r, rg = in.rg;
  const bool valid = in.valid;
  const float x = in.x, y = in.y, zc = in.zc;
  const float *sn = in.sn, *te = in.te;

  // aux fragment(s): slots [sun(3), 1, xyz(3), 0 | t(0..7) | t(8..15) | t(16..23)]
  Frags<NPASS, AUXS> aux;
#ifdef SR_F16
  uint4 aux_ws[AUXS];
#endif
  {
    float av[AUXS][8];  // mlp_fwd_io.inc aux_values' fill, spelled out: hipcc schedules this kernel end to end, and calling the helper moved its instruction count (-11 .. +13)
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
#pragma unroll
    for (int a = 0; a < AUXS; ++a) {
      uint32_t hw[4], lw[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if constexpr (NPASS == 3) split_bf16x2(av[a][2 * q], av[a][2 * q + 1], hw[q], lw[q]);
        else hw[q] = pack_op2(av[a][2 * q], av[a][2 * q + 1]);
      }
      aux.hi[a] = make_uint4(hw[0], hw[1], hw[2], hw[3]);
      if constexpr (NPASS == 3) aux.lo[a] = make_uint4(lw[0], lw[1], lw[2], lw[3]);
#ifdef SR_F16  // the workspace copy of the aux fragment is an operand of the (bf16) backward kernels
      aux_ws[a] = aux_ws_bf16(av[a]);
#endif
    }
  }
  uint4* save = SAVE ? prm.acts + (tile * AK) * 64 + lane : nullptr;
  if constexpr (SAVE != 0) {
#pragma unroll
#ifdef SR_F16
    for (int a = 0; a < AUXS; ++a) ws_store(save + a * 64, aux_ws[a]);
#else
    for (int a = 0; a < AUXS; ++a) ws_store(save + a * 64, aux.hi[a]);
#endif
  }

  __syncthreads();  // l0w visible (drains the prologue DMA too; only here)

  // ---- fc_net.0 (K = 3) on VALU, fp32, w0 = 30 folded into l0 ------------------------------------------
  Frags<NPASS, kKS> cur, nxt;
#pragma unroll
  for (int s = 0; s < kKS; ++s) {
    f32x16 pre;  // reuse pack_tile on pairs of k-steps: build 16 pre-activations = fragments (s even, s odd)
    if ((s & 1) == 0) {
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int ss = s + (g >> 3), j = g & 7;
        const float4 w = l0w[(ss * 2 + h) * 8 + j];
        pre[g] = __builtin_fmaf(w.x, x, __builtin_fmaf(w.y, y, __builtin_fmaf(w.z, zc, w.w)));
      }
      uint4 dl0, dl1;
      uint4* sp = save_at<SAVE>(save, AUXS, s);
      if constexpr (NPASS == 3) pack_tile<NPASS, ACT_SIN, SAVE>(pre, cur.hi[s], cur.hi[s + 1], cur.lo[s], cur.lo[s + 1], sp);
      else pack_tile<NPASS, ACT_SIN, SAVE>(pre, cur.hi[s], cur.hi[s + 1], dl0, dl1, sp);
    }
  }

  // ---- fc_net.2 .. fc_net.14: 7 x (256 -> 256, sin) ------------------------------------------------------
#pragma unroll 1
  for (int l = 0; l < kTrunkLayers; ++l) {
    const long lbase = (long)l * kMT;
    f32x16 tacc[2];
    auto tepi = [&](auto tc) {
      constexpr int t = decltype(tc)::value;
      uint4 dl0, dl1;
      uint4* sp = save_at<SAVE>(save, AUXS, (l + 1) * kKS + 2 * t);
      if constexpr (NPASS == 3) pack_tile<NPASS, ACT_SIN, SAVE>(tacc[t & 1], nxt.hi[2 * t], nxt.hi[2 * t + 1], nxt.lo[2 * t], nxt.lo[2 * t + 1], sp);
      else pack_tile<NPASS, ACT_SIN, SAVE>(tacc[t & 1], nxt.hi[2 * t], nxt.hi[2 * t + 1], dl0, dl1, sp);
    };
    static_for<kMT>([&](auto tc) {
      constexpr int t = decltype(tc)::value;
      if constexpr (KG == 1) {
        wait_then_barrier<(kD - 1) * min_loads<NPASS>(FS::SLOTP)>();
        issue_chunk<NPASS, FS::SLOTP>(shi, slo, (lbase + t + kD) * FS::SLOTP * 1024, ring + ((t + kD) % kNSLOT) * SLOT_BYTES, wave, lane);
      } else if constexpr (t % KG == 0) {
        // vmcnt(0): the group's chunks were requested one group ago, but the workspace stores of the epilogues in between sit in
        // the same counter and complete OUT OF ORDER with respect to the (in-order) loads -- a count that skipped them let the
        // MFMAs read a chunk that had not landed (tried in r02: NaNs)
        wait_then_barrier<0>();
        static_for<KG>([&](auto ic) {
          constexpr int c = t + KG + decltype(ic)::value;  // chunk index within (this layer | next stage): all SLOTP pieces
          issue_chunk<NPASS, FS::SLOTP>(shi, slo, (lbase + c) * FS::SLOTP * 1024, ring + (c % NS) * SLOT_BYTES, wave, lane);
        });
      }
      tacc[t & 1] = f32x16{0};
      mma_chunk<NPASS, kKS + AUXS, 0, kKS, AUXS, kBatchTrunk>(tacc[t & 1], ring + (t % NS) * SLOT_BYTES, cur, aux, lane);
#ifdef SR_NO_EPI_PIPE
      tepi(tc);
#else
      if constexpr (t > 0) tepi(std::integral_constant<int, t - 1>{});
#endif
    });
#ifndef SR_NO_EPI_PIPE
    tepi(std::integral_constant<int, kMT - 1>{});
#endif
    cur = nxt;
  }

  // ---- G1: feats = feats_from_xyz(a7) (identity), sigma = softplus(sigma_from_xyz(a7)) ------------------
  Frags<NPASS, kKS> feats;
  {
    const uint4 fe = dense_stage<NPASS, AUXS, KG, kKS, kMT, ACT_ID, SAVE, FS::G_G1, kKS, kActFeats>(cur, aux, feats, ring, shi, slo, wave, lane, save);
    if constexpr (SAVE == SR_FMT8) {  // kMT scale bytes of the feats tiles
      if constexpr (kMT > 8) *(save + (AUXS + kA8Scale) * 64) = fe;
      else *reinterpret_cast<uint2*>(save + (AUXS + kA8Scale) * 64) = make_uint2(fe.x, fe.y);
    }
  }
  {
    constexpr int g = FS::G_G1 + kMT;
    chunk_enter<NPASS, AUXS, KG, g>(ring, shi, slo, wave, lane);
    f32x16 acc = {0};
    mma_chunk<NPASS, kKS + AUXS, 0, kKS, AUXS, kBatchHead>(acc, ring + (g % NS) * SLOT_BYTES, cur, aux, lane);
    if constexpr (REND) {
      const float sg = softplus_f(acc[0]);
      if (h == 0) r_sigma[wave * 32 + pl] = sg;
      if (h == 0 && valid && prm.sigma) prm.sigma[pt] = sg;
    } else {
      if (h == 0 && valid && prm.sigma) prm.sigma[pt] = softplus_f(acc[0]);
    }
  }

  // ---- head: each hidden vector = sin(W [feats; aux]) is folded into the 5-row output tile as soon as it exists ---
  f32x16 acc = {0};  // rows 0..2 albedo logits, 3 sun-visibility logit, 4 beta pre-softplus
  auto head_part = [&](auto gc, const Frags<NPASS, kHS>& hid, auto npc) {
    constexpr int g = decltype(gc)::value, n = decltype(npc)::value;
    static_assert(FS::np(g) == n, "stream geometry mismatch");
    chunk_enter<NPASS, AUXS, KG, g>(ring, shi, slo, wave, lane);
    mma_chunk<NPASS, n, 0, kHS, AUXS, kBatchHead>(acc, ring + (g % NS) * SLOT_BYTES, hid, aux, lane);
  };
  {
    Frags<NPASS, kHS> rgbh;  // rgb_from_xyzdir.0
    dense_stage<NPASS, AUXS, KG, kKS, kMTH, ACT_SIN, SAVE, FS::G_G2R, kHS, kActRgbh>(feats, aux, rgbh, ring, shi, slo, wave, lane, save);
    head_part(std::integral_constant<int, FS::G_HR>{}, rgbh, std::integral_constant<int, kHS>{});
  }
  {
    Frags<NPASS, kHS> s1, s2, s3;  // sun_v_net.0, .2, .4
    dense_stage<NPASS, AUXS, KG, kKS, kMTH, ACT_SIN, SAVE, FS::G_G2S, kHS, kActS1>(feats, aux, s1, ring, shi, slo, wave, lane, save);
    dense_stage<NPASS, AUXS, KG, kHS, kMTH, ACT_SIN, SAVE, FS::G_S2, kHS, kActS2>(s1, aux, s2, ring, shi, slo, wave, lane, save);
    dense_stage<NPASS, AUXS, KG, kHS, kMTH, ACT_SIN, SAVE, FS::G_S3, kHS, kActS3>(s2, aux, s3, ring, shi, slo, wave, lane, save);
    head_part(std::integral_constant<int, FS::G_HS>{}, s3, std::integral_constant<int, kHS>{});
  }
  {
    Frags<NPASS, kHS> e1;  // beta_from_xyz.0
    dense_stage<NPASS, AUXS, KG, kKS, kMTH, ACT_SIN, SAVE, FS::G_G2B, kHS, kActE1>(feats, aux, e1, ring, shi, slo, wave, lane, save);
    head_part(std::integral_constant<int, FS::G_HB>{}, e1, std::integral_constant<int, kHS + AUXS>{});  // + aux: the five biases
  }
  if constexpr (REND) {
    // per-point outputs -> HBM as before, and -> LDS for the compositing of this workgroup's rays (models/satnerf.py:52-70):
    // wave w composites ray w of the workgroup, lane = sample, with the very functions of the stand-alone kernels
    if (h == 0) {
      const float a0 = sigmoid_f(acc[0]) * 1.002f - 0.001f, a1 = sigmoid_f(acc[1]) * 1.002f - 0.001f, a2 = sigmoid_f(acc[2]) * 1.002f - 0.001f;
      const float sv = sigmoid_f(acc[3]);
      float* la = r_albedo + (wave * 32 + pl) * 3;
      la[0] = a0, la[1] = a1, la[2] = a2;
      r_sun[wave * 32 + pl] = sv;
      if (valid) {
        if (prm.albedo) {
          float* a = prm.albedo + pt * 3;
          a[0] = a0, a[1] = a1, a[2] = a2;
        }
        if (prm.sun_v) prm.sun_v[pt] = sv;
      }
    } else if (valid && prm.beta) {
      prm.beta[pt] = softplus_f(acc[0]);
    }
    __syncthreads();
    const int S = prm.in.n_samples;
    const int rays_here = P / S;  // host contract: S divides P
    for (int lr = wave; lr < rays_here; lr += NW) {
      const long ray = (long)blockIdx.x * rays_here + lr;
      if (ray >= prm.rend.n_rays) break;
      const float* rr = prm.rend.rays + (ray + (rg - r)) * prm.rend.ray_stride;
      float k0, k1, k2;
      sky_ray(rr[8], rr[9], rr[10], prm.rend.sky_hidden, prm.rend.w1, prm.rend.b1, prm.rend.w2, prm.rend.b2, lane, k0, k1, k2);
      if (lane == 0 && prm.rend.sky) prm.rend.sky[ray * 3] = k0, prm.rend.sky[ray * 3 + 1] = k1, prm.rend.sky[ray * 3 + 2] = k2;
      composite_ray(r_z + lr * S, r_sigma + lr * S, prm.rend.noise ? prm.rend.noise + ray * S : nullptr, prm.rend.noise_std,
                    r_albedo + lr * S * 3, r_sun + lr * S, k0, k1, k2, S, lane, 1, prm.rend.weights + ray * S, prm.rend.transp + ray * S,
                    prm.rend.depth ? prm.rend.depth + ray : nullptr, prm.rend.rgb ? prm.rend.rgb + ray * 3 : nullptr);
    }
  } else if (valid) {
    if (h == 0) {
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


namespace sr {
inline namespace SR_FEAT_NS {
// The launch of every forward kernel of this family (this file's and the generated-core ones): workgroups of `nw` waves, one 32-point
// tile per wave; dynamic LDS = the kernel's own `lds_bytes` (ring, fc_net.0 table) + `rend_floats` floats per point of the workgroup
// for the render epilogue (0 = a plain MLP launch; a render launch composites whole rays, so n_samples must divide the workgroup).
using FwdKernel = void (*)(const FwdParams);
inline int launch_fwd_kernel(FwdKernel kern, const char* name, int nw, size_t lds_bytes, int rend_floats, const FwdParams& p, hipStream_t st) {
  const size_t lds = lds_bytes + (size_t)nw * 32 * rend_floats * sizeof(float);
  if (rend_floats != 0 && (nw * 32) % p.in.n_samples != 0) {
    set_error("sr_satnerf_render_fwd: n_samples=%d must divide the %d points of a workgroup (sr_render_points_per_block)", p.in.n_samples, nw * 32);
    return 1;
  }
  const long tiles = (p.in.n_points + 31) / 32;
  const unsigned grid = (unsigned)((tiles + nw - 1) / nw);
  if (!ensure_dynamic_lds((const void*)kern, lds)) return 1;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(nw * 64), lds, st, p);
  return check_launch(name);
}

template <int NPASS, int AUXS, int SAVE, int KG, bool REND = false>
int launch_one(const FwdParams& p, hipStream_t st) {
  using FS = FwdStream<AUXS>;
  static_assert(FS::N_TRUNK % (2 * KG) == 0 && FS::NCH % KG == 0 && kMT % KG == 0, "chunk groups must tile the stream and the ring");
  const size_t ring = (size_t)ring_slots<KG>() * FS::SLOTP * Mode<NPASS>::PIECE_BYTES + kFeat * sizeof(float4);
  return launch_fwd_kernel(satnerf_fwd_kernel<NPASS, AUXS, SAVE, KG, REND>, "satnerf_fwd_kernel", Mode<NPASS>::NW, ring, REND ? 6 : 0, p, st);  // 6: no beta in LDS
}

#ifndef SR_FWD_GROUP
#define SR_FWD_GROUP 4
#endif
#ifndef SR_SAVE_GROUP
#define SR_SAVE_GROUP 2
#endif
#ifndef SR_SAVE8_GROUP
#define SR_SAVE8_GROUP 2
#endif
template <int NPASS, int AUXS>
int launch_fwd(const FwdParams& p, int save_fmt, hipStream_t st) {
  if (p.rend.rays != nullptr) {  // the fused render pass: inference only
    if (save_fmt != 0) {
      set_error("sr_satnerf_render_fwd does not save activations");
      return 1;
    }
    constexpr int KGR = kFeat != 256 ? 2 : (NPASS == 1 ? SR_FWD_GROUP : 2);
    return launch_one<NPASS, AUXS, 0, KGR, true>(p, st);
  }
  if constexpr (kFeat != 256) {  // the wide build: inference only, throughput arithmetic only (512 VGPRs hold one bf16 plane)
    if (save_fmt == SR_FMT8) return launch_one<NPASS, AUXS, SR_FMT8, 2>(p, st);  // training: the 8-bit workspaces only
    if (save_fmt != 0) {
      set_error("sr_satnerf_mlp_fwd: feat=%d saves activations in the 8-bit format only", kFeat);
      return 1;
    }
    return launch_one<NPASS, AUXS, 0, 2>(p, st);  // ring of 2 x 2 slots of 33-34 KiB
  } else {
  // saving activations: bf16 with a rendezvous per 2 chunks (110 -> 107 us against one per chunk; 4 is no better), bf16x3 per chunk
  if (save_fmt == SR_FMT16) return launch_one<NPASS, AUXS, SR_FMT16, NPASS == 1 ? SR_SAVE_GROUP : 1>(p, st);
  if (save_fmt == SR_FMT8) {
    if constexpr (NPASS == 1) return launch_one<NPASS, AUXS, SR_FMT8, SR_SAVE8_GROUP>(p, st);
    set_error("sr_satnerf_mlp_fwd: the 8-bit workspace format belongs to SR_MODE_BF16 (the parity mode saves 16 bits)");
    return 1;
  }
  constexpr int KG = NPASS == 1 ? SR_FWD_GROUP : 2;  // inference: one rendezvous per group of chunks (BF16X3: 2 x 34-KiB slots per group)
  return launch_one<NPASS, AUXS, 0, KG>(p, st);
  }
}
}  // inline namespace SR_FEAT_NS
}  // namespace sr
