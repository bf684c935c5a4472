// Fused Sat-NeRF MLP backward, data-gradient chain ("dX") for gfx950.
//
// Replaces autograd's backward through SatNeRF.forward (models/satnerf.py:156-208) for every sample point: starting
// from the gradients of the four per-point outputs it walks the network in reverse, register-resident exactly like the
// forward kernel (swapped orientation, 32 points per wave, transposed weights streamed L2 -> LDS ring, see mlp_layout.h),
// and writes the gradient of EVERY pre-activation, as bf16 B fragments, to the `dpre` workspace; the weight-gradient GEMMs
// (wgrad.hip) then contract dpre with the activations the forward pass saved.  No gradient flows to xyz / z / rays
// (inputs are data, rendering.py:122-124 detaches the resampled depths), so fc_net.0 needs no dX.
//
// sin stages: the forward saved the pre-activation PHASE (unorm16 revolutions); d pre = d out * cos(2 pi phase) (for
// fc_net.0 the factor w0 = 30 is applied to its weight gradient by the gather scale, packing.backward_maps).
// Arithmetic: single-pass bf16 MFMA with fp32 accumulation (mixed-precision backward) in both numeric modes.
// Workspace format (template FMT, mlp_layout.h): SR_FMT16 reads unorm16 phases and writes bf16 gradients; SR_FMT8 (the
// throughput mode) reads PHASE8 double fragments and writes the gradients as MX8 (codec8.h) -- the gradient that continues down
// the chain stays bf16 in registers either way, only the copy the weight-gradient kernel reads is 8-bit.
#pragma once
#include "mlp_device.h"
#include "mlp_params.h"
#include "codec8.h"

namespace sr {
inline namespace SR_FEAT_NS {

using BS = BwdStream;
constexpr int kBSlot = BS::SLOTP * 1024;  // ring slot bytes
// 32-point tiles per wave (kBT).  1 = 8 waves x 32 points at width 256 (two waves per SIMD), 4 x 32 at width 512.  2 (width 256: 4 waves x 64
// points, one wave per SIMD, 512 registers) lets every transposed-weight fragment read from the LDS feed two MFMAs; it passes every
// gradient test and runs 144 us instead of 111 as compiler-scheduled code: hipcc parks the second tile's vectors in AGPRs and moves them
// with 2.3 v_accvgpr_read/write per MFMA, and halving the LDS reads of the one-tile kernel (SR_ABL_HALF_LDS, results wrong) buys 3 % --
// the LDS port is not what bounds this kernel (profiles/r04_ab_variants.txt).
#ifndef SR_BWD_TILES
#define SR_BWD_TILES 1
#endif
constexpr int kBT = SR_BWD_TILES;

// LIMIT = first chunk the C++ chunk protocol does NOT request (BS::NCH: the whole stream; BS::G_L when the trunk is the generated
// instruction stream, which feeds the ring by its own LDS-DMA rows)
template <int G, int LIMIT>
__device__ __forceinline__ void bchunk_enter(char* ring, const char* stream, int wave, int lane) {
  constexpr int later = [] {
    int n = 0;
    for (int c = 1; c < kD; ++c) n += G + c < LIMIT ? min_loads<1>(BS::np(G + c)) : 0;
    return n;
  }();
  wait_then_barrier<later>();
  if constexpr (G + kD < LIMIT) {
    constexpr long off = BS::offset_pieces(G + kD) * 1024L;
    constexpr int slot = (G + kD) % kNSLOT;
    issue_chunk<1, BS::np(G + kD)>(stream, nullptr, off, ring + slot * kBSlot, wave, lane);
  }
}

__device__ __forceinline__ float phase_cos(uint32_t w, int half) {
  const uint32_t u = half ? (w >> 16) : (w & 0xffffu);
  return __builtin_amdgcn_cosf((float)u * (1.0f / 65535.0f));  // v_cos_f32 takes revolutions
}

// phases of one output tile's 16 values per lane: SR_FMT16 two unorm16 fragments, SR_FMT8 one PHASE8 double fragment
template <int FMT>
struct Phase {
  uint4 p0, p1;
  __device__ __forceinline__ void load(const uint4* acts_tile, int auxs, int frag) {  // frag = logical fragment of value 0 (even)
    if constexpr (FMT == SR_FMT8) p0 = ws_load(acts_tile + (auxs + (frag >> 1)) * 64);
    else p0 = ws_load(acts_tile + (auxs + frag) * 64), p1 = ws_load(acts_tile + (auxs + frag + 1) * 64);
  }
  __device__ __forceinline__ void from_lds(const char* slot, int lane) {  // staged by stage_phase()
    p0 = *reinterpret_cast<const uint4*>(slot + lane * 16);
    if constexpr (FMT != SR_FMT8) p1 = *reinterpret_cast<const uint4*>(slot + 1024 + lane * 16);
  }
  __device__ __forceinline__ float cos(int g) const {
    if constexpr (FMT == SR_FMT8) {
      const uint32_t pw[4] = {p0.x, p0.y, p0.z, p0.w};
      return __builtin_amdgcn_cosf(phase8_rev(pw[g >> 2], g & 3));
    } else {
      const uint32_t pw[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
      return phase_cos(pw[g >> 1], g & 1);
    }
  }
};

// 16 accumulator values (fragments 2T, 2T+1 of the stage's input vector) -> [x cos(phase)] -> two bf16 fragments (the next
// stage's B operand), stored to the dpre workspace at logical fragment `frag` in the format FMT; returns the MX8 scale byte.
template <bool COS, int FMT>
__device__ __forceinline__ uint32_t bpack(const f32x16& acc, const Phase<FMT>& ph, uint4& o0, uint4& o1, uint4* dpre_tile, int frag) {
  float v[16];
#pragma unroll
  for (int g = 0; g < 16; ++g) v[g] = COS ? acc[g] * ph.cos(g) : acc[g];
  o0 = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
  o1 = make_uint4(pack_bf16x2(v[8], v[9]), pack_bf16x2(v[10], v[11]), pack_bf16x2(v[12], v[13]), pack_bf16x2(v[14], v[15]));
  if constexpr (FMT == SR_FMT8) {
    const uint32_t e = mx8_exponent(v, o0.x);  // `after` = o0.x: the pack above has READ v[0], v[1] as ordinary instructions, so the compiler has padded the MFMA -> VALU wait for the whole accumulator (codec8.h contract)
    ws_store(dpre_tile + dp8_unit(frag) * 64, mx8_encode(v, e));
    return e;
  } else {
    ws_store(dpre_tile + frag * 64, o0);
    ws_store(dpre_tile + (frag + 1) * 64, o1);
    return 0u;
  }
}
// largest byte of the first NT bytes packed in eb[]
template <int NT>
__device__ __forceinline__ uint32_t max_byte(const uint32_t (&eb)[4]) {
  uint32_t m = 0;
#pragma unroll
  for (int w = 0; w < (NT + 3) / 4; ++w) {
    const uint32_t a = eb[w] & 0xffu, b = (eb[w] >> 8) & 0xffu, c = (eb[w] >> 16) & 0xffu, d = eb[w] >> 24;
    const uint32_t ab = a > b ? a : b, cd = c > d ? c : d;
    m = m > ab ? m : ab, m = m > cd ? m : cd;
  }
  return m;
}
// maximum of v over the wave, in an SGPR: four row_shr prefix steps, two row broadcasts (lane 63 holds the result), one readlane -- 7
// instructions, no LDS.  (64 lanes doing an LDS atomic on ONE address cost ~8 cycles per lane: 15 of them per wave made this kernel 30 %
// slower.)  update_dpp(old = 0, ...): lanes without a source keep the identity of an unsigned maximum.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_max_step(uint32_t v) {
  const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
  return v > o ? v : o;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  v = dpp_max_step<0x111, 0xf>(v);  // row_shr:1
  v = dpp_max_step<0x112, 0xf>(v);  // row_shr:2
  v = dpp_max_step<0x114, 0xf>(v);  // row_shr:4
  v = dpp_max_step<0x118, 0xf>(v);  // row_shr:8: lane 15 of every row of 16 holds the row's maximum
  v = dpp_max_step<0x142, 0xa>(v);  // row_bcast:15 into rows 1, 3
  v = dpp_max_step<0x143, 0xc>(v);  // row_bcast:31 into rows 2, 3
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// one cell of the wave's row of the exponent maxima (LDS, [wave * kBT + tile][16]): written by one lane, no atomics -- the entry's waves
// are combined when the table is written at the end of the kernel
__device__ __forceinline__ void note_emax(uint32_t* emax, int group, uint32_t lane_max, int lane) {
  const uint32_t m = wave_max_u32(lane_max);
  if (lane == 0) emax[group] = m;
}
// scale bytes of a group's NT tiles (SR_FMT8) into the group's slot of the scale units (mlp_layout.h); their maximum over the lanes goes
// to the wave's cell of the exponent maxima (`emax` = this tile's 16 cells)
template <int FMT, int NT>
__device__ __forceinline__ void store_scales(uint4* dpre_tile, int group, const uint32_t (&eb)[4], uint32_t* emax) {
  if constexpr (FMT == SR_FMT8) {
    note_emax(emax, group, max_byte<NT>(eb), (int)(threadIdx.x & 63));
    char* p = reinterpret_cast<char*>(dpre_tile + (kD8Scale + group / kD8GroupsPerUnit) * 64) + (group % kD8GroupsPerUnit) * kMT;
    if constexpr (NT > 8) *reinterpret_cast<uint4*>(p) = make_uint4(eb[0], eb[1], eb[2], eb[3]);
    else if constexpr (NT > 4) *reinterpret_cast<uint2*>(p) = make_uint2(eb[0], eb[1]);
    else *reinterpret_cast<uint32_t*>(p) = eb[0];
  }
}

// one output tile of each of the wave's kBT point tiles: acc[j] = sum_i A(piece P0+i of the slot) x in[j][i]; an A fragment is read once
template <int KIN>
__device__ __forceinline__ void btile(const char* slot, int p0, const uint4 (&in)[kBT][KIN], f32x16 (&acc)[kBT], int lane) {
#pragma unroll
  for (int j = 0; j < kBT; ++j) acc[j] = f32x16{0};
  uint4 a = {};
#pragma unroll
  for (int i = 0; i < KIN; ++i) {
#ifdef SR_ABL_HALF_LDS  // timing experiment (results wrong): every second A fragment is not read, the previous one is used again
    if (i % 2 == 0)
#endif
    a = *reinterpret_cast<const uint4*>(slot + (p0 + i) * 1024 + lane * 16);
#pragma unroll
    for (int j = 0; j < kBT; ++j) acc[j] = mfma(a, in[j][i], acc[j]);
  }
}
// acc[j] += sum_i A(piece i of the slot) x in[j][OFF + i], i < NP: one part of an output tile whose pieces span several chunks
template <int NP, int OFF, int KIN>
__device__ __forceinline__ void btile_part(const char* slot, const uint4 (&in)[kBT][KIN], f32x16 (&acc)[kBT], int lane) {
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const uint4 a = *reinterpret_cast<const uint4*>(slot + i * 1024 + lane * 16);
#pragma unroll
    for (int j = 0; j < kBT; ++j) acc[j] = mfma(a, in[j][OFF + i], acc[j]);
  }
}

// ---- trunk schedule ---------------------------------------------------------------------------------------------------------
// In the trunk (7 layers x 8 output tiles, two thirds of the kernel) every vector-memory LOAD of a wave is an LDS-DMA issued
// through inline asm -- the weight chunks into the shared ring, the tile's saved phases into a wave-private staging ring -- so
// the compiler never sees a load it would have to wait for (left to hipcc, each tile's phase load became an s_waitcnt vmcnt(0)
// that also drained the weight prefetch and the workspace stores: 62 % of the wave cycles were spent parked, PMC r02a).  The
// waits are ours and counted: LOADS retire in order, the instruction stream of a wave is fixed, so the number of vector-memory
// loads issued after the one being waited for is a compile-time constant of the position in the layer (stores share the counter
// but complete out of order with respect to loads: they are left out of the count, which can only make a wait longer).
// Per layer (NP = phase DMAs per tile, NS = workspace stores per tile, ND = weight DMAs per group of 2 chunks):
//   tile t:   [t even: wait A(t), s_barrier, ND weight DMAs for chunks t+2, t+3]  NP phase DMAs for tile t+2  MFMAs(t)
//             [t > 0: wait B(t-1), epilogue(t-1) = cos, pack, encode, NS stores]
//   end:      wait B(7), epilogue(7), scale store (NSS)
template <int NP, int NS, int NSS>
struct TrunkSched {
  static constexpr int ND = 2 * kKS / Mode<1>::NW;  // 2 chunks x kKS pieces spread over the workgroup's waves
  static constexpr int tile_len(int t) { return (t % 2 == 0 ? ND : 0) + NP + (t > 0 ? NS : 0); }
  static constexpr int tile_start(int t) {
    int p = 0;
    for (int k = 0; k < t; ++k) p += tile_len(k);
    return p;
  }
  static constexpr int period() { return tile_start(kMT) + NS + NSS; }
  static constexpr int after_d(int t) { return tile_start(t) + ND; }                          // just after the weight DMAs of tile t (even)
  static constexpr int after_p(int t) { return tile_start(t) + (t % 2 == 0 ? ND : 0) + NP; }  // just after the phase DMAs issued in tile t
  static constexpr int at_store(int t) { return t < kMT - 1 ? after_p(t + 1) : tile_start(kMT); }  // where epilogue(t)'s wait sits
  // instructions issued after the phase DMAs of tile t (issued in tile t-2; in the previous layer -- or the prologue -- for t < 2)
  static constexpr int wait_b(int t) {
    if (t >= 2) return at_store(t) - after_p(t - 2);
    const int steady = at_store(t) - (after_p(t + kMT - 2) - period());
    const int first = t == 0 ? NP + at_store(0) : at_store(1);  // first layer: phases of tiles 0, 1 are staged by the prologue
    return steady < first ? steady : first;
  }
  // instructions issued after the weight DMAs of tile t's group (issued at the entry of tile t-2)
  static constexpr int wait_a(int t) { return t >= 2 ? tile_start(t) - after_d(t - 2) : tile_start(0) - (after_d(kMT - 2) - period()); }
};

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- phases of the stages before the trunk ---------------------------------------------------------------------------------
// The 28 output tiles before the trunk that multiply by cos(phase) -- bH (12: rgb hidden, sun hidden 3, beta hidden), bS3 (4), bS2
// (4), bG1 (8) -- take their phases the same way: LDS-DMA into the wave's 4-slot staging ring TWO phase tiles ahead (tile k + 2
// is requested right after tile k is used; tiles 0, 1 by the prologue), counted wait before the use.  The instruction stream is
// static, so the loads issued between a request and its use are known: the phase DMAs of tile k + 1 and the weight DMAs of every
// chunk entered in between (at least min_loads per wave).  PreSched replays that stream at compile time.
struct PreSched {
  static constexpr int kTiles = 3 * kMTH + kMTH + kMTH + kMT;  // 28 at feat 256
  // phase tile k -> logical activation fragment of its first value
  static constexpr int frag(int k) {
    if (k < 3 * kMTH) {
      const int part = k / kMTH, t = k % kMTH;
      return (part == 0 ? kActRgbh : part == 1 ? kActS3 : kActE1) + 2 * t;
    }
    k -= 3 * kMTH;
    if (k < kMTH) return kActS2 + 2 * k;  // bS3 multiplies by cos(phase s2)
    k -= kMTH;
    if (k < kMTH) return kActS1 + 2 * k;  // bS2: cos(phase s1)
    return kActA0 + 7 * kKS + 2 * (k - kMTH);  // bG1: cos(phase a7)
  }
  static constexpr int chunk_of(int k) {  // the chunk in which phase tile k is used
    if (k < 3 * kMTH) return BS::G_H;
    k -= 3 * kMTH;
    if (k < kMTH) return BS::G_S3 + k / 2;
    k -= kMTH;
    if (k < kMTH) return BS::G_S2 + k / 2;
    return BS::G_G1 + (k - kMTH);
  }
  // Phase tiles are requested kAhead = 4 tiles ahead (r05; the staging ring has 4 slots: tile k + 4 goes into the slot tile k has just been
  // read from): two tiles ahead -- r04 -- is ~1,500 cycles of lead in bH, whose tiles are ONE MFMA and an epilogue, against a memory latency
  // of 2-4 k cycles under load: every bH tile waited for its phases (stage stamps: 18 k cycles for 12 MFMAs + 12 epilogues, floor ~7 k).
  static constexpr int kAhead = 4;
  // loads (lower bound per wave) issued after the request of phase tile k and before its use; nph = phase DMAs per tile.
  // Request points: tiles 0 .. kAhead - 1 in the prologue (after the DMAs of chunks 0..2, before chunk 0 is entered); tile k >= kAhead
  // right after the use of tile k - kAhead, i.e. inside chunk_of(k - kAhead).  Entering chunk g requests chunk g + kD (below `limit`).
  static constexpr int wait(int k, int nph, int limit) {
    int n = 0;
    const int req_chunk = k >= kAhead ? chunk_of(k - kAhead) : -1;
    for (int g = req_chunk + 1; g <= chunk_of(k); ++g) n += g + kD < limit ? min_loads<1>(BS::np(g + kD)) : 0;  // chunks entered after the request
    const int later = kTiles - 1 - k < kAhead - 1 ? kTiles - 1 - k : kAhead - 1;  // tiles k + 1 .. k + kAhead - 1 are requested in between
    n += nph * later;
    return n < 63 ? n : 63;        // vmcnt is a 6-bit field; a smaller count only waits longer
  }
};

// generic transposed stage: NCHUNK chunks of TPC tiles, each KIN pieces; tile t -> out[2t], out[2t+1], stored to the dpre
// workspace from logical fragment DF0; AF0 = logical activation fragment of the stage's phases (COS stages)
// PK0 = phase-tile index (PreSched) of the stage's first tile; `stage` = the wave's phase staging ring, request(slot, frag) = LDS-DMA
// of a phase tile into it
template <int FMT, int LIMIT, int KIN, int TPC, int NCHUNK, int G0, bool COS, int NOUT, int PK0, int DF0, class Req>
__device__ __forceinline__ void bstage(const uint4 (&in)[kBT][KIN], uint4 (&out)[kBT][NOUT], char* ring, const char* stream, int wave, int lane,
                                       const char* stage, Req&& request, uint4* const (&dpre_tile)[kBT], uint32_t* const (&emax)[kBT]) {
  constexpr int NPH = FMT == SR_FMT8 ? 1 : 2;
  uint32_t eb[kBT][4] = {};
  static_for<NCHUNK>([&](auto cc) {
    constexpr int c = decltype(cc)::value, g = G0 + c;
    static_assert(BS::np(g) == TPC * KIN, "backward stream geometry mismatch");
    bchunk_enter<g, LIMIT>(ring, stream, wave, lane);
    const char* slot = ring + (g % kNSLOT) * kBSlot;
    static_for<TPC>([&](auto tc) {
      constexpr int tt = decltype(tc)::value, t = c * TPC + tt, o = 2 * t;
      Phase<FMT> ph[kBT] = {};
      f32x16 acc[kBT];
      btile<KIN>(slot, tt * KIN, in, acc, lane);
      if constexpr (COS) {
        constexpr int k = PK0 + t;
        wait_vmcnt<PreSched::wait(k, kBT * NPH, LIMIT)>();
#pragma unroll
        for (int j = 0; j < kBT; ++j) ph[j].from_lds(stage + ((k & 3) * kBT + j) * NPH * 1024, lane);
      }
#pragma unroll
      for (int j = 0; j < kBT; ++j)
        eb[j][t >> 2] |= bpack<COS, FMT>(acc[j], ph[j], out[j][o], out[j][o + 1], dpre_tile[j], DF0 + 2 * t) << (8 * (t & 3));
      if constexpr (COS && PK0 + t + PreSched::kAhead < PreSched::kTiles) request((PK0 + t + PreSched::kAhead) & 3, PreSched::frag(PK0 + t + PreSched::kAhead));
    });
  });
#pragma unroll
  for (int j = 0; j < kBT; ++j) store_scales<FMT, TPC * NCHUNK>(dpre_tile[j], dp8_group(DF0), eb[j], emax[j]);
}

// TRUNK_ASM: the seven trunk layers run the generated instruction stream (gen/bwd_core.py -> mlp_bwd_trunk_a{1,2}.inc at width 256,
// mlp_bwd512_trunk_a{1,2}.inc at width 512) instead of the compiler-scheduled loop below (8-bit workspaces, one tile per wave,
// workspaces below 4 GiB: launch_bwd_fmt decides)
typedef uint32_t u32x32w __attribute__((ext_vector_type(32)));
typedef uint32_t u32x4w __attribute__((ext_vector_type(4)));
template <int FMT, bool TRUNK_ASM = false>
__global__ void __launch_bounds__(Mode<1>::NW * 64) satnerf_bwd_kernel(const BwdParams prm) {
  constexpr int NW = Mode<1>::NW;
  // the generated stream starts at the trunk; starting one stage earlier, at bG1 (gen/bwd_core.py Geo.g1), is wired but measured slower at
  // either width (r05: spills at 256, 440 vs 426 us at 512) -- keep in step with Geo.g1
  constexpr bool kStreamG1 = false;
  constexpr int LIMIT = !TRUNK_ASM ? BS::NCH : kStreamG1 ? BS::G_G1 : BS::G_L;  // chunks the C++ chunk protocol requests  // 8 waves of <= 256 VGPRs at feat 256, 4 of <= 512 at feat 512 (or with kBT = 2); kBT 32-point tiles each
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem;
#ifdef SR_BWD_TIMING
  const uint64_t t_kernel0 = __builtin_amdgcn_s_memtime(), r_kernel0 = __builtin_amdgcn_s_memrealtime();
#endif
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, pl = lane & 31;
  const char* stream = prm.stream;
  const int A = prm.auxs, AK = FMT == SR_FMT8 ? act8_units(prm.auxs) : act_ksteps(prm.auxs);
  constexpr int DK = FMT == SR_FMT8 ? kD8Units : kDpFrags;  // workspace units per tile

#pragma unroll
  for (int g = 0; g < kD; ++g) {
    if (g == 0) issue_chunk<1, BS::np(0)>(stream, nullptr, 0, ring, wave, lane);
    if (g == 1) issue_chunk<1, BS::np(1)>(stream, nullptr, BS::offset_pieces(1) * 1024L, ring + kBSlot, wave, lane);
    if (g == 2) issue_chunk<1, BS::np(2)>(stream, nullptr, BS::offset_pieces(2) * 1024L, ring + 2 * kBSlot, wave, lane);
  }

#ifdef SR_BWD_REVERSE
  const long tile0 = ((long)(gridDim.x - 1 - blockIdx.x) * NW + wave) * kBT;  // newest activations first: whatever the Infinity Cache kept
#else
  const long tile0 = ((long)blockIdx.x * NW + wave) * kBT;  // the wave's tiles are consecutive: tile0 + j
#endif
  long pt[kBT];
  bool valid[kBT];
  uint4* dpre[kBT];  // + unit * 64
#pragma unroll
  for (int j = 0; j < kBT; ++j) {
    pt[j] = (tile0 + j) * 32 + pl;
    valid[j] = pt[j] < prm.n_points;
    dpre[j] = prm.dpre + (tile0 + j) * DK * 64 + lane;
  }

  // ---- gradients of the head pre-activations (rows 0..2 albedo logits, 3 sun logit, 4 beta; sigma separately) ----------
  uint4 dhead[kBT][1], dsig[kBT];
  uint32_t e_feats[kBT] = {}, e_raw[kBT] = {};  // SR_FMT8: lane maxima of the feats exponents the FORWARD saved / of the two bf16 row fragments
#pragma unroll
  for (int j = 0; j < kBT; ++j) {
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, sg = 0.f;
    const long q = pt[j];
    uint4 fs = {};
    if constexpr (FMT == SR_FMT8)  // the lane's 16 bytes of the tile's feats scale unit (kMT of them valid): fetched with the loads below
      fs = prm.acts[((tile0 + j) * (long)act8_units(prm.auxs) + prm.auxs + kA8Scale) * 64 + lane];
    if (valid[j]) {
      if (h == 0) {
        if (prm.g_albedo) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float s = (prm.albedo[q * 3 + c] + 0.001f) * (1.0f / 1.002f);  // sigmoid output before the rgb_padding affine
            v[c] = prm.g_albedo[q * 3 + c] * 1.002f * s * (1.0f - s);
          }
        }
        if (prm.g_sun) {
          const float s = prm.sun_v[q];
          v[3] = prm.g_sun[q] * s * (1.0f - s);
        }
        if (prm.g_sigma) sg = prm.g_sigma[q] * (1.0f - expf(-prm.sigma[q]));  // softplus' = 1 - exp(-softplus)
      } else if (prm.g_beta) {
        v[0] = prm.g_beta[q] * (1.0f - expf(-prm.beta[q]));
      }
    }
    dhead[j][0] = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
    dsig[j] = make_uint4(pack_bf16x2(sg, 0.f), 0u, 0u, 0u);
    dpre[j][(FMT == SR_FMT8 ? kD8Head : kDpHead) * 64] = dhead[j][0];
    dpre[j][(FMT == SR_FMT8 ? kD8Sigma : kDpSigma) * 64] = dsig[j];
    if constexpr (FMT == SR_FMT8) {
      const uint32_t w4[4] = {fs.x, fs.y, kMT > 8 ? fs.z : 0u, kMT > 8 ? fs.w : 0u};
      e_feats[j] = max_byte<kMT>(w4);
      const uint32_t hw[5] = {dhead[j][0].x, dhead[j][0].y, dhead[j][0].z, dhead[j][0].w, dsig[j].x};
      uint32_t m = 0;
#pragma unroll
      for (int k = 0; k < 5; ++k) {  // biased exponents of the bf16 halves
        const uint32_t lo = (hw[k] & 0x7fffu) >> 7, hi = (hw[k] >> 23) & 0xffu;
        m = m > lo ? m : lo, m = m > hi ? m : hi;
      }
      e_raw[j] = m;
    }
  }

  // this wave's phase staging ring (4 slots x kBT tiles) behind the weight ring; the first two phase tiles are requested now
  constexpr int NPH = FMT == SR_FMT8 ? 1 : 2;  // phase units per tile
  constexpr int NPT = kBT * NPH;               // phase DMAs per request
  char* stage = smem + kNSLOT * kBSlot + wave * (4 * NPT * 1024);
  const uint32_t stage_addr = __builtin_amdgcn_readfirstlane(lds_addr_of(stage));
  auto stage_phase = [&](int slot, int frag) {  // frag = logical activation fragment of the tile's first value
#ifdef SR_ABL_NO_PHASE_LOADS  // timing experiment (tools/ab_bwd_abl.sh): phases = whatever the LDS holds
    return;
#endif
    // wave-uniform base (this wave's tiles) + the lane's fixed 16-byte offset: no VALU address arithmetic per request
#pragma unroll
    for (int j = 0; j < kBT; ++j) {
      const char* src = reinterpret_cast<const char*>(prm.acts + ((tile0 + j) * AK + A + (FMT == SR_FMT8 ? frag >> 1 : frag)) * 64);
#pragma unroll
      for (int k = 0; k < NPH; ++k) glds16_s(src + k * 1024, (uint32_t)lane * 16u, stage_addr + ((slot * kBT + j) * NPH + k) * 1024);
    }
  };
  auto phases_of = [&](int slot, Phase<FMT> (&ph)[kBT]) {
#pragma unroll
    for (int j = 0; j < kBT; ++j) ph[j].from_lds(stage + (slot * kBT + j) * NPH * 1024, lane);
  };
  static_assert(PreSched::kAhead == 4, "the wave's phase staging ring has four slots");
  stage_phase(0, PreSched::frag(0)), stage_phase(1, PreSched::frag(1)), stage_phase(2, PreSched::frag(2)), stage_phase(3, PreSched::frag(3));

  // ---- exponent maxima (SR_FMT8; mlp_layout.h): 16 LDS cells per (wave, tile) behind the phase staging ring; every cell is written
  // once by its wave (store_scales / below), the entries of kEmaxTiles tiles each are assembled at the end of the kernel
  uint32_t* emax_cells = reinterpret_cast<uint32_t*>(smem + kNSLOT * kBSlot + NW * (4 * NPT * 1024));
  uint32_t* emax[kBT];
#pragma unroll
  for (int j = 0; j < kBT; ++j) emax[j] = emax_cells + (wave * kBT + j) * 16;
  if constexpr (FMT == SR_FMT8) {
#pragma unroll
    for (int j = 0; j < kBT; ++j) note_emax(emax[j], kEmaxFeats, e_feats[j], lane), note_emax(emax[j], kEmaxRaw, e_raw[j], lane);
  }

#ifdef SR_BWD_TIMING
  uint64_t t_stage[5];
  t_stage[0] = __builtin_amdgcn_s_memtime();
#endif
  // ---- bH: d_head -> d rgb-hidden | d sun-hidden-3 | d beta-hidden (12 tiles x 1 piece, one chunk) --------------------
  uint4 d_rgbh[kBT][kHS], d_s3[kBT][kHS], d_e1[kBT][kHS];
  {
    bchunk_enter<BS::G_H, LIMIT>(ring, stream, wave, lane);
    const char* slot = ring + (BS::G_H % kNSLOT) * kBSlot;
    uint32_t eb[kBT][3][4] = {};
    static_for<3 * kMTH>([&](auto tc) {
      constexpr int T = decltype(tc)::value, part = T / kMTH, t = T % kMTH;
      constexpr int dp0 = part == 0 ? kDpRgbh : (part == 1 ? kDpS3 : kDpE1);
      f32x16 acc[kBT];
      btile<1>(slot, T, dhead, acc, lane);
      wait_vmcnt<PreSched::wait(T, NPT, LIMIT)>();
      Phase<FMT> ph[kBT];
      phases_of(T & 3, ph);
#pragma unroll
      for (int j = 0; j < kBT; ++j) {
        uint4 o0, o1;
        eb[j][part][t >> 2] |= bpack<true, FMT>(acc[j], ph[j], o0, o1, dpre[j], dp0 + 2 * t) << (8 * (t & 3));
        if constexpr (part == 0) d_rgbh[j][2 * t] = o0, d_rgbh[j][2 * t + 1] = o1;
        else if constexpr (part == 1) d_s3[j][2 * t] = o0, d_s3[j][2 * t + 1] = o1;
        else d_e1[j][2 * t] = o0, d_e1[j][2 * t + 1] = o1;
      }
      stage_phase((T + PreSched::kAhead) & 3, PreSched::frag(T + PreSched::kAhead));
    });
#pragma unroll
    for (int j = 0; j < kBT; ++j) {
      store_scales<FMT, kMTH>(dpre[j], dp8_group(kDpRgbh), eb[j][0], emax[j]);
      store_scales<FMT, kMTH>(dpre[j], dp8_group(kDpS3), eb[j][1], emax[j]);
      store_scales<FMT, kMTH>(dpre[j], dp8_group(kDpE1), eb[j][2], emax[j]);
    }
  }
#ifdef SR_BWD_TIMING
  t_stage[1] = __builtin_amdgcn_s_memtime();
#endif
  // ---- sun chain: bS3 (d s3 -> d s2), bS2 (d s2 -> d s1) -------------------------------------------------------------
  uint4 d_g2[kBT][3 * kHS];  // [d rgbh | d s1 | d e1] : the input of bG2
  {
    uint4 d_s2[kBT][kHS], d_s1[kBT][kHS];
    bstage<FMT, LIMIT, kHS, 2, kMTH / 2, BS::G_S3, true, kHS, 3 * kMTH, kDpS2>(d_s3, d_s2, ring, stream, wave, lane, stage, stage_phase, dpre, emax);
    bstage<FMT, LIMIT, kHS, 2, kMTH / 2, BS::G_S2, true, kHS, 4 * kMTH, kDpS1>(d_s2, d_s1, ring, stream, wave, lane, stage, stage_phase, dpre, emax);
#pragma unroll
    for (int j = 0; j < kBT; ++j) {
#pragma unroll
      for (int i = 0; i < kHS; ++i) d_g2[j][i] = d_rgbh[j][i], d_g2[j][kHS + i] = d_s1[j][i], d_g2[j][2 * kHS + i] = d_e1[j][i];
    }
  }
#ifdef SR_BWD_TIMING
  t_stage[2] = __builtin_amdgcn_s_memtime();
#endif
  // ---- bG2: -> d feats (identity stage), bDT: d beta-hidden -> d t (embedding columns) ------------------------------
  uint4 d_g1[kBT][kKS + 1];  // [d feats (16) | d sigma_pre (1)] : the input of bG1
  {
    uint4 d_feats[kBT][kKS];
    {  // bG2: a tile's 3 kHS pieces arrive as kG2Split chunks
      uint32_t eb[kBT][4] = {};
      static_for<kMT>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        f32x16 acc[kBT];
#pragma unroll
        for (int j = 0; j < kBT; ++j) acc[j] = f32x16{0};
        static_for<BS::kG2Split>([&](auto sc) {
          constexpr int sp = decltype(sc)::value, g = BS::G_G2 + t * BS::kG2Split + sp;
          static_assert(BS::np(g) == BS::kG2Part, "backward stream geometry mismatch");
          bchunk_enter<g, LIMIT>(ring, stream, wave, lane);
          btile_part<BS::kG2Part, sp * BS::kG2Part>(ring + (g % kNSLOT) * kBSlot, d_g2, acc, lane);
        });
        Phase<FMT> none = {};
#pragma unroll
        for (int j = 0; j < kBT; ++j)
          eb[j][t >> 2] |= bpack<false, FMT>(acc[j], none, d_feats[j][2 * t], d_feats[j][2 * t + 1], dpre[j], kDpFeats + 2 * t) << (8 * (t & 3));
      });
#pragma unroll
      for (int j = 0; j < kBT; ++j) store_scales<FMT, kMT>(dpre[j], dp8_group(kDpFeats), eb[j], emax[j]);
    }
    bchunk_enter<BS::G_DT, LIMIT>(ring, stream, wave, lane);
    f32x16 acc[kBT];
    btile<kHS>(ring + (BS::G_DT % kNSLOT) * kBSlot, 0, d_e1, acc, lane);
#pragma unroll
    for (int j = 0; j < kBT; ++j) {
      if (valid[j] && prm.d_t) {
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const int row = (g & 3) + 8 * (g >> 2) + 4 * h;  // = embedding component
          if (row < prm.tau) prm.d_t[pt[j] * prm.tau + row] = acc[j][g];
        }
      }
#pragma unroll
      for (int i = 0; i < kKS; ++i) d_g1[j][i] = d_feats[j][i];
      d_g1[j][kKS] = dsig[j];
    }
  }
#ifdef SR_BWD_TIMING
  t_stage[3] = __builtin_amdgcn_s_memtime();
#endif
  // ---- bG1: -> d a7, x cos(phase a7) = d pre_7 ----------------------------------------------------------------------
  uint4 cur[kBT][kKS], nxt[kBT][kKS];
  if constexpr (!kStreamG1)
    bstage<FMT, LIMIT, kKS + 1, 1, kMT, BS::G_G1, true, kKS, 5 * kMTH, kDpL + 7 * kKS>(d_g1, cur, ring, stream, wave, lane, stage, stage_phase, dpre, emax);
  // ---- bL7 .. bL1: d pre_l -> d a_{l-1}, x cos(phase a_{l-1}) = d pre_{l-1}; scheduled by TrunkSched (above) -------------------
  constexpr long offL = BS::offset_pieces(BS::G_L);
  // stores are NOT counted (NS = NSS = 0): loads retire in order among themselves, but a store may complete before an older load,
  // so only "younger LOADS still outstanding" proves that an older load has landed; the price is an occasional wait for a store
  using TS = TrunkSched<NPT, 0, 0>;  // (counting the stores as well measured the same: 138.3 vs 139.6 us)
  // G1's chunk protocol already requested the first trunk chunks; drain everything once and start from a known queue
  wait_then_barrier<0>();
#ifdef SR_BWD_TIMING
  t_stage[4] = __builtin_amdgcn_s_memtime();
#endif
  if constexpr (TRUNK_ASM) {
    // ---- the generated trunk (gen/bwd_core.py): d pre_7 in v[0:4 kKS), ring = the chunk ring, phases straight into registers ----------
    static_assert(FMT == SR_FMT8 && kBT == 1, "the generated trunk reads and writes the 8-bit workspaces, one tile per wave");
    static_assert((kFeat == 256 && NW == 8 && kNSLOT * kBSlot == 96 * 1024) || (kFeat == 512 && NW == 4 && kNSLOT * kBSlot >= 128 * 1024),
                  "the generated trunk's geometry (gen/bwd_core.py Geo)");
    u32x32w xq[kKS / 8];
    u32x4w xs = {0u, 0u, 0u, 0u};  // (kStreamG1) the d sigma_pre fragment of bG1's last k-step
#pragma unroll
    for (int i = 0; i < kKS; ++i) {
      const uint4 f = kStreamG1 ? d_g1[0][i] : cur[0][i];
      xq[i / 8][4 * (i % 8)] = f.x, xq[i / 8][4 * (i % 8) + 1] = f.y, xq[i / 8][4 * (i % 8) + 2] = f.z, xq[i / 8][4 * (i % 8) + 3] = f.w;
    }
    if constexpr (kStreamG1) xs = u32x4w{d_g1[0][kKS].x, d_g1[0][kKS].y, d_g1[0][kKS].z, d_g1[0][kKS].w};
    const uint32_t ring_addr = lds_addr_of(ring);
    const uint32_t vl0 = ring_addr + (uint32_t)lane * 16u, vl1 = vl0 + 65536u;
    uint32_t voff = (uint32_t)wave * 1024u + (uint32_t)lane * 16u;
    uint32_t poff = (uint32_t)((unsigned long)tile0 * AK * 1024ul) + (uint32_t)lane * 16u;  // (launch_bwd_fmt: both workspaces below 4 GiB)
    uint32_t soff = (uint32_t)((unsigned long)tile0 * DK * 1024ul) + (uint32_t)lane * 16u;
    const uint32_t vcell = lds_addr_of(reinterpret_cast<const char*>(emax[0]));
    const uint32_t wb = (uint32_t)__builtin_amdgcn_readfirstlane((int)(ring_addr + (uint32_t)wave * 1024u));
    const uint64_t sb = uniform64(stream + (kStreamG1 ? BS::offset_pieces(BS::G_G1) : offL) * 1024L), ab = uniform64(prm.acts), db = uniform64(prm.dpre);
    const float magic = 12583040.0f;  // 1.5 * 2^23 + 128 (codec8.h mx8_encode)
    const uint32_t k43 = 0x43000000u;
    uint32_t m0save;
#ifdef SR_BWD_TIMING  // experiments: shader cycles of the pre-trunk part / the trunk per wave, written over d_t (tools/ab_bwd_timing.py)
    const uint64_t t_trunk0 = __builtin_amdgcn_s_memtime(), r_trunk0 = __builtin_amdgcn_s_memrealtime();
#endif
#if SR_FEAT == 512  // (register numbers: gen/bwd_core.py Geo(512))
#define SR_TRUNK_OUTS "+{v[0:31]}"(xq[0]), "+{v[32:63]}"(xq[1]), "+{v[64:95]}"(xq[2]), "+{v[96:127]}"(xq[3]), "+{a[124:127]}"(xs), "+{v217}"(voff), "+{v218}"(poff), "+{v219}"(soff), [m0save] "=&s"(m0save)
#define SR_TRUNK_INS "{v212}"(magic), "{v214}"(k43), "{v215}"(vl0), "{v216}"(vl1), "{v220}"(vcell), [sb] "s"(sb), [wb] "s"(wb), [ab] "s"(ab), [db] "s"(db)
#define SR_TRUNK_A1_DEFAULT "mlp_bwd512_trunk_a1.inc"
#define SR_TRUNK_A2 "mlp_bwd512_trunk_a2.inc"
#define SR_TRUNK_CLOBBERS "mlp_bwd512_trunk_clobbers.inc"
#else
#define SR_TRUNK_OUTS "+{v[0:31]}"(xq[0]), "+{v[32:63]}"(xq[1]), "+{v223}"(voff), "+{v224}"(poff), "+{v225}"(soff), [m0save] "=&s"(m0save)
#define SR_TRUNK_INS "{v218}"(magic), "{v220}"(k43), "{v221}"(vl0), "{v222}"(vl1), "{v230}"(vcell), [sb] "s"(sb), [wb] "s"(wb), [ab] "s"(ab), [db] "s"(db)
#define SR_TRUNK_A1_DEFAULT "mlp_bwd_trunk_a1.inc"
#define SR_TRUNK_A2 "mlp_bwd_trunk_a2.inc"
#define SR_TRUNK_CLOBBERS "mlp_bwd_trunk_clobbers.inc"
#endif
#ifndef SR_TRUNK_A1
#define SR_TRUNK_A1 SR_TRUNK_A1_DEFAULT
#endif
    if (prm.auxs == 1) {
      asm volatile(
#include SR_TRUNK_A1
          : SR_TRUNK_OUTS
          : SR_TRUNK_INS
          :
#include SR_TRUNK_CLOBBERS
      );
    } else {
      asm volatile(
#include SR_TRUNK_A2
          : SR_TRUNK_OUTS
          : SR_TRUNK_INS
          :
#include SR_TRUNK_CLOBBERS
      );
    }
#undef SR_TRUNK_OUTS
#undef SR_TRUNK_INS
#ifdef SR_BWD_TIMING
    {
      const uint64_t t_trunk1 = __builtin_amdgcn_s_memtime(), r_trunk1 = __builtin_amdgcn_s_memrealtime();
      if (lane == 0 && prm.d_t) {
        prm.d_t[tile0 * 8 + 0] = (float)(t_trunk0 - t_kernel0), prm.d_t[tile0 * 8 + 1] = (float)(t_trunk1 - t_trunk0);
        prm.d_t[tile0 * 8 + 2] = (float)(r_trunk1 - r_trunk0), prm.d_t[tile0 * 8 + 3] = (float)(r_trunk0 - r_kernel0);
        prm.d_t[tile0 * 8 + 4] = (float)(t_stage[0] - t_kernel0), prm.d_t[tile0 * 8 + 5] = (float)(t_stage[1] - t_stage[0]);
        prm.d_t[tile0 * 8 + 6] = (float)(t_stage[2] - t_stage[1]), prm.d_t[tile0 * 8 + 7] = (float)(t_stage[3] - t_stage[2]);
      }
    }
#endif
  } else {
  stage_phase(0, kActA0 + 6 * kKS), stage_phase(1, kActA0 + 6 * kKS + 2);
#pragma unroll 1
  for (int l = 7; l >= 1; --l) {
    const long cbase = (long)(7 - l) * kMT;
    const int lfrag = (l - 1) * kKS;                    // logical fragment of a_{l-1} / d_pre_{l-1}
    const int nfrag = l >= 2 ? lfrag - kKS : lfrag;     // ... of the next layer (the last layer re-stages its own: uniform counts)
    f32x16 acc[2][kBT];
    uint32_t eb[kBT][4] = {};
    auto epilogue = [&](auto tc) {
      constexpr int t = decltype(tc)::value;
      Phase<FMT> ph[kBT];
      phases_of(t & 3, ph);
#pragma unroll
      for (int j = 0; j < kBT; ++j)
        eb[j][t >> 2] |= bpack<true, FMT>(acc[t & 1][j], ph[j], nxt[j][2 * t], nxt[j][2 * t + 1], dpre[j], kDpL + lfrag + 2 * t) << (8 * (t & 3));
    };
    static_for<kMT>([&](auto tc) {
      constexpr int t = decltype(tc)::value;
      if constexpr (t % 2 == 0) {
        wait_then_barrier<TS::wait_a(t)>();
#pragma unroll
        for (int k = 2; k < 4; ++k) {  // chunks t+2, t+3 (clamped at the end of the stream: same instruction count every layer)
          long c = cbase + t + k;
          c = c < kTrunkLayers * kMT ? c : kTrunkLayers * kMT - 1;
          issue_chunk<1, kKS>(stream, nullptr, (offL + c * kKS) * 1024L, ring + ((BS::G_L + t + k) % kNSLOT) * kBSlot, wave, lane);
        }
      }
      stage_phase((t + 2) & 3, kActA0 + (t + 2 < kMT ? lfrag : nfrag) + 2 * ((t + 2) % kMT));
      // the wait for tile t-1's phases sits BEFORE tile t's matrix chain (no load is issued in between: the count is the same), so that
      // the chain and the epilogue of tile t-1 share one scheduling region; with one wave per SIMD nothing else would hide the epilogue
      if constexpr (t > 0) wait_vmcnt<TS::wait_b(t - 1)>();
      btile<kKS>(ring + ((BS::G_L + t) % kNSLOT) * kBSlot, 0, cur, acc[t & 1], lane);
      if constexpr (t > 0) epilogue(std::integral_constant<int, t - 1>{});
#ifdef SR_BWD_INTERLEAVE
      if constexpr (t > 0) {  // [1 LDS read, kBT MFMAs, SR_BWD_INTERLEAVE VALU] x kKS
#pragma unroll
        for (int i = 0; i < kKS; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, kBT, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, SR_BWD_INTERLEAVE, 0);
        }
      }
#endif
    });
    wait_vmcnt<TS::wait_b(kMT - 1)>();
    epilogue(std::integral_constant<int, kMT - 1>{});
#pragma unroll
    for (int j = 0; j < kBT; ++j) {
      store_scales<FMT, kMT>(dpre[j], l - 1, eb[j], emax[j]);
#pragma unroll
      for (int i = 0; i < kKS; ++i) cur[j][i] = nxt[j][i];
    }
  }
#ifdef SR_BWD_TIMING
    if (lane == 0 && prm.d_t) {
      const uint64_t t_end = __builtin_amdgcn_s_memtime();
      prm.d_t[tile0 * 8 + 0] = (float)(t_stage[4] - t_kernel0), prm.d_t[tile0 * 8 + 1] = (float)(t_end - t_stage[4]);
      prm.d_t[tile0 * 8 + 2] = 1.f, prm.d_t[tile0 * 8 + 3] = 1.f;
      prm.d_t[tile0 * 8 + 4] = (float)(t_stage[0] - t_kernel0), prm.d_t[tile0 * 8 + 5] = (float)(t_stage[1] - t_stage[0]);
      prm.d_t[tile0 * 8 + 6] = (float)(t_stage[2] - t_stage[1]), prm.d_t[tile0 * 8 + 7] = (float)(t_stage[3] - t_stage[2]);
    }
#endif
  }  // (compiler-scheduled trunk)
  // ---- the workgroup's entries of the exponent-maxima table: entry = kEmaxTiles consecutive (wave, tile) rows of cells -------------
  if constexpr (FMT == SR_FMT8) {
    constexpr int kRows = NW * kBT, kEntries = (kRows + kEmaxTiles - 1) / kEmaxTiles;
    __syncthreads();
    if (tid < kEntries && prm.emax) {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        uint32_t m = 0;
#pragma unroll
        for (int r = 0; r < kEmaxTiles; ++r) {
          const int row = tid * kEmaxTiles + r;
          const uint32_t c = row < kRows ? emax_cells[row * 16 + g] : 0u;
          m = m > c ? m : c;
        }
        w[g >> 2] |= m << (8 * (g & 3));
      }
      prm.emax[(tile0 - (long)wave * kBT) / kEmaxTiles + tid] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
}


template <int FMT, bool TRUNK_ASM>
int launch_bwd_kernel(const BwdParams& p, size_t lds, hipStream_t st) {
  constexpr int NW = Mode<1>::NW;
  if (!ensure_dynamic_lds((const void*)satnerf_bwd_kernel<FMT, TRUNK_ASM>, lds)) return 1;
  const long tiles = (p.n_points + 31) / 32;
  hipLaunchKernelGGL((satnerf_bwd_kernel<FMT, TRUNK_ASM>), dim3((unsigned)((tiles + NW * kBT - 1) / (NW * kBT))), dim3(NW * 64), lds, st, p);
  return check_launch("satnerf_bwd_kernel");
}

template <int FMT>
int launch_bwd_fmt(const BwdParams& p, hipStream_t st) {
  constexpr int NW = Mode<1>::NW;
  // weight ring + per-wave phase staging + the cells of the exponent maxima
  const size_t lds = (size_t)kNSLOT * kBSlot + NW * 4 * kBT * (FMT == SR_FMT8 ? 1 : 2) * 1024 + (FMT == SR_FMT8 ? NW * kBT * 64 : 0);
  if constexpr (FMT == SR_FMT8 && (kFeat == 256 || kFeat == 512) && kBT == 1) {
    // the generated trunk addresses both workspaces by 32-bit per-lane offsets; SATNERF_BWD_V1=1 keeps the compiler-scheduled trunk (A/B)
    const char* e = getenv("SATNERF_BWD_V1");  // (read per launch: the A/B test flips it inside one process)
    const bool v1 = e && e[0] == '1';
    const unsigned long big = (unsigned long)ws_tiles(p.n_points) * (kD8Units > act8_units(2) ? kD8Units : act8_units(2)) * 1024ul;
    if (!v1 && big < (1ul << 32)) return launch_bwd_kernel<FMT, true>(p, lds, st);
  }
  return launch_bwd_kernel<FMT, false>(p, lds, st);
}

}  // inline namespace SR_FEAT_NS
}  // namespace sr
