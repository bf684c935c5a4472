// Fused classic-NeRF forward for gfx950 (width 256, single-pass bf16 operands, fp32 accumulation): one launch evaluates both positional
// encodings, the 8 x 256 ReLU trunk with its encoded-xyz skip, the density head and the direction-conditioned colour head for every
// sample point -- and, in the render entry, the stratified depths in front and the compositing behind.
//
// Replaces: Mapping.forward models/nerf.py:53-69 + NeRF.forward models/nerf.py:184-227 (12 launches of csrc/linear.hip and two of
// positional_map_kernel per pass in satnerf_amd/generic.py: nerf_points), and with REND rendering.py:62-81 + models/nerf.py:71-133.
//
// Same decomposition as mlp_fwd.inc, whose building blocks it uses unchanged (mma_chunk, issue_chunk, wait_then_barrier): a workgroup is
// 8 waves, a wave owns 32 points and carries their activations in registers as B fragments, the weight stream is pulled L2 -> LDS by
// LDS-DMA into a 4-slot ring with one rendezvous per two chunks (a chunk = one 32-row output tile).  What is new is the stage list
// (NerfStream), the ReLU epilogue and the encodings as aux k-steps.  Biases ride in a constant-1 slot of an aux k-step, as in the
// Sat-NeRF stream: slot 60 of the encoded-xyz k-steps (fc_net.0, fc_net.8), slot 24 of the encoded-direction k-steps
// (rgb_from_xyzdir.0), and a k-step of their own ("ones": slot 0 = 1) behind every other stage's 16 / 8 k-steps.
#pragma once
#include "mlp_fwd.inc"

namespace sr {
inline namespace SR_FEAT_NS {

// chunk list in consumption order (mirrored by packing.nerf_forward_maps):
//   L0 (8 x 4 enc) | L1..L3 (8 x 16+1) | L4 (8 x 4 enc + 16) | L5..L7 (8 x 16+1) | feats (8 x 16+1) | sigma (1 x 16+1) |
//   rgb hidden (4 x 16 + 2 dir) | rgb (1 x 8+1)
constexpr int kEncS = 4, kDirS = 2;      // aux k-steps: 60 encoded-xyz values + 1 | 24 encoded-direction values + 1
constexpr int kEncOne = 60, kDirOne = 24;  // their constant-1 slots
constexpr int kXyzFreqs = 10, kDirFreqs = 4;
struct NerfStream {
  static constexpr int SLOTP = kEncS + kKS;  // pieces per ring slot (the skip layer's tile)
  static constexpr int NSTAGE = 12;
  static constexpr int cnt(int st) {
    constexpr int c[NSTAGE] = {kMT, kMT, kMT, kMT, kMT, kMT, kMT, kMT, kMT, 1, kMTH, 1};
    return c[st];
  }
  static constexpr int size(int st) {
    constexpr int z[NSTAGE] = {kEncS, kKS + 1, kKS + 1, kKS + 1, kEncS + kKS, kKS + 1, kKS + 1, kKS + 1, kKS + 1, kKS + 1, kKS + kDirS, kHS + 1};
    return z[st];
  }
  static constexpr int first(int st) {
    int g = 0;
    for (int k = 0; k < st; ++k) g += cnt(k);
    return g;
  }
  static constexpr int G_FEATS = 8 * kMT, G_SIGMA = G_FEATS + kMT, G_RGBH = G_SIGMA + 1, G_RGB = G_RGBH + kMTH;
  static constexpr int NCH = G_RGB + 1;
  static constexpr int np(int g) {
    if (g < 0 || g >= NCH) return 0;
    int st = 0;
    while (g >= first(st) + cnt(st)) ++st;
    return size(st);
  }
  static constexpr long offset_pieces(int g) {
    long n = 0;
    for (int c = 0; c < g; ++c) n += np(c);
    return n;
  }
  static constexpr long total_pieces() { return offset_pieces(NCH); }
};
constexpr int kNerfBatch = 1;                 // A fragments per mma_chunk batch: scheduling is left to hipcc (mlp_device.h)
constexpr int kNerfGroup = 2;                 // chunks per rendezvous
constexpr int kNerfSlots = 2 * kNerfGroup;    // ring slots
constexpr int kNerfSlotBytes = NerfStream::SLOTP * 1024;
constexpr int kNerfPoints = 8 * 32;           // points of a workgroup
static_assert(NerfStream::NCH % kNerfGroup == 0, "chunk groups must tile the stream");
static_assert(Mode<1>::NW * 32 == kNerfPoints, "issue_chunk spreads a chunk's pieces over the 8 waves this kernel launches");

struct NerfParams {
  const char* stream;
  // per-point entry: xyz (P, >=3), dirs (rows, >=3) read at row point / row_div
  const float* xyz;
  const float* dirs;
  int xyz_stride, dir_stride, row_div;
  long n_points;
  float *rgb, *sigma;  // (P,3), (P)
  // render entry: rays (N, >=8) = o d near far; depths from u (stratified) or z_in (as given)
  const float* rays;
  int ray_stride, n_samples, rays_per_block;
  long n_rays;
  const float *u, *z_in, *noise;
  float noise_std;
  float *z_out, *r_rgb, *depth, *weights, *transp;
};

enum { NACT_RELU = 0, NACT_ID = 1 };
template <int ACT>
__device__ __forceinline__ void nerf_pack(const f32x16& acc, uint4& h0, uint4& h1) {
  uint32_t w[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    float a = acc[2 * q], b = acc[2 * q + 1];
    if (ACT == NACT_RELU) a = __builtin_fmaxf(a, 0.f), b = __builtin_fmaxf(b, 0.f);
    w[q] = pack_op2(a, b);
  }
  h0 = make_uint4(w[0], w[1], w[2], w[3]);
  h1 = make_uint4(w[4], w[5], w[6], w[7]);
}

// entry protocol of chunk G: at a group start wait for the whole group's DMA, rendezvous, request the next group into the slots the
// previous group was read from (every wave's ds_reads of them have returned: lgkmcnt(0) in front of the barrier)
template <int G>
__device__ __forceinline__ void nerf_enter(char* ring, const char* stream, int wave, int lane) {
  if constexpr (G % kNerfGroup == 0) {
    wait_then_barrier<0>();
    static_for<kNerfGroup>([&](auto ic) {
      constexpr int c = G + kNerfGroup + decltype(ic)::value;
      if constexpr (c < NerfStream::NCH) {
        constexpr long off = NerfStream::offset_pieces(c) * 1024L;
        issue_chunk<1, NerfStream::np(c)>(stream, nullptr, off, ring + (c % kNerfSlots) * kNerfSlotBytes, wave, lane);
      }
    });
  }
}

// a dense stage: MT output tiles; `mma(acc, slot)` adds one tile's k-steps; tile t -> out fragments 2t, 2t+1.  Tile t's MFMAs are issued
// before tile t-1's epilogue, as in dense_stage.
template <int G0, int MT, int NP, int ACT, int NOUT, class MMA>
__device__ __forceinline__ void nerf_stage(Frags<1, NOUT>& out, char* ring, const char* stream, int wave, int lane, MMA&& mma) {
  static_assert(2 * MT <= NOUT, "output fragments");
  f32x16 acc[2];
  static_for<MT>([&](auto tc) {
    constexpr int t = decltype(tc)::value, g = G0 + t;
    static_assert(NerfStream::np(g) == NP, "stream geometry mismatch");
    nerf_enter<g>(ring, stream, wave, lane);
    acc[t & 1] = f32x16{0};
    mma(acc[t & 1], ring + (g % kNerfSlots) * kNerfSlotBytes);
    if constexpr (t > 0) nerf_pack<ACT>(acc[(t - 1) & 1], out.hi[2 * (t - 1)], out.hi[2 * (t - 1) + 1]);
  });
  nerf_pack<ACT>(acc[(MT - 1) & 1], out.hi[2 * (MT - 1)], out.hi[2 * (MT - 1) + 1]);
}

// Mapping.forward (models/nerf.py:53-69), one aux k-step: slot c = 16 a + 8 h + j holds column c of [sin(2^k v), cos(2^k v)]_k (k = c / 6,
// cos for c % 6 >= 3, channel c % 3), slot `one` holds 1, the rest 0.  fp32: the angle in revolutions is 2^k v (exact) times 1 / 2 pi as
// a two-term product (hi * arg rounded, its error and lo * arg recovered by fma), the exact fraction of the rounded product plus that
// remainder goes to the hardware sine (cos = a quarter revolution on): 1e-6 of sinf / cosf up to the 2^9 * 6 rad the frequencies reach.
template <int NFREQ>
__device__ __forceinline__ uint4 nerf_encode_step(int a, int h, float x, float y, float z, int one) {
  constexpr double inv2pi = 0.15915494309189533576888;
  constexpr float c_hi = (float)inv2pi, c_lo = (float)(inv2pi - (double)c_hi);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = 16 * a + 8 * h + j;
    const int k = c / 6, m = c - 6 * k, ch = m >= 3 ? m - 3 : m;
    const float arg = __builtin_ldexpf(ch == 0 ? x : (ch == 1 ? y : z), k);
    const float p = arg * c_hi;
    const float e = __builtin_fmaf(arg, c_lo, __builtin_fmaf(arg, c_hi, -p));
    const float rev = __builtin_amdgcn_fractf(p) + e + (m >= 3 ? 0.25f : 0.f);
    const float s = sin_rev_fast(rev);
    v[j] = c < 6 * NFREQ ? s : (c == one ? 1.f : 0.f);
  }
  return make_uint4(pack_op2(v[0], v[1]), pack_op2(v[2], v[3]), pack_op2(v[4], v[5]), pack_op2(v[6], v[7]));
}

struct NerfIndex {
  bool valid;  // the lane's point exists
  long pt;     // its index (clamped to an existing point for tail lanes)
  long row;    // REND: its ray; else: its row of `dirs`
  int j;       // REND: its sample along the ray
};
template <bool REND>
__device__ __forceinline__ NerfIndex nerf_index(const NerfParams& prm, int q) {
  NerfIndex ix;
  if constexpr (REND) {
    const int S = prm.n_samples;
    const int lr = q / S;
    const long ray = (long)blockIdx.x * prm.rays_per_block + lr;
    ix.valid = lr < prm.rays_per_block && ray < prm.n_rays;
    ix.row = ix.valid ? ray : prm.n_rays - 1;
    ix.j = ix.valid ? q - lr * S : 0;
    ix.pt = ix.row * S + ix.j;
  } else {
    const long pt = (long)blockIdx.x * kNerfPoints + q;
    ix.valid = pt < prm.n_points;
    ix.pt = ix.valid ? pt : prm.n_points - 1;
    ix.row = ix.pt / prm.row_div;
    ix.j = 0;
  }
  return ix;
}

template <bool REND>
__global__ void __launch_bounds__(512) nerf_fwd_kernel(const NerfParams prm) {
  using NS = NerfStream;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem;
  float* r_z = reinterpret_cast<float*>(smem + kNerfSlots * kNerfSlotBytes);  // REND: the workgroup's per-point values = whole rays
  float *r_sigma = r_z + kNerfPoints, *r_col = r_z + 2 * kNerfPoints;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, pl = lane & 31;
  const char* stream = prm.stream;

  // start the weight stream
#pragma unroll
  for (int g = 0; g < kNerfGroup; ++g) issue_chunk<1, NS::np(0)>(stream, nullptr, (long)g * NS::np(0) * 1024, ring + g * kNerfSlotBytes, wave, lane);

  // this lane's sample point (tail lanes compute a valid point again and store nothing)
  const int q = wave * 32 + pl;  // point of the workgroup
  float x, y, zc;
  {
    const NerfIndex ix = nerf_index<REND>(prm, q);
    if constexpr (REND) {
#pragma clang fp contract(off)  // rendering.py:81 is an unfused mul then add
      const float* rr = prm.rays + ix.row * prm.ray_stride;
      const float zz = prm.z_in ? prm.z_in[ix.pt] : stratified_z(rr[6], rr[7], ix.j, prm.n_samples, prm.u[ix.pt]);
      if (h == 0) {
        r_z[q] = zz;
        if (ix.valid && prm.z_out) prm.z_out[ix.pt] = zz;
      }
      const float mx = rr[3] * zz, my = rr[4] * zz, mz = rr[5] * zz;
      x = rr[0] + mx, y = rr[1] + my, zc = rr[2] + mz;
    } else {
      const float* xp = prm.xyz + ix.pt * prm.xyz_stride;
      x = xp[0], y = xp[1], zc = xp[2];
    }
  }

  Frags<1, kEncS> enc;  // live until the skip layer
#pragma unroll
  for (int a = 0; a < kEncS; ++a) enc.hi[a] = nerf_encode_step<kXyzFreqs>(a, h, x, y, zc, kEncOne);
  Frags<1, 1> ones;
  ones.hi[0] = make_uint4(h == 0 ? pack_op2(1.f, 0.f) : 0u, 0u, 0u, 0u);

  Frags<1, kKS> cur, nxt;
  // ---- fc_net.0: encoded xyz (+ bias) -> 256, ReLU ----------------------------------------------------------------------------
  nerf_stage<0, kMT, kEncS, NACT_RELU>(cur, ring, stream, wave, lane,
                                       [&](f32x16& acc, const char* slot) { mma_chunk<1, kEncS, 0, kEncS, 1, kNerfBatch>(acc, slot, enc, ones, lane); });
  // ---- fc_net.2 .. fc_net.14 -----------------------------------------------------------------------------------------------------
  static_for<7>([&](auto lc) {
    constexpr int l = decltype(lc)::value + 1;
    if constexpr (l == 4) {  // torch.cat([e, h]) (models/nerf.py:204): the encoded columns first
      nerf_stage<NS::first(l), kMT, kEncS + kKS, NACT_RELU>(nxt, ring, stream, wave, lane, [&](f32x16& acc, const char* slot) {
        mma_chunk<1, kEncS, 0, kEncS, 1, kNerfBatch>(acc, slot, enc, ones, lane);
        mma_chunk<1, kKS, 0, kKS, 1, kNerfBatch>(acc, slot + kEncS * 1024, cur, ones, lane);
      });
    } else {
      nerf_stage<NS::first(l), kMT, kKS + 1, NACT_RELU>(nxt, ring, stream, wave, lane,
                                                        [&](f32x16& acc, const char* slot) { mma_chunk<1, kKS + 1, 0, kKS, 1, kNerfBatch>(acc, slot, cur, ones, lane); });
    }
    cur = nxt;
  });
  // ---- feats = feats_from_xyz(h) (identity), sigma = softplus(sigma_from_xyz(h)) ------------------------------------------------
  Frags<1, kKS> feats;
  nerf_stage<NS::G_FEATS, kMT, kKS + 1, NACT_ID>(feats, ring, stream, wave, lane,
                                                 [&](f32x16& acc, const char* slot) { mma_chunk<1, kKS + 1, 0, kKS, 1, kNerfBatch>(acc, slot, cur, ones, lane); });
  float sg;
  {
    constexpr int g = NS::G_SIGMA;
    static_assert(NS::np(g) == kKS + 1, "stream geometry mismatch");
    nerf_enter<g>(ring, stream, wave, lane);
    f32x16 acc = {0};
    mma_chunk<1, kKS + 1, 0, kKS, 1, kNerfBatch>(acc, ring + (g % kNerfSlots) * kNerfSlotBytes, cur, ones, lane);
    sg = softplus_f(acc[0]);  // row 0 of the tile (lane half 0)
  }
  // ---- colour head: rgb_from_xyzdir.0 on [feats | map(dir)] (ReLU), rgb_from_xyzdir.2 (sigmoid, padded) ----------------------------
  // (the point's indices are worked out again here and at the end from a laundered copy of q: held through the trunk, the direction
  //  and the output index cost the registers that make the difference between 256 VGPRs and scratch)
  Frags<1, kDirS> dirf;
  {
    int q2 = q;
    asm volatile("" : "+v"(q2));
    const NerfIndex ix = nerf_index<REND>(prm, q2);
    const float* dp = REND ? prm.rays + ix.row * prm.ray_stride + 3 : prm.dirs + ix.row * prm.dir_stride;
    const float dx = dp[0], dy = dp[1], dz = dp[2];
#pragma unroll
    for (int a = 0; a < kDirS; ++a) dirf.hi[a] = nerf_encode_step<kDirFreqs>(a, h, dx, dy, dz, kDirOne);
  }
  Frags<1, kHS> rgbh;
  nerf_stage<NS::G_RGBH, kMTH, kKS + kDirS, NACT_RELU>(rgbh, ring, stream, wave, lane, [&](f32x16& acc, const char* slot) {
    mma_chunk<1, kKS + kDirS, 0, kKS, kDirS, kNerfBatch>(acc, slot, feats, dirf, lane);
  });
  float c0, c1, c2;
  {
    constexpr int g = NS::G_RGB;
    static_assert(NS::np(g) == kHS + 1, "stream geometry mismatch");
    nerf_enter<g>(ring, stream, wave, lane);
    f32x16 acc = {0};
    mma_chunk<1, kHS + 1, 0, kHS, 1, kNerfBatch>(acc, ring + (g % kNerfSlots) * kNerfSlotBytes, rgbh, ones, lane);
    c0 = sigmoid_f(acc[0]) * 1.002f - 0.001f;  // models/nerf.py:225, rgb_padding = 0.001
    c1 = sigmoid_f(acc[1]) * 1.002f - 0.001f;
    c2 = sigmoid_f(acc[2]) * 1.002f - 0.001f;
  }

  if constexpr (REND) {
    // per-point values -> LDS; wave w composites rays w, w + 8, ... of the workgroup with the stand-alone kernel's own function
    if (h == 0) {
      r_sigma[q] = sg;
      r_col[q * 3] = c0, r_col[q * 3 + 1] = c1, r_col[q * 3 + 2] = c2;
    }
    __syncthreads();
    const int S = prm.n_samples;
    for (int lr = wave; lr < prm.rays_per_block; lr += 8) {
      const long ray = (long)blockIdx.x * prm.rays_per_block + lr;
      if (ray >= prm.n_rays) break;
      composite_ray(r_z + lr * S, r_sigma + lr * S, prm.noise ? prm.noise + ray * S : nullptr, prm.noise_std, r_col + lr * S * 3, nullptr, 0.f, 0.f,
                    0.f, S, lane, 0, prm.weights + ray * S, prm.transp + ray * S, prm.depth ? prm.depth + ray : nullptr,
                    prm.r_rgb ? prm.r_rgb + ray * 3 : nullptr);
    }
  } else {
    int q2 = q;
    asm volatile("" : "+v"(q2));
    const NerfIndex ix = nerf_index<REND>(prm, q2);
    if (ix.valid && h == 0) {
      prm.sigma[ix.pt] = sg;
      float* o = prm.rgb + ix.pt * 3;
      o[0] = c0, o[1] = c1, o[2] = c2;
    }
  }
}

template <bool REND>
int nerf_launch(const NerfParams& p, hipStream_t st) {
  const size_t lds = (size_t)kNerfSlots * kNerfSlotBytes + (REND ? kNerfPoints * 5 * sizeof(float) : 0);
  const long blocks = REND ? (p.n_rays + p.rays_per_block - 1) / p.rays_per_block : (p.n_points + kNerfPoints - 1) / kNerfPoints;
  if (blocks > 0x7fffffffl) {
    set_error("nerf_fwd_kernel: %ld workgroups exceed the grid limit", blocks);
    return 1;
  }
  auto kern = nerf_fwd_kernel<REND>;
  if (!ensure_dynamic_lds((const void*)kern, lds)) return 1;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(512), lds, st, p);
  return check_launch("nerf_fwd_kernel");
}

}  // inline namespace SR_FEAT_NS
}  // namespace sr
