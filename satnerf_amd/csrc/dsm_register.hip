// DSM registration for gfx950: the reference's dsmr.compute_shift / dsmr.apply_shift (dsmr.py:6-148,
// 163-215), the integer XY + Z registration behind every DSM MAE the reference prints (sat_utils.py:172-177).
//
// A coarse-to-fine NCC search: while min(H_u, W_u) > 100 both images are halved (downsample2x_), the coarsest level scans
// (0, 0) +- irange, and each finer level scans twice the coarser winner +- irange.  Every statistic is fp64 over exact widenings of
// the input (numba types all of mean_std's accumulators fp64), in mean_std's two-pass form.  The whole search is enqueued on one
// stream with the running shift in device memory: no host round trip, capturable into a graph.  Partial sums are combined in a fixed
// order whose split depends only on the image shapes, so results are bitwise repeatable on any device.
#include <math.h>

#include "common.h"

// The downsample and apply arithmetic must round as the reference's does, operation for operation: no fused multiply-adds.
#pragma clang fp contract(off)

namespace sr {
namespace reg {

constexpr int kMaxRange = 16;
constexpr int kMaxSide = 16384;
constexpr int kTH = 4, kTW = 64;                           // u tile of one statistics step
constexpr int kMaxPitch = kTW + 2 * kMaxRange + 31;        // v halo row pitch (see halo_pitch)
constexpr int kMaxPartials = 4096;                         // workgroups (= partial slots) of a statistics launch
constexpr int kMaxShifts = (2 * kMaxRange + 1) * (2 * kMaxRange + 1);
constexpr int kMaxPerThread = (kMaxShifts + 255) / 256;    // shifts one thread of a 256-thread workgroup owns
constexpr int kStat = 8;                                   // per shift: count, mu_u, mu_v, sig_u, sig_v, xcorr, ncc, unused

__device__ __forceinline__ double nan64() { return __builtin_nan(""); }

// Row pitch (doubles) of the v halo in LDS: >= kTW + 2r and = 2r + 1 modulo 32, so the lanes of a half-wave, which hold
// consecutive shift indices s = oy (2r + 1) + ox, read 32 distinct ds_read_b64 bank pairs.
__host__ __device__ inline int halo_pitch(int r) {
  const int n = 2 * r + 1, lo = kTW + 2 * r;
  return lo + (((n - lo) % 32) + 32) % 32;
}

// ---- downsample2x_ (dsmr.py:17-39) ---------------------------------------------------------------------------------------------
// out (ceil(h/2), ceil(w/2)).  The reference writes out[j // 2, i // 2] for every (j, i), so the last write wins: cell (J, I) is the
// window whose top-left pixel is (min(2J + 1, h - 1), min(2I + 1, w - 1)).  Finite in-bounds values are summed in the order (j, i),
// (j + 1, i), (j, i + 1), (j + 1, i + 1) and divided by their count; NaN when there is none.  blockIdx.z picks one of two images.
__global__ void __launch_bounds__(256) downsample_kernel(const double* __restrict__ in0, int h0, int w0, double* __restrict__ out0,
                                                         const double* __restrict__ in1, int h1, int w1, double* __restrict__ out1) {
  const double* in = blockIdx.z ? in1 : in0;
  double* out = blockIdx.z ? out1 : out0;
  const int h = blockIdx.z ? h1 : h0, w = blockIdx.z ? w1 : w0;
  const int ho = (h + 1) / 2, wo = (w + 1) / 2;
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c >= (long)ho * wo) return;
  const int J = (int)(c / wo), I = (int)(c % wo);
  const int j = min(2 * J + 1, h - 1), i = min(2 * I + 1, w - 1);
  double s = 0.0;
  int n = 0;
  for (int k = 0; k < 2; ++k) {
    for (int l = 0; l < 2; ++l) {
      const int y = j + l, x = i + k;
      if (y < h && x < w) {
        const double t = in[(long)y * w + x];
        if (isfinite(t)) s = s + t, ++n;  // from 0.0, as the reference's integer 0: a lone -0.0 sums to +0.0
      }
    }
  }
  out[c] = n ? s / n : nan64();
}

// ---- mean_std (dsmr.py:50-88) at every shift of one level -------------------------------------------------------------------------
// Shift s = oy (2r + 1) + ox pairs u[j, i] with v[j + sy - r + oy, i + sx - r + ox], (sx, sy) = the level's start (read from
// `start`, or (0, 0) when it is null).  The workgroup owns u tiles b, b + P, b + 2P, ... (P = gridDim.x; kTH x kTW each), stages each
// tile with its +- r halo of v in LDS (NaN outside either image), and each thread accumulates the shifts s = tid + k blockDim.x over
// those tiles: within a tile in row-major order, even and odd columns in separate sums added at the tile's end.  PASS 1 sums {count, u, v} over pairs where both are finite; PASS 2 sums
// {du^2, dv^2, du dv} with du = u - mu_u, dv = v - mu_v over pairs where du and dv are finite (the reference's test).  One partial per
// (shift, quantity, workgroup) goes to part[(3 s + q) P + b].
template <int PASS>
__global__ void __launch_bounds__(256) stats_kernel(const double* __restrict__ u, int hu, int wu, const double* __restrict__ v, int hv, int wv,
                                                    int r, const int* __restrict__ start, int tiles_x, int ntiles, double* __restrict__ part,
                                                    const double* __restrict__ stats) {
  __shared__ double us[kTH * kTW];
  __shared__ double vs[(kTH + 2 * kMaxRange) * kMaxPitch];
  const int n = 2 * r + 1, S = n * n, pitch = halo_pitch(r);
  const int sx = start ? start[0] : 0, sy = start ? start[1] : 0;
  const int P = gridDim.x, nt = blockDim.x, tid = threadIdx.x;
  double acc[kMaxPerThread][3], mu[kMaxPerThread][2];
#pragma unroll
  for (int k = 0; k < kMaxPerThread; ++k) {
    acc[k][0] = acc[k][1] = acc[k][2] = 0.0;
    mu[k][0] = mu[k][1] = 0.0;
    const int s = tid + k * nt;
    if (PASS == 2 && s < S) mu[k][0] = stats[s * kStat + 1], mu[k][1] = stats[s * kStat + 2];
  }
  for (int t = blockIdx.x; t < ntiles; t += P) {
    const int y0 = (t / tiles_x) * kTH, x0 = (t % tiles_x) * kTW;
    for (int e = tid; e < kTH * kTW; e += nt) {
      const int y = y0 + e / kTW, x = x0 + e % kTW;
      us[e] = (y < hu && x < wu) ? u[(long)y * wu + x] : nan64();
    }
    const int hh = kTH + 2 * r, hw = kTW + 2 * r;
    const int vy0 = y0 + sy - r, vx0 = x0 + sx - r;
    for (int e = tid; e < hh * hw; e += nt) {
      const int a = e / hw, b = e % hw;
      const long y = (long)vy0 + a, x = (long)vx0 + b;
      vs[a * pitch + b] = (y >= 0 && y < hv && x >= 0 && x < wv) ? v[y * wv + x] : nan64();
    }
    __syncthreads();
    const int jn = min(kTH, hu - y0), in = min(kTW, wu - x0);  // pixels past u's edge are NaN: skipping them changes nothing
#pragma unroll
    for (int k = 0; k < kMaxPerThread; ++k) {
      const int s = tid + k * nt;
      if (s >= S) break;
      const double* vb = vs + (s / n) * pitch + (s % n);
      // two chains, even and odd columns, for instruction-level parallelism; joined once per tile (a fixed order)
      double c[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
      const double m0 = mu[k][0], m1 = mu[k][1];
      for (int j = 0; j < jn; ++j) {
#pragma unroll 4
        for (int i = 0; i < in; ++i) {
          const double a = us[j * kTW + i], b = vb[j * pitch + i];
          double* e = c[i & 1];
          if (PASS == 1) {
            if (isfinite(a) && isfinite(b)) e[0] += 1.0, e[1] += a, e[2] += b;
          } else {
            const double du = a - m0, dv = b - m1;
            if (isfinite(du) && isfinite(dv)) e[0] += du * du, e[1] += dv * dv, e[2] += du * dv;
          }
        }
      }
      for (int q = 0; q < 3; ++q) acc[k][q] += c[0][q] + c[1][q];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kMaxPerThread; ++k) {
    const int s = tid + k * nt;
    if (s < S)
      for (int q = 0; q < 3; ++q) part[(long)(3 * s + q) * P + blockIdx.x] = acc[k][q];
  }
}

// One workgroup per shift: the P partials of each quantity summed in a fixed order (thread t takes t, t + 256, ..., then a fixed LDS
// tree), then PASS 1 stores count, mu_u = sum u / count, mu_v = sum v / count (NaN when count = 0); PASS 2 stores sig_u =
// sqrt(sum du^2 / count), sig_v, xcorr = sum du dv / count and ncc = xcorr / (sig_u sig_v), NaN where the reference would raise
// ZeroDivisionError (count = 0 or sig_u sig_v = 0).
template <int PASS>
__global__ void __launch_bounds__(256) reduce_kernel(const double* __restrict__ part, int P, double* __restrict__ stats) {
  __shared__ double red[3][256];
  const int s = blockIdx.x, tid = threadIdx.x;
  for (int q = 0; q < 3; ++q) {
    const double* p = part + (long)(3 * s + q) * P;
    double a = 0.0;
    for (int w = tid; w < P; w += 256) a += p[w];
    red[q][tid] = a;
  }
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h)
      for (int q = 0; q < 3; ++q) red[q][tid] += red[q][tid + h];
    __syncthreads();
  }
  if (tid) return;
  double* st = stats + s * kStat;
  if (PASS == 1) {
    const double count = red[0][0];
    st[0] = count;
    st[1] = count > 0 ? red[1][0] / count : nan64();
    st[2] = count > 0 ? red[2][0] / count : nan64();
  } else {
    const double count = st[0];
    const double su = sqrt(red[0][0] / count), sv = sqrt(red[1][0] / count), xc = red[2][0] / count;
    st[3] = su, st[4] = sv, st[5] = xc;
    const double den = su * sv;
    st[6] = (count > 0 && den != 0) ? xc / den : nan64();
  }
}

// compute_ncc's choice (dsmr.py:102-118) among one level's shifts: scanning y outer, x inner, the first strict maximum, i.e. the
// largest NCC with the smallest index among equals; NaN is never chosen, and a level without a finite NCC keeps its start.  Writes
// the level's NCC map and start to the optional outputs; then the next level's start (2 x the winner, recursive_ncc's doubling)
// into `cur`, or at level 0 the final shift and compute_shift's coefficients (dsmr.py:184-188), taken from the level-0 statistics
// of the winner -- mean_std at that shift, which is what compute_shift recomputes.  One wave.
__global__ void __launch_bounds__(64) select_kernel(const double* __restrict__ stats, int r, int level, const int* start, int* cur,
                                                    int scaling, double* __restrict__ ncc_out, int* __restrict__ start_out,
                                                    int* __restrict__ shift, double* __restrict__ coef) {
  const int n = 2 * r + 1, S = n * n, lane = threadIdx.x;
  const int sx = start ? start[0] : 0, sy = start ? start[1] : 0;
  double best = -INFINITY;
  int bi = S / 2;  // the start itself: the centre of the map
  bool any = false;
  for (int s = lane; s < S; s += 64) {
    const double c = stats[s * kStat + 6];
    if (ncc_out) ncc_out[(long)level * S + s] = c;
    if (c > best) best = c, bi = s, any = true;  // first strict maximum of this lane's subsequence
  }
  for (int off = 32; off >= 1; off >>= 1) {
    const double ob = __shfl_xor(best, off);
    const int oi = __shfl_xor(bi, off);
    const bool oa = __shfl_xor((int)any, off) != 0;
    if (oa && (!any || ob > best || (ob == best && oi < bi))) best = ob, bi = oi, any = true;
  }
  if (lane) return;
  if (start_out) start_out[2 * level] = sx, start_out[2 * level + 1] = sy;
  const int dx = sx - r + bi % n, dy = sy - r + bi / n;
  if (level > 0) {
    cur[0] = 2 * dx, cur[1] = 2 * dy;
    return;
  }
  const double* st = stats + bi * kStat;
  const double a = scaling ? st[3] / st[4] : 1.0;
  shift[0] = dx, shift[1] = dy;
  coef[0] = a, coef[1] = st[1] - st[2] * a;
  for (int q = 1; q < 6; ++q) coef[q + 1] = st[q];  // mu_u, mu_v, sig_u, sig_v, xcorr
  coef[7] = st[0];                                  // count (0: compute_shift has no defined answer)
}

// apply_shift_ (dsmr.py:138-148) over v's extent: out[j, i] = a v[j + dy, i + dx] + b in fp64 (NaN outside v), rounded to fp32.  The
// reference's trailing "+ c i + d j" adds an integer 0 (its c is the channel index, d is 0 at every call site): that + 0.0 is kept,
// since it turns a -0.0 into +0.0.
__global__ void __launch_bounds__(256) apply_kernel(const double* __restrict__ v, int hv, int wv, const int* __restrict__ shift,
                                                    const double* __restrict__ coef, float* __restrict__ out) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c >= (long)hv * wv) return;
  const int j = (int)(c / wv), i = (int)(c % wv);
  const long y = (long)j + shift[1], x = (long)i + shift[0];
  const double t = (y >= 0 && y < hv && x >= 0 && x < wv) ? v[y * wv + x] : nan64();
  const double a = coef[0], b = coef[1];
  out[c] = (float)(a * t + b + 0.0);
}

// ---- the plan: level shapes and scratch layout, a function of the shapes and irange alone ----------------------------------------
struct Plan {
  int levels;
  int hu[16], wu[16], hv[16], wv[16];
  double* img[16][2];  // level k's u / v (k >= 1)
  double *part, *stats;
  int* cur;       // 2 ints
  int64_t bytes;  // whole doubles
  int S;
};

inline int tiles_of(int h, int w) { return ((h + kTH - 1) / kTH) * ((w + kTW - 1) / kTW); }
inline int partials_of(int h, int w) { return (int)partial_slots(tiles_of(h, w), 1, kMaxPartials); }

// base == nullptr: sizes only
inline Plan make_plan(void* base, int hu, int wu, int hv, int wv, int r) {
  Plan p{};
  ScratchCarver c(base);
  p.hu[0] = hu, p.wu[0] = wu, p.hv[0] = hv, p.wv[0] = wv;
  p.levels = 1;
  while ((p.hu[p.levels - 1] < p.wu[p.levels - 1] ? p.hu[p.levels - 1] : p.wu[p.levels - 1]) > 100) {
    const int k = p.levels++;
    p.hu[k] = (p.hu[k - 1] + 1) / 2, p.wu[k] = (p.wu[k - 1] + 1) / 2;
    p.hv[k] = (p.hv[k - 1] + 1) / 2, p.wv[k] = (p.wv[k - 1] + 1) / 2;
    p.img[k][0] = c.take<double>((int64_t)p.hu[k] * p.wu[k], 8);
    p.img[k][1] = c.take<double>((int64_t)p.hv[k] * p.wv[k], 8);
  }
  p.S = (2 * r + 1) * (2 * r + 1);
  p.part = c.take<double>(3L * p.S * partials_of(hu, wu), 8);  // level 0 has the most tiles
  p.stats = c.take<double>((int64_t)kStat * p.S, 8);
  p.cur = c.take<int>(2, 8);
  p.bytes = c.bytes();
  return p;
}

}  // namespace reg
}  // namespace sr

using namespace sr;
using namespace sr::reg;

static int check_shape(const char* fn, int hu, int wu, int hv, int wv, int irange) {
  SR_REQUIRE(hu >= 1 && wu >= 1 && hv >= 1 && wv >= 1 && hu <= kMaxSide && wu <= kMaxSide && hv <= kMaxSide && wv <= kMaxSide,
             "%s: each side must be in 1..%d (u %d x %d, v %d x %d)", fn, kMaxSide, hu, wu, hv, wv);
  SR_REQUIRE(irange >= 1 && irange <= kMaxRange, "%s: irange must be in 1..%d (got %d)", fn, kMaxRange, irange);
  return 0;
}

extern "C" int sr_dsm_register_scratch(int hu, int wu, int hv, int wv, int irange, int64_t* bytes, int* levels) {
  SR_REQUIRE(bytes && levels, "sr_dsm_register_scratch: null pointer");
  if (check_shape("sr_dsm_register_scratch", hu, wu, hv, wv, irange)) return 1;
  const Plan p = make_plan(nullptr, hu, wu, hv, wv, irange);
  *bytes = p.bytes;
  *levels = p.levels;
  return 0;
}

extern "C" int sr_dsm_downsample2x(const double* in, int h, int w, double* out, void* stream) {
  SR_REQUIRE(in && out, "sr_dsm_downsample2x: null pointer");
  SR_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "sr_dsm_downsample2x: each side must be in 1..%d (%d x %d)", kMaxSide, h, w);
  const long cells = (long)((h + 1) / 2) * ((w + 1) / 2);
  hipLaunchKernelGGL(downsample_kernel, dim3(blocks_for(cells), 1, 1), dim3(256), 0, (hipStream_t)stream, in, h, w, out, in, h, w, out);
  return check_launch("downsample_kernel");
}

extern "C" int sr_dsm_compute_shift(const double* u, int hu, int wu, const double* v, int hv, int wv, int irange, int scaling,
                                    void* scratch, int64_t scratch_bytes, int* shift, double* coef, double* ncc_levels, int* start_levels,
                                    void* stream) {
  SR_REQUIRE(u && v && scratch && shift && coef, "sr_dsm_compute_shift: null pointer");
  if (check_shape("sr_dsm_compute_shift", hu, wu, hv, wv, irange)) return 1;
  const Plan p = make_plan(scratch, hu, wu, hv, wv, irange);
  if (require_scratch("sr_dsm_compute_shift", scratch_bytes, p.bytes)) return 1;
  hipStream_t s = (hipStream_t)stream;
  const double* lu[16];
  const double* lv[16];
  lu[0] = u, lv[0] = v;
  for (int k = 1; k < p.levels; ++k) {
    const long cells = (long)p.hu[k] * p.wu[k] > (long)p.hv[k] * p.wv[k] ? (long)p.hu[k] * p.wu[k] : (long)p.hv[k] * p.wv[k];
    hipLaunchKernelGGL(downsample_kernel, dim3(blocks_for(cells), 1, 2), dim3(256), 0, s, lu[k - 1], p.hu[k - 1], p.wu[k - 1], p.img[k][0],
                       lv[k - 1], p.hv[k - 1], p.wv[k - 1], p.img[k][1]);
    if (check_launch("downsample_kernel")) return 2;
    lu[k] = p.img[k][0], lv[k] = p.img[k][1];
  }
  const unsigned nt = (unsigned)((p.S + 63) / 64 * 64 < 256 ? (p.S + 63) / 64 * 64 : 256);
  for (int k = p.levels - 1; k >= 0; --k) {
    const int tiles_x = (p.wu[k] + kTW - 1) / kTW, ntiles = tiles_of(p.hu[k], p.wu[k]), P = partials_of(p.hu[k], p.wu[k]);
    const int* start = k == p.levels - 1 ? nullptr : p.cur;
    hipLaunchKernelGGL(stats_kernel<1>, dim3(P), dim3(nt), 0, s, lu[k], p.hu[k], p.wu[k], lv[k], p.hv[k], p.wv[k], irange, start, tiles_x,
                       ntiles, p.part, (const double*)p.stats);
    if (check_launch("stats_kernel<1>")) return 2;
    hipLaunchKernelGGL(reduce_kernel<1>, dim3(p.S), dim3(256), 0, s, (const double*)p.part, P, p.stats);
    if (check_launch("reduce_kernel<1>")) return 2;
    hipLaunchKernelGGL(stats_kernel<2>, dim3(P), dim3(nt), 0, s, lu[k], p.hu[k], p.wu[k], lv[k], p.hv[k], p.wv[k], irange, start, tiles_x,
                       ntiles, p.part, (const double*)p.stats);
    if (check_launch("stats_kernel<2>")) return 2;
    hipLaunchKernelGGL(reduce_kernel<2>, dim3(p.S), dim3(256), 0, s, (const double*)p.part, P, p.stats);
    if (check_launch("reduce_kernel<2>")) return 2;
    hipLaunchKernelGGL(select_kernel, dim3(1), dim3(64), 0, s, (const double*)p.stats, irange, k, start, p.cur, scaling, ncc_levels, start_levels,
                       shift, coef);
    if (check_launch("select_kernel")) return 2;
  }
  return 0;
}

extern "C" int sr_dsm_apply_shift(const double* v, int hv, int wv, const int* shift, const double* coef, float* out, void* stream) {
  SR_REQUIRE(v && shift && coef && out, "sr_dsm_apply_shift: null pointer");
  SR_REQUIRE(hv >= 1 && wv >= 1 && hv <= kMaxSide && wv <= kMaxSide, "sr_dsm_apply_shift: each side must be in 1..%d (%d x %d)", kMaxSide,
             hv, wv);
  hipLaunchKernelGGL(apply_kernel, dim3(blocks_for((long)hv * wv)), dim3(256), 0, (hipStream_t)stream, v, hv, wv, shift, coef, out);
  return check_launch("apply_kernel");
}
