// Point clouds -> one DSM by a per-cell min / max / mean / median: eval_s2p.project_cloud_into_utm_grid
// (eval_s2p.py:175-226) for gfx950.  Five stages on one stream, no host round trip: cell key + histogram, exclusive scan, scatter into
// per-cell segments, segmented sort on an order-preserving 64-bit key, reduce.  Every mode reads the sorted segment, and only 32-bit
// integer atomics are used, so the raster is bitwise independent of point and arrival order.  Do not build this file with fast-math:
// the cell index is IEEE fp64 division + round-half-even and must equal numpy's.
#include <math.h>

#include "block_device.h"
#include "common.h"

namespace sr {
namespace cg {

constexpr int kScanBlock = 1024;  // cells per workgroup of the scan (256 threads x 4)
constexpr int kWaveCap = 64;      // segments up to this length are sorted by one wave in registers
constexpr int kChunk = 4096;      // longer ones by one workgroup: in LDS up to this length (32 KiB), beyond it in chunks of this length
constexpr unsigned long long kInf = ~0ull;  // pads a segment to a power of two: above every finite key

enum { kRuleNearest = 0, kRuleFloor = 1 };
enum { kMin = 0, kMax = 1, kAvg = 2, kMed = 3 };

// ---- stage 1: key[i] = output cell of point i (-1 when dropped), count[cell] += 1 ----------------------------------------------------
// nearest: col = rint((e - x0) / d), row = rint((n - y0) / d), output row map_h - 1 - row (the reference's flipud).  -0 counts as 0.
// floor:   col = floor((e - x0) / d), row = floor((y0 - n) / d) (sr_dsm_rasterize's cell), output row = row.
__global__ void __launch_bounds__(256) key_count_kernel(const double* __restrict__ east, const double* __restrict__ north,
                                                        const double* __restrict__ alt, int n, double x0, double y0, double d, int map_w,
                                                        int map_h, int rule, int* __restrict__ key, int* __restrict__ count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double e = east[i], nn = north[i];
  int cell = -1;
  if (isfinite(e) && isfinite(nn) && isfinite(alt[i])) {
    double c, r;
    if (rule == kRuleNearest) {
      c = rint((e - x0) / d), r = rint((nn - y0) / d);
    } else {
      c = floor((e - x0) / d), r = floor((y0 - nn) / d);
    }
    if (c >= 0 && c < map_w && r >= 0 && r < map_h) {
      const int row = rule == kRuleNearest ? map_h - 1 - (int)r : (int)r;
      cell = row * map_w + (int)c;
    }
  }
  key[i] = cell;
  if (cell >= 0) atomicAdd(count + cell, 1);
}

// ---- stage 2: exclusive scan of count, three launches -----------------------------------------------------------------------------------
__device__ __forceinline__ int wave_inclusive(int v) {
  const int lane = threadIdx.x & 63;
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(v, off);
    if (lane >= off) v += o;
  }
  return v;
}
// exclusive prefix of v over the 256 threads of a workgroup (red: 4 ints of LDS), and the workgroup's total
__device__ __forceinline__ int block_exclusive(int v, int* red, int& total) {
  const int inc = wave_inclusive(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();  // red may still be read from a previous call
  if ((threadIdx.x & 63) == 63) red[w] = inc;
  __syncthreads();
  int base = 0;
  for (int k = 0; k < 4; ++k) base += k < w ? red[k] : 0;
  total = red[0] + red[1] + red[2] + red[3];
  return base + inc - v;
}

__global__ void __launch_bounds__(256) scan_sums_kernel(const int* __restrict__ count, int cells, int* __restrict__ bsum) {
  __shared__ int red[4];
  const int base = blockIdx.x * kScanBlock + threadIdx.x * 4;
  int s = 0;
  for (int k = 0; k < 4; ++k) s += base + k < cells ? count[base + k] : 0;
  int total;
  block_exclusive(s, red, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: bsum -> its exclusive scan in place, 256 entries at a time with a running carry; also zeroes the long-segment counter
__global__ void __launch_bounds__(256) scan_carry_kernel(int* __restrict__ bsum, int nb, int* __restrict__ n_long) {
  __shared__ int red[4];
  if (threadIdx.x == 0) *n_long = 0;
  int carry = 0;
  for (int b0 = 0; b0 < nb; b0 += 256) {
    const int i = b0 + threadIdx.x;
    const int v = i < nb ? bsum[i] : 0;
    int total;
    const int ex = block_exclusive(v, red, total);
    if (i < nb) bsum[i] = carry + ex;
    carry += total;
  }
}

__global__ void __launch_bounds__(256) scan_add_kernel(const int* __restrict__ count, int cells, const int* __restrict__ bsum,
                                                       int* __restrict__ offs, int* __restrict__ cursor) {
  __shared__ int red[4];
  const int base = blockIdx.x * kScanBlock + threadIdx.x * 4;
  int c[4], s = 0;
  for (int k = 0; k < 4; ++k) c[k] = base + k < cells ? count[base + k] : 0, s += c[k];
  int total;
  int o = bsum[blockIdx.x] + block_exclusive(s, red, total);
  for (int k = 0; k < 4; ++k) {
    if (base + k < cells) offs[base + k] = o, cursor[base + k] = o;
    o += c[k];
  }
}

// ---- stage 3: scatter each kept altitude's key into its cell's segment -------------------------------------------------------------------
__global__ void __launch_bounds__(256) scatter_kernel(const double* __restrict__ alt, int n, const int* __restrict__ key,
                                                      int* __restrict__ cursor, unsigned long long* __restrict__ vals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int cell = key[i];
  if (cell < 0) return;
  vals[atomicAdd(cursor + cell, 1)] = order_key(alt[i]);
}

// ---- stage 4: sort every segment in place ------------------------------------------------------------------------------------------------
// One network everywhere: for k = 2, 4, .. P (P = the power of two >= the length): a flip (i against i ^ (k - 1)), then half-cleaners of
// stride k/4 .. 1 (i against i ^ s); every comparator leaves the smaller key at the lower index.  Indices >= the length stand for
// kInf, which such comparators never move, so a pair whose upper index is outside the segment is skipped.  Trip counts depend on the
// length alone.

// one wave per cell: lengths 2 .. kWaveCap in registers; longer segments are appended to `longs` for sort_long_kernel
__global__ void __launch_bounds__(256) sort_wave_kernel(const int* __restrict__ count, const int* __restrict__ offs, int cells,
                                                        unsigned long long* __restrict__ vals, int* __restrict__ n_long,
                                                        int* __restrict__ longs) {
  const int cell = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (cell >= cells) return;
  const int n = count[cell];
  if (n < 2) return;
  if (n > kWaveCap) {
    if (lane == 0) longs[atomicAdd(n_long, 1)] = cell;
    return;
  }
  unsigned long long* seg = vals + offs[cell];
  unsigned long long v = lane < n ? seg[lane] : kInf;
  for (int k = 2; (k >> 1) < n; k <<= 1) {
    for (int s = k; s >= 2; s >>= 1) {
      const int partner = lane ^ (s == k ? k - 1 : (s >> 1));
      const unsigned long long o = __shfl(v, partner);
      v = (lane < partner) == (v < o) ? v : o;
    }
  }
  if (lane < n) seg[lane] = v;
}

__device__ __forceinline__ void cmpswap(unsigned long long& a, unsigned long long& b) {
  const unsigned long long x = a, y = b;
  a = x < y ? x : y, b = x < y ? y : x;
}
// half-cleaners of stride s_from .. 1 over p (a power of two <= kChunk) keys in LDS; ends with a barrier
__device__ __forceinline__ void lds_strides(unsigned long long* lds, int p, int s_from) {
  for (int s = s_from; s >= 1; s >>= 1) {
    for (int t = threadIdx.x; t < (p >> 1); t += 256) {
      const int i = (t / s) * 2 * s + (t % s);
      cmpswap(lds[i], lds[i + s]);
    }
    __syncthreads();
  }
}
__device__ __forceinline__ void lds_flip(unsigned long long* lds, int p, int k) {
  const int h = k >> 1;
  for (int t = threadIdx.x; t < (p >> 1); t += 256) {
    const int b = (t / h) * k, r = t % h;
    cmpswap(lds[b + r], lds[b + k - 1 - r]);
  }
  __syncthreads();
}

// one workgroup per long segment (list entry blockIdx.x).  Up to kChunk keys: wholly in LDS.  Beyond: each kChunk-chunk is sorted in LDS,
// then for k = 2 kChunk .. P the flip and the strides >= kChunk run on the segment in global memory and the strides below on chunks in LDS.
__global__ void __launch_bounds__(256) sort_long_kernel(const int* __restrict__ count, const int* __restrict__ offs,
                                                        unsigned long long* __restrict__ vals, const int* __restrict__ n_long,
                                                        const int* __restrict__ longs) {
  __shared__ unsigned long long lds[kChunk];
  if ((int)blockIdx.x >= *n_long) return;
  const int cell = longs[blockIdx.x];
  const unsigned n = (unsigned)count[cell];
  unsigned long long* seg = vals + offs[cell];
  if (n <= (unsigned)kChunk) {
    int p = kWaveCap * 2;
    while ((unsigned)p < n) p <<= 1;
    for (int i = threadIdx.x; i < p; i += 256) lds[i] = (unsigned)i < n ? seg[i] : kInf;
    __syncthreads();
    for (int k = 2; k <= p; k <<= 1) {
      lds_flip(lds, p, k);
      lds_strides(lds, p, k >> 2);
    }
    for (int i = threadIdx.x; (unsigned)i < n; i += 256) seg[i] = lds[i];
    return;
  }
  unsigned p = 2u * kChunk;  // n < 2^31, so p <= 2^31 fits
  while (p < n) p <<= 1;
  const unsigned chunks = (n + kChunk - 1) / kChunk;
  for (unsigned c = 0; c < chunks; ++c) {
    const unsigned base = c * kChunk;
    for (int i = threadIdx.x; i < kChunk; i += 256) lds[i] = base + i < n ? seg[base + i] : kInf;
    __syncthreads();
    for (int k = 2; k <= kChunk; k <<= 1) {
      lds_flip(lds, kChunk, k);
      lds_strides(lds, kChunk, k >> 2);
    }
    for (int i = threadIdx.x; i < kChunk; i += 256)
      if (base + i < n) seg[base + i] = lds[i];
    __syncthreads();
  }
  for (unsigned k = 2u * kChunk; k <= p && k != 0; k <<= 1) {
    const unsigned h = k >> 1;
    for (unsigned t = threadIdx.x; t < (p >> 1); t += 256) {  // flip
      const unsigned b = (t / h) * k, r = t % h;
      const unsigned i = b + r, j = b + (k - 1 - r);
      if (j < n) cmpswap(seg[i], seg[j]);
    }
    __syncthreads();
    for (unsigned s = k >> 2; s >= (unsigned)kChunk; s >>= 1) {
      for (unsigned t = threadIdx.x; t < (p >> 1); t += 256) {
        const unsigned i = (t / s) * 2 * s + (t % s), j = i + s;
        if (j < n) cmpswap(seg[i], seg[j]);
      }
      __syncthreads();
    }
    for (unsigned c = 0; c < chunks; ++c) {
      const unsigned base = c * kChunk;
      for (int i = threadIdx.x; i < kChunk; i += 256) lds[i] = base + i < n ? seg[base + i] : kInf;
      __syncthreads();
      lds_strides(lds, kChunk, kChunk >> 1);
      for (int i = threadIdx.x; i < kChunk; i += 256)
        if (base + i < n) seg[base + i] = lds[i];
      __syncthreads();
    }
  }
}

// ---- stage 5: one thread per cell reads its sorted segment ------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) reduce_kernel(const int* __restrict__ count, const int* __restrict__ offs, int cells,
                                                     const unsigned long long* __restrict__ vals, int mode, double* __restrict__ out) {
  const int cell = blockIdx.x * 256 + threadIdx.x;
  if (cell >= cells) return;
  const int n = count[cell];
  double r = __builtin_nan("");
  if (n > 0) {
    const unsigned long long* seg = vals + offs[cell];
    if (mode == kMin) {
      r = from_key(seg[0]);
    } else if (mode == kMax) {
      r = from_key(seg[n - 1]);
    } else if (mode == kMed) {
      r = (n & 1) ? from_key(seg[n >> 1]) : (from_key(seg[(n >> 1) - 1]) + from_key(seg[n >> 1])) / 2;
    } else {
      double s = 0;
      for (int i = 0; i < n; ++i) s += from_key(seg[i]);  // ascending: one fixed order
      r = s / n;
    }
  }
  out[cell] = r;
}

// scratch layout (bytes): vals 8 n | key 4 n | offs 4 cells | cursor 4 cells | bsum 4 nb | n_long 4 | longs 4 (n / 65), each rounded to 8
struct Layout {
  unsigned long long* vals;
  int *key, *offs, *cursor, *bsum, *n_long, *longs;
  int64_t bytes;
  int nb;
};
static Layout layout(void* base, int64_t n, int64_t cells) {
  ScratchCarver c(base);
  Layout l;
  l.nb = (int)((cells + kScanBlock - 1) / kScanBlock);
  l.vals = c.take<unsigned long long>(n, 8);
  l.key = c.take<int>(n, 8);
  l.offs = c.take<int>(cells, 8);
  l.cursor = c.take<int>(cells, 8);
  l.bsum = c.take<int>(l.nb, 8);
  l.n_long = c.take<int>(1, 8);
  l.longs = c.take<int>(n / (kWaveCap + 1), 8);
  l.bytes = c.bytes();
  return l;
}

}  // namespace cg
}  // namespace sr

using namespace sr;
using namespace sr::cg;

// int32 offsets everywhere, with room for a launch's last partial block of indices
constexpr int64_t kMaxCount = 2147483648LL - 4096;
static int check_sizes(const char* who, int64_t n, int map_w, int map_h) {
  SR_REQUIRE(n >= 0 && n <= kMaxCount, "%s: the point count must be in [0, 2^31 - 4096] (got %lld)", who, (long long)n);
  SR_REQUIRE(map_w >= 1 && map_h >= 1, "%s: empty grid (%d x %d)", who, map_h, map_w);
  SR_REQUIRE((int64_t)map_w * map_h <= kMaxCount, "%s: the grid must hold at most 2^31 - 4096 cells (got %d x %d)", who, map_h, map_w);
  return 0;
}

extern "C" int sr_cloud_grid_scratch(int64_t n, int map_w, int map_h, int64_t* bytes) {
  SR_REQUIRE(bytes, "sr_cloud_grid_scratch: null pointer");
  if (check_sizes("sr_cloud_grid_scratch", n, map_w, map_h)) return 1;
  *bytes = layout(nullptr, n, (int64_t)map_w * map_h).bytes;
  return 0;
}

extern "C" int sr_cloud_grid(const double* east, const double* north, const double* alt, int64_t n, double x0, double y0,
                             double definition, int map_w, int map_h, int rule, int mode, void* scratch, int64_t scratch_bytes,
                             double* out, int* count, int stages, void* stream) {
  if (check_sizes("sr_cloud_grid", n, map_w, map_h)) return 1;
  SR_REQUIRE(out && count, "sr_cloud_grid: null pointer");
  SR_REQUIRE(n == 0 || (east && north && alt), "sr_cloud_grid: null pointer");
  SR_REQUIRE(rule == kRuleNearest || rule == kRuleFloor, "sr_cloud_grid: rule must be 0 (nearest) or 1 (floor) (got %d)", rule);
  SR_REQUIRE(mode >= kMin && mode <= kMed, "sr_cloud_grid: mode must be 0 (min), 1 (max), 2 (avg) or 3 (med) (got %d)", mode);
  SR_REQUIRE(isfinite(definition) && definition > 0, "sr_cloud_grid: definition must be finite and > 0 (got %g)", definition);
  SR_REQUIRE(isfinite(x0) && isfinite(y0), "sr_cloud_grid: non-finite grid origin");
  SR_REQUIRE(stages >= 0 && stages <= 5, "sr_cloud_grid: stages must be in 0..5 (got %d)", stages);
  const int cells = map_w * map_h;
  const Layout l = layout(scratch, n, cells);
  if (require_scratch("sr_cloud_grid", scratch ? scratch_bytes : 0, l.bytes)) return 1;
  SR_REQUIRE(((uintptr_t)scratch & 7) == 0, "sr_cloud_grid: scratch must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int last = stages == 0 ? 5 : stages;
  const int ni = (int)n;
  const unsigned pgrid = blocks_for(n), cgrid = blocks_for(cells);

  if (hipMemsetAsync(count, 0, (size_t)cells * sizeof(int), s) != hipSuccess) {
    set_error("sr_cloud_grid: hipMemsetAsync of the counts failed");
    return 2;
  }
  if (n > 0) {
    hipLaunchKernelGGL(key_count_kernel, dim3(pgrid), dim3(256), 0, s, east, north, alt, ni, x0, y0, definition, map_w, map_h, rule, l.key,
                       count);
    if (check_launch("cloud_grid key_count_kernel")) return 2;
    if (last >= 2) {
      hipLaunchKernelGGL(scan_sums_kernel, dim3(l.nb), dim3(256), 0, s, count, cells, l.bsum);
      if (check_launch("cloud_grid scan_sums_kernel")) return 2;
      hipLaunchKernelGGL(scan_carry_kernel, dim3(1), dim3(256), 0, s, l.bsum, l.nb, l.n_long);
      if (check_launch("cloud_grid scan_carry_kernel")) return 2;
      hipLaunchKernelGGL(scan_add_kernel, dim3(l.nb), dim3(256), 0, s, count, cells, l.bsum, l.offs, l.cursor);
      if (check_launch("cloud_grid scan_add_kernel")) return 2;
    }
    if (last >= 3) {
      hipLaunchKernelGGL(scatter_kernel, dim3(pgrid), dim3(256), 0, s, alt, ni, l.key, l.cursor, l.vals);
      if (check_launch("cloud_grid scatter_kernel")) return 2;
    }
    if (last >= 4) {
      hipLaunchKernelGGL(sort_wave_kernel, dim3((unsigned)((cells + 3) / 4)), dim3(256), 0, s, count, l.offs, cells, l.vals, l.n_long, l.longs);
      if (check_launch("cloud_grid sort_wave_kernel")) return 2;
      const int64_t max_long = n / (kWaveCap + 1) < cells ? n / (kWaveCap + 1) : cells;  // segments longer than kWaveCap
      if (max_long > 0) {
        hipLaunchKernelGGL(sort_long_kernel, dim3((unsigned)max_long), dim3(256), 0, s, count, l.offs, l.vals, l.n_long, l.longs);
        if (check_launch("cloud_grid sort_long_kernel")) return 2;
      }
    }
  }
  if (last >= 5) {
    hipLaunchKernelGGL(reduce_kernel, dim3(cgrid), dim3(256), 0, s, count, l.offs, cells, l.vals, mode, out);
    if (check_launch("cloud_grid reduce_kernel")) return 2;
  }
  return 0;
}
