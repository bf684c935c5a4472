// Tie-point interpolation on the GPU: study_depth_supervision.idw_interpolation (:64-103), an exact
// N-nearest-neighbour inverse-distance weighting that the reference runs with scipy's cKDTree, and scipy.ndimage.gaussian_filter with
// mode "reflect" (:36), the two steps of save_heatmap_of_reprojection_error (:18-61) and check_depth_supervision_points (:105-203).
//
// kNN: a uniform grid of square cells over the points' bounding box, built per call in four launches -- grid_setup_kernel (one
// workgroup: bounds, cell size, zeroed counts), count_kernel (cell of each point; an integer atomicAdd gives its rank inside the cell),
// scan_kernel (one workgroup: exclusive scan of the counts), scatter_kernel (points sorted by cell).  idw_kernel gives each query one
// thread that visits Chebyshev rings of cells around the query's cell, clipped to the grid, and keeps the N best (d^2, index) pairs
// in registers in lexicographic order.  It stops once every unvisited cell lies farther than the N-th best (the distance from the
// query to the visited block's sides, less a slack for rounding) or the whole grid is visited.  The selection is an exact function of
// the point set, so the order the atomics land in does not matter: results are bitwise repeatable.  IDW in fp64 in increasing
// (d^2, index) order.  Non-finite points go to an overflow bucket that no query visits.
//
// Gaussian: two LDS-tiled passes, axis 0 then axis 1 (scipy's order), fp64 in and out, reflect borders by index mapping (period 2n),
// each output summed as scipy's correlate1d does for a symmetric kernel: x[i] w[0], then + (x[i-k] + x[i+k]) w[k] for k = r .. 1.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace sr {
namespace tiep {

constexpr int kThreads = 256;
constexpr int kSetupThreads = 1024;
constexpr int64_t kMaxCells = (int64_t)1 << 22;
constexpr int kMaxRadius = 200;        // Gaussian taps per side; scipy's radius = int(truncate * sigma + 0.5)
constexpr int kColW = 16, kColH = 64;  // axis-0 pass: 16 columns x 64 output rows per workgroup, (64 + 2r) x 16 doubles of LDS
constexpr int kRowW = 256;             // axis-1 pass: 256 outputs of one row per workgroup, 256 + 2r doubles of LDS

struct GridParams {
  double x0, y0, s, inv_s;
  int gx, gy, n_valid, pad;
};

// cells of the grid for k points and n neighbours: about max(2, n / 2) points per cell
inline int64_t grid_cells(int64_t k, int n) {
  const int64_t per = n / 2 > 2 ? n / 2 : 2;
  const int64_t c = (k + per - 1) / per;
  return c < 1 ? 1 : (c > kMaxCells ? kMaxCells : c);
}

struct Scratch {
  GridParams* prm;
  int *start, *cell, *rank, *sidx;
  double *sx, *sy;
};

// byte layout of the scratch, every piece rounded to 256 bytes (base == nullptr: sizes only)
inline int64_t scratch_layout(int64_t k, int64_t cells, void* base, Scratch* s) {
  ScratchCarver c(base);
  GridParams* prm = c.take<GridParams>(1, 256);
  int* start = c.take<int>(cells + 2, 256);  // the cells, the overflow bucket, the end
  int* cell = c.take<int>(k, 256);
  int* rank = c.take<int>(k, 256);
  int* sidx = c.take<int>(k, 256);
  double* sx = c.take<double>(k, 256);
  double* sy = c.take<double>(k, 256);
  if (s) *s = Scratch{prm, start, cell, rank, sidx, sx, sy};
  return c.bytes();
}

__device__ __forceinline__ bool finite2(double x, double y) { return isfinite(x) && isfinite(y); }

// bounds of the finite points -> square cells of side s with gx x gy <= cells; zeroes the counts
__global__ void __launch_bounds__(kSetupThreads) grid_setup_kernel(const double* __restrict__ pts, int64_t k, int64_t cells,
                                                                   GridParams* __restrict__ prm, int* __restrict__ count) {
  for (int64_t c = threadIdx.x; c < cells + 2; c += kSetupThreads) count[c] = 0;
  double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
  int nv = 0;
  for (int64_t i = threadIdx.x; i < k; i += kSetupThreads) {
    const double x = pts[2 * i], y = pts[2 * i + 1];
    if (!finite2(x, y)) continue;
    xmin = fmin(xmin, x), xmax = fmax(xmax, x), ymin = fmin(ymin, y), ymax = fmax(ymax, y);
    ++nv;
  }
  for (int off = 32; off >= 1; off >>= 1) {
    xmin = fmin(xmin, __shfl_xor(xmin, off)), xmax = fmax(xmax, __shfl_xor(xmax, off));
    ymin = fmin(ymin, __shfl_xor(ymin, off)), ymax = fmax(ymax, __shfl_xor(ymax, off));
    nv += __shfl_xor(nv, off);
  }
  __shared__ double red[4][kSetupThreads / 64];
  __shared__ int rn[kSetupThreads / 64];
  const int wv = threadIdx.x / 64;
  if ((threadIdx.x & 63) == 0) red[0][wv] = xmin, red[1][wv] = xmax, red[2][wv] = ymin, red[3][wv] = ymax, rn[wv] = nv;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int j = 1; j < kSetupThreads / 64; ++j) {
    xmin = fmin(xmin, red[0][j]), xmax = fmax(xmax, red[1][j]), ymin = fmin(ymin, red[2][j]), ymax = fmax(ymax, red[3][j]);
    nv += rn[j];
  }
  GridParams g;
  g.n_valid = nv, g.pad = 0;
  if (nv == 0) {
    g.x0 = g.y0 = 0.0, g.s = g.inv_s = 1.0, g.gx = g.gy = 1;
  } else {
    const double ex = xmax - xmin, ey = ymax - ymin, c = (double)cells;
    double s = fmax(sqrt(ex * ey / c), fmax(ex, ey) / c);  // ex / s and ey / s <= cells
    s = fmax(s, 1e-12 * (fabs(xmin) + fabs(ymin) + 1.0));   // coincident points: no zero or denormal cell
    double fx, fy;
    for (;;) {  // grow s until gx * gy fits
      fx = floor(ex / s) + 1.0, fy = floor(ey / s) + 1.0;
      if (fx * fy <= c) break;
      s *= 1.0625;
    }
    g.x0 = xmin, g.y0 = ymin, g.s = s, g.inv_s = 1.0 / s, g.gx = (int)fx, g.gy = (int)fy;
  }
  *prm = g;
}

__device__ __forceinline__ int64_t cell_coord(double v, double v0, double inv_s) {
  double c = floor((v - v0) * inv_s);
  c = fmin(fmax(c, -1073741824.0), 1073741824.0);  // far queries: the ring search starts at the grid's edge anyway
  return (int64_t)c;
}

__global__ void __launch_bounds__(kThreads) count_kernel(const double* __restrict__ pts, int64_t k, int64_t cells,
                                                         const GridParams* __restrict__ prm, int* __restrict__ count,
                                                         int* __restrict__ cell, int* __restrict__ rank) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= k) return;
  const GridParams g = *prm;
  const double x = pts[2 * i], y = pts[2 * i + 1];
  int64_t c = cells;  // the overflow bucket
  if (finite2(x, y)) {
    int64_t cx = cell_coord(x, g.x0, g.inv_s), cy = cell_coord(y, g.y0, g.inv_s);
    cx = cx < 0 ? 0 : (cx >= g.gx ? g.gx - 1 : cx);
    cy = cy < 0 ? 0 : (cy >= g.gy ? g.gy - 1 : cy);
    c = cy * g.gx + cx;
  }
  cell[i] = (int)c;
  rank[i] = atomicAdd(count + c, 1);
}

// exclusive scan of n = cells + 2 counts in place (one workgroup: a contiguous chunk per thread, then a scan of the chunk sums)
__global__ void __launch_bounds__(kSetupThreads) scan_kernel(int* __restrict__ count, int64_t n) {
  __shared__ int part[kSetupThreads];
  const int64_t chunk = (n + kSetupThreads - 1) / kSetupThreads;
  const int64_t a = threadIdx.x * chunk, b = a + chunk < n ? a + chunk : n;
  int s = 0;
  for (int64_t i = a; i < b; ++i) s += count[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int off = 1; off < kSetupThreads; off <<= 1) {
    const int v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int run = part[threadIdx.x] - s;
  for (int64_t i = a; i < b; ++i) {
    const int c = count[i];
    count[i] = run;
    run += c;
  }
}

__global__ void __launch_bounds__(kThreads) scatter_kernel(const double* __restrict__ pts, int64_t k, const int* __restrict__ start,
                                                           const int* __restrict__ cell, const int* __restrict__ rank,
                                                           double* __restrict__ sx, double* __restrict__ sy, int* __restrict__ sidx) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= k) return;
  const int p = start[cell[i]] + rank[i];
  sx[p] = pts[2 * i], sy[p] = pts[2 * i + 1], sidx[p] = (int)i;
}

__device__ __forceinline__ bool before(double d, int i, double bd, int bi) { return d < bd || (d == bd && i < bi); }

// Sorted ascending list of NMAX (d^2, index) slots.  Slots 0 .. NMAX-n-1 hold -inf sentinels that never move, so the live n entries
// sit at NMAX-n .. NMAX-1 and the worst is always slot NMAX-1: static register indices only.
template <int NMAX>
__device__ __forceinline__ void offer(double d, int i, double (&bd)[NMAX], int (&bi)[NMAX]) {
  if (!before(d, i, bd[NMAX - 1], bi[NMAX - 1])) return;
#pragma unroll
  for (int j = NMAX - 1; j >= 0; --j) {
    if (j > 0 && before(d, i, bd[j - 1], bi[j - 1])) {
      bd[j] = bd[j - 1], bi[j] = bi[j - 1];
    } else if (before(d, i, bd[j], bi[j])) {
      bd[j] = d, bi[j] = i;
    }
  }
}

template <int NMAX>
__device__ __forceinline__ void scan_run(int a, int b, double qx, double qy, const double* __restrict__ sx, const double* __restrict__ sy,
                                         const int* __restrict__ sidx, double (&bd)[NMAX], int (&bi)[NMAX], int& seen) {
#pragma clang fp contract(off)
  seen += b - a;
  for (int p = a; p < b; ++p) {
    const double dx = qx - sx[p], dy = qy - sy[p];
    offer<NMAX>(dx * dx + dy * dy, sidx[p], bd, bi);
  }
}

// One thread per query: explicit (col, row) pairs, or (query == nullptr) pixel i = (i % width, i / width) of the raster, walked in
// 16 x 16 tiles (8 x 8 per wave) so that a wave's lanes share cells.
template <int NMAX>
__global__ void __launch_bounds__(kThreads) idw_kernel(const GridParams* __restrict__ prm, const int* __restrict__ start,
                                                       const double* __restrict__ sx, const double* __restrict__ sy,
                                                       const int* __restrict__ sidx, const float* __restrict__ z, int n,
                                                       const double* __restrict__ query, int64_t n_query, int width, int height,
                                                       double* __restrict__ out, int* __restrict__ nn_idx, int* __restrict__ visited) {
#pragma clang fp contract(off)
  int64_t q;
  double qx, qy;
  if (query) {
    q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= n_query) return;
    qx = query[2 * q], qy = query[2 * q + 1];
  } else {
    const int tiles_x = (width + 15) / 16;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int px = tx * 16 + (wv & 1) * 8 + (l & 7), py = ty * 16 + (wv >> 1) * 8 + (l >> 3);
    if (px >= width || py >= height) return;
    q = (int64_t)py * width + px;
    qx = (double)px, qy = (double)py;
  }
  double bd[NMAX];
  int bi[NMAX];
#pragma unroll
  for (int j = 0; j < NMAX; ++j) {
    const bool live = j >= NMAX - n;
    bd[j] = live ? INFINITY : -INFINITY;
    bi[j] = live ? INT_MAX : -1;
  }
  int seen = 0;
  const GridParams g = *prm;
  if (finite2(qx, qy) && g.n_valid > 0) {
    const int64_t gx = g.gx, gy = g.gy;
    const int64_t cx = cell_coord(qx, g.x0, g.inv_s), cy = cell_coord(qy, g.y0, g.inv_s);
    int64_t r = 0;  // the first ring that meets the grid
    r = -cx > r ? -cx : r;
    r = cx - (gx - 1) > r ? cx - (gx - 1) : r;
    r = -cy > r ? -cy : r;
    r = cy - (gy - 1) > r ? cy - (gy - 1) : r;
    // rounding slack of the cell assignment and of the side distances: far below any distance that separates two keypoints
    const double slack = 1e-9 * (fabs(qx - g.x0) + fabs(qy - g.y0) + (double)(gx + gy) * g.s);
    for (;; ++r) {
      const int64_t xa = cx - r < 0 ? 0 : cx - r, xb = cx + r > gx - 1 ? gx - 1 : cx + r;
      for (int side = 0; side < 2; ++side) {  // rows cy - r and cy + r (one row when r == 0): their cells are contiguous
        const int64_t y = side ? cy + r : cy - r;
        if ((side && r == 0) || y < 0 || y >= gy || xa > xb) continue;
        scan_run<NMAX>(start[y * gx + xa], start[y * gx + xb + 1], qx, qy, sx, sy, sidx, bd, bi, seen);
      }
      if (r > 0) {
        const int64_t ya = cy - r + 1 < 0 ? 0 : cy - r + 1, yb = cy + r - 1 > gy - 1 ? gy - 1 : cy + r - 1;
        for (int side = 0; side < 2; ++side) {  // columns cx - r and cx + r without their corners
          const int64_t x = side ? cx + r : cx - r;
          if (x < 0 || x >= gx) continue;
          for (int64_t y = ya; y <= yb; ++y) scan_run<NMAX>(start[y * gx + x], start[y * gx + x + 1], qx, qy, sx, sy, sidx, bd, bi, seen);
        }
      }
      const bool left = cx - r > 0, right = cx + r < gx - 1, top = cy - r > 0, bottom = cy + r < gy - 1;
      if (!(left || right || top || bottom)) break;  // every cell visited
      if (bd[NMAX - 1] < INFINITY) {
        double lb = INFINITY;
        if (left) lb = fmin(lb, qx - (g.x0 + (double)(cx - r) * g.s));
        if (right) lb = fmin(lb, g.x0 + (double)(cx + r + 1) * g.s - qx);
        if (top) lb = fmin(lb, qy - (g.y0 + (double)(cy - r) * g.s));
        if (bottom) lb = fmin(lb, g.y0 + (double)(cy + r + 1) * g.s - qy);
        lb -= slack;
        if (lb > 0 && lb * lb * (1.0 - 1e-12) > bd[NMAX - 1]) break;  // no unvisited point can enter the list
      }
    }
  }
  double v = __builtin_nan("");
  const bool full = bi[NMAX - 1] != INT_MAX && finite2(qx, qy);  // fewer than n finite points: NaN, indices -1
  if (full) {
    int first = 0;
    double d0 = 0.0;
#pragma unroll
    for (int j = 0; j < NMAX; ++j)
      if (j == NMAX - n) first = bi[j], d0 = sqrt(bd[j]);
    if (n == 1 || d0 < 1e-10) {  // one neighbour, or the query falls on a keypoint (:101; also d = 0, where 1/d is inf)
      v = (double)z[first];
    } else {
      double sw = 0.0;
#pragma unroll
      for (int j = 0; j < NMAX; ++j)
        if (j >= NMAX - n) sw += 1.0 / sqrt(bd[j]);
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < NMAX; ++j)
        if (j >= NMAX - n) acc += ((1.0 / sqrt(bd[j])) / sw) * (double)z[bi[j]];
      v = acc;
    }
  }
  out[q] = v;
  if (nn_idx) {
    int* o = nn_idx + q * n;
#pragma unroll
    for (int j = 0; j < NMAX; ++j)
      if (j >= NMAX - n) o[j - (NMAX - n)] = full ? bi[j] : -1;
  }
  if (visited) visited[q] = seen;
}

// reflect mode (half-sample symmetric, period 2n) for any i
__device__ __forceinline__ int reflect_index(int64_t i, int n) {
  const int64_t p = 2 * (int64_t)n;
  int64_t m = i % p;
  if (m < 0) m += p;
  return (int)(m < n ? m : p - 1 - m);
}

// axis 0: out[y, x] from rows y - r .. y + r of column x; a workgroup stages kColH + 2r rows of kColW columns
__global__ void __launch_bounds__(kThreads) gauss_axis0_kernel(const double* __restrict__ in, int h, int w, const double* __restrict__ taps,
                                                               int r, double* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ double lds[];
  double* wk = lds;              // wk[k] = the tap at offset +-k
  double* tile = lds + (r + 1);  // (kColH + 2r) rows x kColW columns
  const int c0 = blockIdx.x * kColW, r0 = blockIdx.y * kColH;
  for (int k = threadIdx.x; k <= r; k += kThreads) wk[k] = taps[r + k];
  const int n_el = (kColH + 2 * r) * kColW;
  for (int e = threadIdx.x; e < n_el; e += kThreads) {
    const int rr = e / kColW, x = c0 + e % kColW;
    tile[e] = x < w ? in[(int64_t)reflect_index((int64_t)r0 - r + rr, h) * w + x] : 0.0;
  }
  __syncthreads();
  const int cc = threadIdx.x % kColW, ry = threadIdx.x / kColW, x = c0 + cc;
  if (x >= w) return;
  for (int m = 0; m < kColH / (kThreads / kColW); ++m) {
    const int yy = ry + m * (kThreads / kColW), y = r0 + yy;
    if (y >= h) break;
    const double* t = tile + (yy + r) * kColW + cc;
    double acc = t[0] * wk[0];
    for (int k = r; k >= 1; --k) acc += (t[-k * kColW] + t[k * kColW]) * wk[k];
    out[(int64_t)y * w + x] = acc;
  }
}

// axis 1: out[y, x] from columns x - r .. x + r of row y; a workgroup stages kRowW + 2r samples of one row
__global__ void __launch_bounds__(kThreads) gauss_axis1_kernel(const double* __restrict__ in, int h, int w, const double* __restrict__ taps,
                                                               int r, double* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ double lds[];
  double* wk = lds;
  double* seg = lds + (r + 1);
  const int x0 = blockIdx.x * kRowW, y = blockIdx.y;
  const double* row = in + (int64_t)y * w;
  for (int k = threadIdx.x; k <= r; k += kThreads) wk[k] = taps[r + k];
  for (int e = threadIdx.x; e < kRowW + 2 * r; e += kThreads) seg[e] = row[reflect_index((int64_t)x0 - r + e, w)];
  __syncthreads();
  const int x = x0 + threadIdx.x;
  if (x >= w) return;
  const double* t = seg + threadIdx.x + r;
  double acc = t[0] * wk[0];
  for (int k = r; k >= 1; --k) acc += (t[-k] + t[k]) * wk[k];
  out[(int64_t)y * w + x] = acc;
}

}  // namespace tiep
}  // namespace sr

using namespace sr;
using namespace sr::tiep;

extern "C" int sr_idw_grid_scratch(int64_t k, int n_neighbors, int64_t* bytes) {
  SR_REQUIRE(bytes, "sr_idw_grid_scratch: null pointer");
  SR_REQUIRE(n_neighbors >= 1 && n_neighbors <= 32, "sr_idw_grid_scratch: n_neighbors must be in 1..32 (got %d)", n_neighbors);
  SR_REQUIRE(k >= n_neighbors && k <= ((int64_t)1 << 30), "sr_idw_grid_scratch: need n_neighbors <= k <= 2^30 points (got %lld for %d)",
             (long long)k, n_neighbors);
  *bytes = scratch_layout(k, grid_cells(k, n_neighbors), nullptr, nullptr);
  return 0;
}

template <int NMAX>
static void launch_idw(unsigned grid, hipStream_t st, const Scratch& s, const float* z, int n, const double* query, int64_t nq, int width,
                       int height, double* out, int* nn_idx, int* visited) {
  hipLaunchKernelGGL(idw_kernel<NMAX>, dim3(grid), dim3(kThreads), 0, st, (const GridParams*)s.prm, (const int*)s.start,
                     (const double*)s.sx, (const double*)s.sy, (const int*)s.sidx, z, n, query, nq, width, height, out, nn_idx, visited);
}

extern "C" int sr_idw_interpolate(const double* pts2d, const float* z, int64_t k, const double* query, int64_t n_query, int height, int width,
                                  int n_neighbors, void* scratch, int64_t scratch_bytes, double* out, int* nn_idx, int* visited, void* stream) {
  int64_t need = 0;
  if (sr_idw_grid_scratch(k, n_neighbors, &need)) return 1;
  SR_REQUIRE(pts2d && z && scratch && out, "sr_idw_interpolate: null pointer");
  if (require_scratch("sr_idw_interpolate", scratch_bytes, need)) return 1;
  int64_t nq;
  unsigned grid;
  if (query) {
    SR_REQUIRE(n_query >= 0 && n_query <= ((int64_t)1 << 36), "sr_idw_interpolate: n_query must be in 0..2^36 (got %lld)", (long long)n_query);
    nq = n_query;
    grid = blocks_for(nq);
  } else {
    SR_REQUIRE(height >= 1 && width >= 1 && height <= 65536 && width <= 65536,
               "sr_idw_interpolate: the raster must be 1..65536 pixels on each side (got %d x %d)", height, width);
    nq = (int64_t)height * width;
    grid = (unsigned)(((width + 15) / 16) * (int64_t)((height + 15) / 16));
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t cells = grid_cells(k, n_neighbors);
  Scratch s;
  scratch_layout(k, cells, scratch, &s);
  hipLaunchKernelGGL(grid_setup_kernel, dim3(1), dim3(kSetupThreads), 0, st, pts2d, k, cells, s.prm, s.start);
  if (check_launch("grid_setup_kernel")) return 2;
  const unsigned kb = blocks_for(k);
  hipLaunchKernelGGL(count_kernel, dim3(kb), dim3(kThreads), 0, st, pts2d, k, cells, (const GridParams*)s.prm, s.start, s.cell, s.rank);
  if (check_launch("count_kernel")) return 2;
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kSetupThreads), 0, st, s.start, cells + 2);
  if (check_launch("scan_kernel")) return 2;
  hipLaunchKernelGGL(scatter_kernel, dim3(kb), dim3(kThreads), 0, st, pts2d, k, (const int*)s.start, (const int*)s.cell, (const int*)s.rank,
                     s.sx, s.sy, s.sidx);
  if (check_launch("scatter_kernel")) return 2;
  if (nq == 0) return 0;
  const int n = n_neighbors;
  if (n <= 1)
    launch_idw<1>(grid, st, s, z, n, query, nq, width, height, out, nn_idx, visited);
  else if (n <= 2)
    launch_idw<2>(grid, st, s, z, n, query, nq, width, height, out, nn_idx, visited);
  else if (n <= 4)
    launch_idw<4>(grid, st, s, z, n, query, nq, width, height, out, nn_idx, visited);
  else if (n <= 8)
    launch_idw<8>(grid, st, s, z, n, query, nq, width, height, out, nn_idx, visited);
  else if (n <= 16)
    launch_idw<16>(grid, st, s, z, n, query, nq, width, height, out, nn_idx, visited);
  else
    launch_idw<32>(grid, st, s, z, n, query, nq, width, height, out, nn_idx, visited);
  return check_launch("idw_kernel");
}

extern "C" int sr_gaussian_filter_f64(const double* in, int h, int w, const double* taps0, int radius0, const double* taps1, int radius1,
                                      double* tmp, double* out, void* stream) {
  SR_REQUIRE(in && out, "sr_gaussian_filter_f64: null pointer");
  SR_REQUIRE(h >= 1 && w >= 1 && h <= 65535 && w <= 65535 * kRowW, "sr_gaussian_filter_f64: bad raster %d x %d", h, w);
  SR_REQUIRE(radius0 >= -1 && radius0 <= kMaxRadius && radius1 >= -1 && radius1 <= kMaxRadius,
             "sr_gaussian_filter_f64: radii must be in -1..%d (got %d, %d)", kMaxRadius, radius0, radius1);
  SR_REQUIRE((radius0 < 0 || taps0) && (radius1 < 0 || taps1), "sr_gaussian_filter_f64: null taps");
  SR_REQUIRE(in != out && (radius0 < 0 || radius1 < 0 || (tmp && tmp != in && tmp != out)),
             "sr_gaussian_filter_f64: in, tmp and out must be distinct buffers (tmp is needed when both axes are filtered)");
  hipStream_t st = (hipStream_t)stream;
  if (radius0 < 0 && radius1 < 0) {
    SR_REQUIRE(hipMemcpyAsync(out, in, (size_t)h * w * sizeof(double), hipMemcpyDeviceToDevice, st) == hipSuccess,
               "sr_gaussian_filter_f64: hipMemcpyAsync failed");
    return 0;
  }
  const double* src = in;
  if (radius0 >= 0) {
    double* dst = radius1 >= 0 ? tmp : out;
    const size_t lds = (size_t)(radius0 + 1 + (kColH + 2 * radius0) * kColW) * sizeof(double);
    hipLaunchKernelGGL(gauss_axis0_kernel, dim3((w + kColW - 1) / kColW, (h + kColH - 1) / kColH), dim3(kThreads), lds, st, src, h, w, taps0,
                       radius0, dst);
    if (check_launch("gauss_axis0_kernel")) return 2;
    src = dst;
  }
  if (radius1 >= 0) {
    const size_t lds = (size_t)(radius1 + 1 + kRowW + 2 * radius1) * sizeof(double);
    hipLaunchKernelGGL(gauss_axis1_kernel, dim3((w + kRowW - 1) / kRowW, h), dim3(kThreads), lds, st, src, h, w, taps1, radius1, out);
    if (check_launch("gauss_axis1_kernel")) return 2;
  }
  return 0;
}
