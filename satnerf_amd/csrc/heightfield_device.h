// The traversal of a segment through the cells of a DSM raster, shared by the kernels of heightfield.hip.
// Plain fp64 C++ with contraction off and no device intrinsic, __host__ __device__: a CPU build walks bit for bit as the GPU does.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace sr {

constexpr int kHfBlock = 16;  // cells per side of a block of the two-level walk

struct HfGrid {  // host-filled, passed by value
  const float* hgt;       // (ysize, xsize), row 0 at y = 0 (north); a non-finite value is an empty cell
  const float* blockmax;  // (ceil(ysize / 16), ceil(xsize / 16)), -inf for a block without a finite cell; read only when accelerate
  const float* gmax;      // 1 value: the maximum over the raster, -inf without a finite cell
  double res;
  int xsize, ysize, bw, accelerate;
};

// One axis of a segment in the grid frame: coordinate a + s d, lines at k res, cells 0 .. n - 1.
struct HfAxis {
  double a, d, res;
  int n;
  // parameter of the crossing of line k, from the absolute index: never accumulated
  __host__ __device__ __forceinline__ double cross(int k) const {
#pragma clang fp contract(off)
    return ((double)k * res - a) / d;
  }
  // The cell the segment is in at parameter s, DEFINED by the crossing values: for d > 0 the largest k with cross(k) <= s, for d < 0
  // the smallest k with cross(k + 1) <= s, for d = 0 the k with k res <= a < (k + 1) res.  The floor of the position is only the
  // first guess.  Returns -1 / n when that cell lies outside the grid.  Both loops move towards their fixed point and stop at the
  // grid's edge: at most n steps (one, in practice).
  __host__ __device__ __forceinline__ int index_at(double s) const {
#pragma clang fp contract(off)
    const double p = (a + s * d) / res;
    int k = p >= (double)(n - 1) ? n - 1 : (p > 0 ? (int)p : 0);  // a NaN lands on 0
    if (d > 0) {
      while (k < n && cross(k + 1) <= s) ++k;
      while (k >= 0 && cross(k) > s) --k;
    } else if (d < 0) {
      while (k >= 0 && cross(k) <= s) --k;
      while (k < n && cross(k + 1) > s) ++k;
    } else {
      while (k < n && (double)(k + 1) * res <= a) ++k;
      while (k >= 0 && (double)k * res > a) --k;
    }
    return k;
  }
  // The line the segment leaves cell k through -- or, with `block`, the block of cell k: its far line, or the grid's edge line n where
  // the block is a partial one -- the crossing of that line (inf where the axis stands still), and the cell behind it.
  __host__ __device__ __forceinline__ int exit_line(int k, bool block) const {
    if (!block) return d > 0 ? k + 1 : k;
    if (d > 0) {
      const int line = (k / kHfBlock + 1) * kHfBlock;
      return line < n ? line : n;
    }
    return k / kHfBlock * kHfBlock;
  }
  __host__ __device__ __forceinline__ double line_cross(int line) const { return d != 0 ? cross(line) : __builtin_inf(); }
  __host__ __device__ __forceinline__ int behind(int line) const { return d > 0 ? line : line - 1; }
  // [lo, hi] of s over which the coordinate lies within the grid's extent [0, n res]; false when it never does
  __host__ __device__ __forceinline__ bool clip(double& lo, double& hi) const {
    if (d > 0) {
      lo = cross(0), hi = cross(n);
    } else if (d < 0) {
      lo = cross(n), hi = cross(0);
    } else {
      lo = -__builtin_inf(), hi = __builtin_inf();
      return a >= 0 && a < (double)n * res;
    }
    return true;
  }
};

// The walk of DESIGN.md section 7.15.  A -> B in the grid frame, s in [0, 1]; `skip` = the index of a cell that is passed through
// whatever its height (the shadow mask's start cell), or -1.  Returns true on a hit and sets s_hit and cell = j xsize + c.
// The state (c, j, s_in) is at every step the cell given by HfAxis::index_at on both axes.  The two-level walk takes the same step
// with a block's lines in place of a cell's where the block's maximum lies below the segment (a rising segment is lowest where it
// enters the block, a falling one where it leaves it), and re-derives by index_at the index of the axis it did not cross: it passes
// through the same states as the plain walk and tests the same cells with the same s_in and s_out -- bit-identical results.
__host__ __device__ __forceinline__ bool hf_walk(const HfGrid& g, double xa, double ya, double za, double xb, double yb, double zb, int skip,
                                                 double& s_hit, int& cell) {
#pragma clang fp contract(off)
  const HfAxis X = {xa, xb - xa, g.res, g.xsize}, Y = {ya, yb - ya, g.res, g.ysize};
  const double dz = zb - za;
  if (!(isfinite(xa) && isfinite(ya) && isfinite(za) && isfinite(X.d) && isfinite(Y.d) && isfinite(dz) && isfinite(xb) && isfinite(yb) &&
        isfinite(zb)))
    return false;
  double lx, hx, ly, hy;
  if (!X.clip(lx, hx) || !Y.clip(ly, hy)) return false;
  double s_in = 0.0, s_end = 1.0;
  s_in = lx > s_in ? lx : s_in, s_in = ly > s_in ? ly : s_in;
  s_end = hx < s_end ? hx : s_end, s_end = hy < s_end ? hy : s_end;
  if (!(s_in <= s_end)) return false;
  int c = X.index_at(s_in), j = Y.index_at(s_in);
  if (c < 0 || c >= g.xsize || j < 0 || j >= g.ysize) return false;
  const double gmax = g.accelerate ? (double)*g.gmax : 0.0;
  bool fresh = g.accelerate != 0;  // (c, j) is the first cell of a block not yet judged
  // every turn either ends the walk or moves (c, j) one cell or one block onwards along the segment: at most xsize + ysize turns
  for (;;) {
    bool jump = false;  // this turn steps over the whole block
    int kx = X.exit_line(c, false), ky = Y.exit_line(j, false);
    if (fresh) {
      const double bmax = (double)g.blockmax[(j / kHfBlock) * g.bw + c / kHfBlock];
      if (dz >= 0) {
        const double z_in = za + s_in * dz;
        if (z_in > gmax) return false;  // rising above everything
        jump = z_in > bmax;
      } else {
        const double bx = X.line_cross(X.exit_line(c, true)), by = Y.line_cross(Y.exit_line(j, true));
        const double s_nb = bx < by ? bx : by;
        jump = za + (s_nb < 1.0 ? s_nb : 1.0) * dz > bmax;
      }
      if (jump) kx = X.exit_line(c, true), ky = Y.exit_line(j, true);
      fresh = false;
    }
    const double sx = X.line_cross(kx), sy = Y.line_cross(ky);
    const double s_next = sx < sy ? sx : sy;
    if (!jump) {
      const double s_out = s_next < 1.0 ? s_next : 1.0;
      const int idx = j * g.xsize + c;
      const float hf = g.hgt[idx];
      if (idx != skip && isfinite(hf)) {
        const double h = (double)hf;
        if (za + s_in * dz <= h) {  // a wall, or a start inside the column
          s_hit = s_in, cell = idx;
          return true;
        }
        if (za + s_out * dz <= h) {  // the top
          s_hit = (h - za) / dz, cell = idx;
          return true;
        }
      }
    }
    if (s_next >= 1.0) return false;
    const int c0 = c, j0 = j;
    // on a tie both step: the two cells touched at a point are not visited
    if (sx <= s_next) c = X.behind(kx);
    else if (jump) c = X.index_at(s_next);
    if (sy <= s_next) j = Y.behind(ky);
    else if (jump) j = Y.index_at(s_next);
    if (c < 0 || c >= g.xsize || j < 0 || j >= g.ysize) return false;
    s_in = s_next;
    fresh = g.accelerate && (c / kHfBlock != c0 / kHfBlock || j / kHfBlock != j0 / kHfBlock);
  }
}

}  // namespace sr
