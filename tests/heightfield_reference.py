"""fp64 numpy reference of the ray cast against a DSM raster (csrc/heightfield.hip), deliberately NOT a walk.

Every finite cell (j, c) of the raster is the solid column x in [c r, (c+1) r], y in [j r, (j+1) r], z <= h of the grid frame.  A
segment A -> B, s in [0, 1], is intersected with every column on its own -- a slab test in x and y, then z(s) <= h -- and the smallest
s wins.  A column the segment touches in a single point of its footprint (a corner, or a segment that ends on its edge) is not
visited, which is the kernel's tie rule; a segment that runs along a cell edge belongs to the cell the layout gives that edge to.
O(N * cells): fine at test size.

It also defines stability.  A ray is *stable* when this reference returns the same cell, or the same miss, for seven inputs: as given,
all heights +- delta, the segment shifted +- delta east and +- delta north.  Grazes and corner touches fail that and are left out of
the comparisons with the GPU; the inputs must keep at least 99 % of their rays (tests/test_heightfield_host.py asserts it).
"""
import functools

import numpy as np

from oracle import satnerf_oracle as O
from tests import ortho_reference as R
from tests import sun_rays_reference as S

BLOCK = 16


def _axis(a, d, k, r):
    """(lo, hi) of s over which coordinate a + s d lies in [k r, (k+1) r]: a (N, 1), d (N, 1), k (1, K).  Empty = (inf, -inf).  d = 0:
    everything or nothing, by the layout's half-open cell k r <= a < (k+1) r."""
    with np.errstate(all="ignore"):
        t1, t2 = (k * r - a) / d, ((k + 1) * r - a) / d
        lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
        inside = (k * r <= a) & (a < (k + 1) * r)
        still = d == 0
    lo = np.where(still, np.where(inside, -np.inf, np.inf), lo)
    hi = np.where(still, np.where(inside, np.inf, -np.inf), hi)
    return lo, hi


def cast_np(hgt, r, A, B, skip=None, chunk=512):
    """(s (N,) float64, NaN on a miss; cell (N,) int64 = j xsize + c, -1 on a miss) of segments A -> B ((N, 3) grid-frame metres)
    against the (ysize, xsize) raster ``hgt`` of resolution ``r``.  ``skip`` (N,): per ray one cell index that is passed through."""
    hgt = np.asarray(hgt, np.float64)
    A, B = np.asarray(A, np.float64).reshape(-1, 3), np.asarray(B, np.float64).reshape(-1, 3)
    ysize, xsize = hgt.shape
    n = A.shape[0]
    s_out, cell_out = np.full(n, np.nan), np.full(n, -1, np.int64)
    cols, rows = np.arange(xsize, dtype=np.float64)[None, :], np.arange(ysize, dtype=np.float64)[None, :]
    h = hgt.reshape(1, ysize, xsize)
    solid = np.isfinite(h)
    for i0 in range(0, n, chunk):
        a, b = A[i0:i0 + chunk], B[i0:i0 + chunk]
        d = b - a
        ok = np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(d).all(1)
        lox, hix = _axis(a[:, 0:1], d[:, 0:1], cols, r)  # (n, xsize)
        loy, hiy = _axis(a[:, 1:2], d[:, 1:2], rows, r)  # (n, ysize)
        lo = np.maximum(np.maximum(lox[:, None, :], loy[:, :, None]), 0.0)
        hi = np.minimum(np.minimum(hix[:, None, :], hiy[:, :, None]), 1.0)
        za, dz = a[:, 2].reshape(-1, 1, 1), d[:, 2].reshape(-1, 1, 1)
        with np.errstate(all="ignore"):
            sz = (h - za) / dz
        falling, rising = dz < 0, dz > 0
        level_in = (dz == 0) & (za <= h)
        loz = np.where(falling, sz, np.where(rising | level_in, -np.inf, np.inf))
        hiz = np.where(rising, sz, np.where(falling | level_in, np.inf, -np.inf))
        first, last = np.maximum(lo, loz), np.minimum(hi, hiz)
        hit = solid & (lo < hi) & (first <= last) & ok[:, None, None]
        if skip is not None:
            sk = np.asarray(skip)[i0:i0 + chunk]
            flat = hit.reshape(len(a), -1)
            flat[np.arange(len(a))[sk >= 0], sk[sk >= 0]] = False
        first = np.where(hit, first, np.inf).reshape(len(a), -1)
        best = first.argmin(1)
        s = first[np.arange(len(a)), best]
        found = np.isfinite(s)
        s_out[i0:i0 + chunk] = np.where(found, s, np.nan)
        cell_out[i0:i0 + chunk] = np.where(found, best, -1)
    return s_out, cell_out


def stable_np(hgt, r, A, B, delta, skip=None):
    """(stable (N,) bool, s, cell): the reference's result as given, and whether the six perturbed inputs give the same cell or miss."""
    hgt = np.asarray(hgt, np.float64)
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    s, cell = cast_np(hgt, r, A, B, skip)
    stable = np.ones(A.shape[0], bool)
    for dh, dx, dy in ((delta, 0, 0), (-delta, 0, 0), (0, delta, 0), (0, -delta, 0), (0, 0, -delta), (0, 0, delta)):  # y = yoff - north
        shift = np.array([dx, dy, 0.0])
        stable &= cast_np(hgt + dh, r, A + shift, B + shift, skip)[1] == cell
    return stable, s, cell


def blockmax_np(hgt):
    """((ceil(ysize / 16), ceil(xsize / 16)) fp32 block maxima, -inf for a block without a finite cell; the global maximum)."""
    hgt = np.asarray(hgt, np.float32)
    ysize, xsize = hgt.shape
    bh, bw = -(-ysize // BLOCK), -(-xsize // BLOCK)
    pad = np.full((bh * BLOCK, bw * BLOCK), -np.inf, np.float32)
    pad[:ysize, :xsize] = np.where(np.isfinite(hgt), hgt, -np.inf)
    bm = pad.reshape(bh, BLOCK, bw, BLOCK).max((1, 3))
    return bm, bm.max()


def shadow_segments_np(hgt, r, sun_d, bias=0.0):
    """The shadow mask's segments, one per cell in raster order: (A, B (N, 3), skip (N,) = the cell's own index or -1 where no ray is
    cast, lit (N,) float: NaN for an empty cell, 1 for a start at or above the raster's maximum, 0 where a ray is cast)."""
    hgt32 = np.asarray(hgt, np.float32)
    ysize, xsize = hgt32.shape
    h = hgt32.astype(np.float64).ravel()
    u = np.asarray(sun_d, np.float64)
    u = u / np.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    top = float(blockmax_np(hgt32)[1])
    jj, cc = np.divmod(np.arange(h.size), xsize)
    A = np.stack([(cc + 0.5) * r, (jj + 0.5) * r, h + bias], 1)
    finite = np.isfinite(h)
    cast = finite & (A[:, 2] < top)
    with np.errstate(all="ignore"):
        t = (top - A[:, 2]) / u[2]
        B = np.stack([A[:, 0] + t * u[0], A[:, 1] - t * u[1], np.full(h.size, top)], 1)
    lit = np.where(finite, np.where(cast, 0.0, 1.0), np.nan)
    return A, B, np.where(cast, np.arange(h.size), -1), lit, cast


def shadow_mask_np(hgt, r, sun_d, bias=0.0, delta=None):
    """(mask (ysize, xsize) float64: 1 lit, 0 shadowed, NaN empty; stable (ysize, xsize) bool, all True without ``delta``)."""
    hgt = np.asarray(hgt, np.float32)
    A, B, skip, lit, cast = shadow_segments_np(hgt, r, sun_d, bias)
    mask, stable = lit.copy(), np.ones(lit.size, bool)
    if cast.any():
        if delta is None:
            cell = cast_np(hgt, r, A[cast], B[cast], skip[cast])[1]
        else:
            stable[cast], _, cell = stable_np(hgt, r, A[cast], B[cast], delta, skip[cast])
        mask[cast] = np.where(cell < 0, 1.0, 0.0)
    return mask.reshape(hgt.shape), stable.reshape(hgt.shape)


# ---- the inputs the host and the GPU tests share ----------------------------------------------------------------------------------------
RES = 0.5
RASTERS = {"37x53": (53, 37, None), "16x16": (16, 16, None), "33x17": (17, 33, (0, 1)), "1x1": (1, 1, None),
           "37x53_hole": (53, 37, (2, 0))}  # name -> (ysize, xsize, the (block row, block column) made all-NaN)
H_LO, H_HI = 2.0, 30.0


@functools.lru_cache(maxsize=None)
def raster(name):
    """Random heights in [2, 30) m, fp32, read-only: rough ground in [2, 4) m with flat-roofed boxes of up to 5 x 5 cells on it (so
    that rays run far before they meet something), about 5 % NaN; some rasters have one all-NaN block."""
    ysize, xsize, hole = RASTERS[name]
    rng = np.random.default_rng(1000 + sorted(RASTERS).index(name))
    h = rng.uniform(H_LO, 4.0, (ysize, xsize)).astype(np.float32)
    for _ in range(-(-ysize * xsize // 60)):
        j, c, dj, dc = rng.integers(0, ysize), rng.integers(0, xsize), rng.integers(1, 6), rng.integers(1, 6)
        h[j:j + dj, c:c + dc] = np.float32(rng.uniform(6.0, H_HI))
    if ysize * xsize > 1:
        h[rng.random((ysize, xsize)) < 0.05] = np.nan
    if hole is not None:
        h[hole[0] * BLOCK:(hole[0] + 1) * BLOCK, hole[1] * BLOCK:(hole[1] + 1) * BLOCK] = np.nan
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def segments(name, n=2000):
    """About ``n`` random grid-frame segments over ``raster(name)``: elevations 8 .. 80 degrees, half rising and half falling; starts
    above the surface, inside columns and outside the grid; every eighth with one zero horizontal component.  (A, B) read-only."""
    hgt = raster(name)
    ysize, xsize = hgt.shape
    w, hh = xsize * RES, ysize * RES
    rng = np.random.default_rng(2000 + sorted(RASTERS).index(name))
    az = rng.uniform(0, 2 * np.pi, n)
    el = np.radians(rng.uniform(8, 80, n))
    length = rng.uniform(0.5, 1.5, n) * (w + hh)
    rising = np.arange(n) % 2 == 0
    kind = rng.integers(0, 4, n)  # 0, 1: a start in the grid; 2: inside a column; 3: outside the grid
    A = np.stack([rng.uniform(0, w, n), rng.uniform(0, hh, n), np.where(rising, rng.uniform(0, H_HI, n), rng.uniform(H_LO, 2 * H_HI, n))], 1)
    out = kind == 3
    A[out, 0] = np.where(rng.random(out.sum()) < 0.5, -rng.uniform(0.1, 5, out.sum()), w + rng.uniform(0.1, 5, out.sum()))
    A[kind == 2, 2] = rng.uniform(-1, H_LO, (kind == 2).sum())
    d = np.stack([np.sin(az) * np.cos(el), -np.cos(az) * np.cos(el), np.where(rising, 1, -1) * np.sin(el)], 1)
    axis = np.arange(n) % 16
    d[axis == 3, 0] = 0.0
    d[axis == 11, 1] = 0.0
    B = A + d * length[:, None]
    A.setflags(write=False), B.setflags(write=False)
    return A, B


def edge_segments(name):
    """Segments on the walk's special lines: exact diagonals through cell corners, both ways, and segments along cell edges (one zero
    component on a line k r), starting inside and outside the grid.  Mostly unstable by construction: for plain against two-level."""
    hgt = raster(name)
    ysize, xsize = hgt.shape
    A, B = [], []
    for k in range(0, min(xsize, ysize) + 1, max(1, min(xsize, ysize) // 6)):
        for z0, z1 in ((40.0, 1.0), (1.0, 40.0), (12.0, 12.0)):
            m = max(xsize, ysize) * RES + 1.0
            A += [(k * RES, 0.0, z0), (k * RES + m, m, z0), (-1.0, k * RES - 1.0, z0), (k * RES, -0.5, z0), (-0.5, k * RES, z0)]
            B += [(k * RES + m, m, z1), (k * RES, 0.0, z1), (m - 1.0, k * RES + m - 1.0, z1), (k * RES, m, z1), (m, k * RES, z1)]
    return np.array(A), np.array(B)


# ---- scene-frame rays: the all-numpy chain -------------------------------------------------------------------------------------------
def utm_segments_np(rays, center, scene_range, zone):
    """(UA, UB) (N, 3) fp64: the UTM (east, north, alt) of o + d near and o + d far of fp32 rays, by the oracle's geodetic conversion and
    ``utm_forward_np``."""
    from tests.test_dsm_host import utm_forward_np

    r = np.asarray(rays, np.float64)
    ends = []
    for col in (6, 7):
        lat, lon, alt = O.latlonalt_from_depth(r, r[:, col], np.asarray(center, np.float64), scene_range)
        e, n = utm_forward_np(lat, lon, zone)
        ends.append(np.stack([e, n, alt], 1))
    return ends[0], ends[1]


def altitude_ld(rays, depth, center, scene_range):
    """The altitude of ``latlonalt_from_depth`` (sat_utils.ecef_to_latlon_custom's formulas) in numpy's extended precision: p / cos(lat)
    - N cancels 6.4e6 m down to the altitude, which in fp64 leaves a noise of some 1e-9 m -- above the 1e-9 m the chord test allows."""
    ld = np.longdouble
    r, t = np.asarray(rays, np.float64).astype(ld), np.asarray(depth, np.float64).astype(ld).reshape(-1, 1)
    xyz = (r[:, 0:3] + r[:, 3:6] * t) * ld(scene_range) + np.asarray(center, np.float64).astype(ld)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    a, e = ld(6378137.0), ld(8.1819190842622e-2)
    asq, esq = a * a, e * e
    b = np.sqrt(asq * (1 - esq))
    ep2 = (asq - b * b) / (b * b)
    p = np.sqrt(x * x + y * y)
    th = np.arctan2(a * z, b * p)
    lat = np.arctan2(z + ep2 * b * np.sin(th) ** 3, p - esq * a * np.cos(th) ** 3)
    return p / np.cos(lat) - a / np.sqrt(1 - esq * np.sin(lat) ** 2)


def to_grid(U, xoff, yoff):
    """UTM (east, north, alt) -> grid frame (x, y, z) = (east - xoff, yoff - north, alt)."""
    return np.stack([U[:, 0] - xoff, yoff - U[:, 1], U[:, 2]], 1)


def oblique_rays_np(grid, zone, min_alt, max_alt, center, scene_range, sun_d, off_nadir_deg=35.0, azimuth_deg=70.0):
    """(N, 11) float64 rays, one per cell: each looks at its cell centre at the mean altitude from ``off_nadir_deg`` off the vertical,
    starts at about max_alt + 5 m and ends at about min_alt - 5 m (on the tangent plane of the target)."""
    east, north = R.cell_centres(grid)
    lat, lon = R.utm_inverse_np(east.ravel(), north.ravel(), zone)
    mid = 0.5 * (min_alt + max_alt)
    x, y, z = R.latlon_to_ecef(lat, lon, mid)
    e, n, u = S.tangent_frame(lat, lon)
    t, a = np.radians(off_nadir_deg), np.radians(azimuth_deg)
    look = np.sin(t) * np.sin(a) * e + np.sin(t) * np.cos(a) * n - np.cos(t) * u  # unit, downwards
    back = (max_alt + 5.0 - mid) / np.cos(t)
    rays = np.zeros((lat.size, 11))
    rays[:, 0:3] = (np.stack([x, y, z], 1) - look * back - np.asarray(center)) / scene_range
    rays[:, 3:6] = look
    rays[:, 7] = (max_alt - min_alt + 10.0) / np.cos(t) / scene_range
    rays[:, 8:11] = np.asarray(sun_d, np.float32).astype(np.float64)
    return rays


@functools.lru_cache(maxsize=None)
def scene_rays(name):
    """The fp32 rays cast in the scene frame on ``sun_rays_reference.scene(name)``: its nadir rays, then the oblique ones; read-only."""
    sc = S.scene(name)
    rays = np.concatenate([sc["rays"], oblique_rays_np(**sc["s"]).astype(np.float32)])
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def scene_raster(name):
    """A DSM raster on the scene's own grid: random heights inside the scene's altitude range, about 5 % NaN; fp32, read-only."""
    s = S.scene(name)["s"]
    xsize, ysize = s["grid"][2], s["grid"][3]
    rng = np.random.default_rng(3000 + len(name))
    h = rng.uniform(s["min_alt"] + 4, s["max_alt"] - 4, (ysize, xsize)).astype(np.float32)
    h[rng.random((ysize, xsize)) < 0.05] = np.nan
    h.setflags(write=False)
    return h


# ---- references computed once and shared ------------------------------------------------------------------------------------------------
DELTA, DELTA_SCENE = 1e-6, 1e-5  # metres: the stability perturbations of the grid-frame and of the scene-frame comparisons
SEGMENT_RASTERS = ("37x53", "16x16", "33x17", "1x1")
SUNS = tuple((el, az) for el in (60.0, 25.0, 8.0) for az in (40.0, 140.0))
SHADOW_CASES = tuple([(n, el, az) for n in ("16x16", "33x17", "1x1") for el, az in SUNS]
                     + [("37x53", 60.0, 40.0), ("37x53", 25.0, 140.0), ("37x53", 8.0, 40.0), ("37x53_hole", 8.0, 140.0)])
SCENE_STEP = 3  # every third ray of scene_rays: the brute force is O(rays * cells)


@functools.lru_cache(maxsize=None)
def segment_truth(name):
    """(stable, s, cell) of ``segments(name)`` over ``raster(name)`` at DELTA."""
    return stable_np(raster(name), RES, *segments(name), DELTA)


@functools.lru_cache(maxsize=None)
def shadow_truth(name, elevation, azimuth):
    """(mask, stable) of ``raster(name)`` under the sun at (elevation, azimuth) degrees, bias 0, at DELTA."""
    return shadow_mask_np(raster(name), RES, S.sun_direction(elevation, azimuth), 0.0, DELTA)


@functools.lru_cache(maxsize=None)
def scene_cast_inputs(name):
    """(rays fp32 (n, 11), UA, UB) of the scene-frame comparison: every SCENE_STEP-th ray of ``scene_rays(name)`` and the UTM ends of
    its segment by the all-numpy chain."""
    s = S.scene(name)["s"]
    rays = np.ascontiguousarray(scene_rays(name)[::SCENE_STEP])
    UA, UB = utm_segments_np(rays, s["center"], s["scene_range"], s["zone"])
    return rays, UA, UB


@functools.lru_cache(maxsize=None)
def scene_truth(name):
    """(stable, s, cell) of the all-numpy chain on ``scene_raster(name)`` at DELTA_SCENE."""
    s = S.scene(name)["s"]
    _, UA, UB = scene_cast_inputs(name)
    xoff, yoff = s["grid"][0], s["grid"][1]
    return stable_np(scene_raster(name), s["grid"][4], to_grid(UA, xoff, yoff), to_grid(UB, xoff, yoff), DELTA_SCENE)
