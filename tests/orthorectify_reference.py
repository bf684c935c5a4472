"""fp64 numpy reference of the orthorectification onto a DSM raster (csrc/orthorectify.hip), built from the
yardsticks the tree already has: ``tests.test_dsm_host.utm_inverse_np`` / ``utm_forward_np``, ``oracle.rpc_oracle.projection`` /
``localization``, the brute-force ``tests.heightfield_reference.cast_np`` / ``stable_np`` (not a walk) and a plain restatement of the
three samplers.

Per cell (j, c) of the raster: empty (status 0) when its height is not finite; else (col, row) = the RPC projection of the cell centre
at its height; outside (3) when that is not finite or outside [0, W-1] x [0, H-1]; else the segment from (centre, h + bias) to the
camera's localisation of (col, row) at the raster's maximum is cast against every column but the cell's own: a hit is occluded (2), a
miss visible (1); a cell with h + bias at or above the maximum is visible without a cast.

It also says which cells are *unstable*, i.e. left out of the status and colour comparisons with the GPU: those whose cast changes
under ``stable_np``'s perturbations (delta = 1e-5 m), those whose (col, row) lies within ``eps_px`` of an image border and, for the
nearest sampler, those whose fractional part lies within ``eps_px`` of 0.5.  tests/test_orthorectify_host.py holds them to 1 %.
"""
import functools

import numpy as np

from oracle import rpc_oracle as RO
from tests import heightfield_reference as H
from tests import ortho_reference as R
from tests.test_dsm_host import utm_forward_np, utm_inverse_np

EMPTY, VISIBLE, OCCLUDED, OUTSIDE = 0, 1, 2, 3
MODES = ("nearest", "bilinear", "bicubic")
DELTA = 1e-5  # metres: stable_np's perturbation
DEG_TOL = 1e-11  # degrees: what tests/test_hip_ortho.py holds sr_utm_to_latlon to


# ---- the three samplers ---------------------------------------------------------------------------------------------------------------
def pixel_values(image):
    """(H, W, C) float64 values of a uint8 (v / 255) or fp32 (v) image, (H, W) gaining a channel."""
    image = np.asarray(image)
    if image.ndim == 2:
        image = image[:, :, None]
    assert image.dtype in (np.uint8, np.float32), image.dtype
    return image.astype(np.float64) / 255.0 if image.dtype == np.uint8 else image.astype(np.float64)


def _tap(values, iy, ix):
    h, w = values.shape[:2]
    return values[np.clip(iy, 0, h - 1), np.clip(ix, 0, w - 1)]  # (N, C): edge replicate


def keys(s):
    """Keys' cubic convolution kernel with a = -0.5 at distance s >= 0."""
    a = -0.5
    inner = ((a + 2.0) * s - (a + 3.0)) * s * s + 1.0
    outer = ((a * s - 5.0 * a) * s + 8.0 * a) * s - 4.0 * a
    return np.where(s <= 1.0, inner, np.where(s < 2.0, outer, 0.0))


def sample_np(image, col, row, mode):
    """(N, C) float64, not yet rounded to fp32: ``image`` at the points (col, row) ((N,) each, inside the image)."""
    v = pixel_values(image)
    col, row = np.asarray(col, np.float64), np.asarray(row, np.float64)
    if mode == "nearest":
        return _tap(v, np.floor(row + 0.5).astype(np.int64), np.floor(col + 0.5).astype(np.int64))
    x0, y0 = np.floor(col), np.floor(row)
    fx, fy = (col - x0)[:, None], (row - y0)[:, None]
    ix, iy = x0.astype(np.int64), y0.astype(np.int64)
    if mode == "bilinear":
        t0 = (1.0 - fx) * _tap(v, iy, ix) + fx * _tap(v, iy, ix + 1)
        t1 = (1.0 - fx) * _tap(v, iy + 1, ix) + fx * _tap(v, iy + 1, ix + 1)
        return t0 * (1.0 - fy) + t1 * fy
    assert mode == "bicubic", mode
    wx = [keys(1.0 + fx), keys(fx), keys(1.0 - fx), keys(2.0 - fx)]
    wy = [keys(1.0 + fy), keys(fy), keys(1.0 - fy), keys(2.0 - fy)]
    acc = np.zeros((col.size, v.shape[2]))
    for m in range(4):
        line = np.zeros_like(acc)
        for k in range(4):
            line = line + wx[k] * _tap(v, iy - 1 + m, ix - 1 + k)
        acc = acc + wy[m] * line
    return acc


# ---- geometry ------------------------------------------------------------------------------------------------------------------------
def project_np(hgt, grid, zone, rpc):
    """(col, row), each (ysize, xsize) float64, NaN for an empty cell: the cell centres at their heights through the camera."""
    hgt = np.asarray(hgt, np.float32)
    ysize, xsize = hgt.shape
    east, north = R.cell_centres((grid[0], grid[1], xsize, ysize, grid[2]))
    lat, lon = utm_inverse_np(east.ravel(), north.ravel(), zone)
    with np.errstate(all="ignore"):
        col, row = RO.projection(rpc, lon, lat, hgt.astype(np.float64).ravel())
    finite = np.isfinite(hgt).ravel()
    return np.where(finite, col, np.nan).reshape(hgt.shape), np.where(finite, row, np.nan).reshape(hgt.shape)


def eps_px(hgt, grid, zone, rpc):
    """The bound on |colrow - reference|: DEG_TOL degrees times the largest partial derivative of (col, row) by (lat, lon) over the
    raster's cells, evaluated by central differences, plus 1e-9 px."""
    hgt = np.asarray(hgt, np.float32)
    ysize, xsize = hgt.shape
    east, north = R.cell_centres((grid[0], grid[1], xsize, ysize, grid[2]))
    lat, lon = utm_inverse_np(east.ravel(), north.ravel(), zone)
    alt = np.where(np.isfinite(hgt), hgt, 0.0).astype(np.float64).ravel()
    step = 1e-6
    worst = 0.0
    for dlat, dlon in ((step, 0.0), (0.0, step)):
        hi, lo = RO.projection(rpc, lon + dlon, lat + dlat, alt), RO.projection(rpc, lon - dlon, lat - dlat, alt)
        worst = max(worst, np.abs((hi[0] - lo[0]) / (2 * step)).max(), np.abs((hi[1] - lo[1]) / (2 * step)).max())
    return DEG_TOL * float(worst) + 1e-9


def sight_segments_np(hgt, grid, zone, rpc, col, row, bias=0.0):
    """(A, B (n, 3) grid-frame metres, idx (n,) = the cells a line of sight is cast for): from the cell centre at h + bias to the
    camera's localisation of (col, row) at the raster's maximum."""
    hgt = np.asarray(hgt, np.float32)
    ysize, xsize = hgt.shape
    h = hgt.astype(np.float64).ravel()
    top = float(H.blockmax_np(hgt)[1])
    c, r = col.ravel(), row.ravel()
    with np.errstate(invalid="ignore"):
        inside = np.isfinite(h) & np.isfinite(c) & np.isfinite(r) & (c >= 0) & (c <= rpc_width(rpc) - 1) & (r >= 0) & (r <= rpc_height(rpc) - 1)
        idx = np.flatnonzero(inside & (h + bias < top))
    jj, cc = np.divmod(idx, xsize)
    res = grid[2]
    A = np.stack([(cc + 0.5) * res, (jj + 0.5) * res, h[idx] + bias], 1)
    if idx.size:
        lon_b, lat_b = RO.localization(rpc, c[idx], r[idx], np.full(idx.size, top))
        e_b, n_b = utm_forward_np(lat_b, lon_b, zone)
        back = RO.projection(rpc, lon_b, lat_b, np.full(idx.size, top))
        # B lies on the pixel's own ray: the localisation stops at a normalised error below 1e-9
        assert max(np.abs(back[0] - c[idx]).max(), np.abs(back[1] - r[idx]).max()) <= 1e-9 * max(abs(rpc["col_scale"]), abs(rpc["row_scale"]))
        B = np.stack([e_b - grid[0], grid[1] - n_b, np.full(idx.size, top)], 1)
    else:
        B = np.zeros((0, 3))
    return A, B, idx, inside


def rpc_width(rpc):
    return int(rpc["_width"])


def rpc_height(rpc):
    return int(rpc["_height"])


def status_np(hgt, grid, zone, rpc, bias=0.0, delta=DELTA):
    """(status (ysize, xsize) uint8, col, row (ysize, xsize) float64, cast_stable (ysize, xsize) bool).  The camera dict carries its
    image size as ``_width`` / ``_height`` (keys ``ops.rpc_buffer`` does not read)."""
    hgt = np.asarray(hgt, np.float32)
    col, row = project_np(hgt, grid, zone, rpc)
    A, B, idx, inside = sight_segments_np(hgt, grid, zone, rpc, col, row, bias)
    status = np.where(np.isfinite(hgt).ravel(), np.where(inside, VISIBLE, OUTSIDE), EMPTY).astype(np.uint8)
    stable = np.ones(hgt.size, bool)
    if idx.size:
        if delta is None:
            cell = H.cast_np(hgt, grid[2], A, B, idx)[1]
        else:
            stable[idx], _, cell = H.stable_np(hgt, grid[2], A, B, delta, idx)
        status[idx] = np.where(cell >= 0, OCCLUDED, VISIBLE)
    return status.reshape(hgt.shape), col, row, stable.reshape(hgt.shape)


def unstable_np(col, row, cast_stable, width, height, eps, nearest=False):
    """The cells left out of status and colour comparisons."""
    with np.errstate(invalid="ignore"):
        border = (np.abs(col) <= eps) | (np.abs(col - (width - 1)) <= eps) | (np.abs(row) <= eps) | (np.abs(row - (height - 1)) <= eps)
        out = ~cast_stable | border
        if nearest:
            out |= (np.abs(col - np.floor(col) - 0.5) <= eps) | (np.abs(row - np.floor(row) - 0.5) <= eps)
    return out


def colors_np(image, status, col, row, mode):
    """(ysize, xsize, C) float64: ``sample_np`` where status is visible, NaN elsewhere."""
    channels = pixel_values(image).shape[2]
    out = np.full(status.shape + (channels,), np.nan)
    vis = status == VISIBLE
    out[vis] = sample_np(image, col[vis], row[vis], mode)
    return out


def mosaic_np(colors32, statuses):
    """(sum float64, count int32, mean float32) of per-view fp32 colours and statuses, accumulated in view order."""
    total = np.zeros(colors32[0].shape, np.float64)
    count = np.zeros(statuses[0].shape, np.int32)
    for c32, st in zip(colors32, statuses):
        vis = st == VISIBLE
        total[vis] = total[vis] + c32[vis].astype(np.float64)
        count[vis] += 1
    with np.errstate(all="ignore"):
        mean = (total / count[:, :, None].astype(np.float64)).astype(np.float32)
    return total, count, mean


# ---- cameras -------------------------------------------------------------------------------------------------------------------------
def metres_per_degree(lat):
    """(per degree of latitude, per degree of longitude) on WGS84 at ``lat`` degrees: the usual series, good to a few metres."""
    p = np.radians(lat)
    return 111132.92 - 559.82 * np.cos(2 * p) + 1.175 * np.cos(4 * p), 111412.84 * np.cos(p) - 93.5 * np.cos(3 * p)


def camera(seed, height, width, xsize, ysize, res, tan_theta, lat0=30.30, lon0=-81.66, span=1.6):
    """``rpc_oracle.synthetic_rpc(seed, height, width)`` re-aimed at a raster of xsize x ysize cells around (lat0, lon0): lat / lon
    scales so that the camera's normalised range [-1, 1] spans ``span`` x the raster's extent (the image itself a little more than the
    raster: part of it falls outside), altitudes normalised by offset 15 m and scale 30 m, and
    col_num[3] such that a point 1 m higher appears ``tan_theta`` metres further east (negative: further west)."""
    rpc = {k: (np.array(v, np.float64) if np.ndim(v) else v) for k, v in RO.synthetic_rpc(seed, height=height, width=width).items()}
    m_lat, m_lon = metres_per_degree(lat0)
    rpc["lat_offset"], rpc["lon_offset"] = float(lat0), float(lon0)
    rpc["lon_scale"] = span * xsize * res / (2.0 / rpc["col_num"][1]) / m_lon
    rpc["lat_scale"] = span * ysize * res / (2.0 / abs(rpc["row_num"][2])) / m_lat
    rpc["alt_offset"], rpc["alt_scale"] = 15.0, 30.0
    rpc["col_num"][3] = tan_theta * rpc["col_num"][1] * rpc["alt_scale"] / (rpc["lon_scale"] * m_lon)
    rpc["_width"], rpc["_height"] = int(width), int(height)
    return rpc


def affine_camera(grid, xsize, ysize, zone, width, height, margin, lean=0.0):
    """A camera with linear numerators and unit denominators whose pixel (c + margin, j + margin) falls on the centre of cell (j, c) at
    altitude 0: the numerators' constant and lat / lon terms are a least-squares fit to ``utm_inverse_np``'s cell centres, which absorbs
    the grid's convergence and the mean residual.  ``lean``: columns per metre of altitude."""
    east, north = R.cell_centres((grid[0], grid[1], xsize, ysize, grid[2]))
    lat, lon = utm_inverse_np(east.ravel(), north.ravel(), zone)
    lat0, lon0 = float(lat.mean()), float(lon.mean())
    m_lat, m_lon = metres_per_degree(lat0)
    lat_scale, lon_scale = max(ysize, 2) * grid[2] / m_lat, max(xsize, 2) * grid[2] / m_lon
    x, y = (lat - lat0) / lat_scale, (lon - lon0) / lon_scale
    jj, cc = np.divmod(np.arange(lat.size), xsize)
    basis = np.stack([np.ones_like(x), y, x], 1)
    if lat.size < 3:  # a raster too small to fit: the plain north-up camera
        fit_c, fit_r = np.array([cc[0] + margin, max(xsize, 2), 0.0]), np.array([jj[0] + margin, 0.0, -max(ysize, 2)])
    else:
        fit_c = np.linalg.lstsq(basis, cc + float(margin), rcond=None)[0]
        fit_r = np.linalg.lstsq(basis, jj + float(margin), rcond=None)[0]
    one = np.zeros(20)
    one[0] = 1.0
    col_num, row_num = np.zeros(20), np.zeros(20)
    col_num[:3], row_num[:3] = fit_c, fit_r
    col_num[3] = lean
    return {"row_num": row_num, "row_den": one.copy(), "col_num": col_num, "col_den": one.copy(), "row_offset": 0.0, "col_offset": 0.0,
            "row_scale": 1.0, "col_scale": 1.0, "lat_offset": lat0, "lon_offset": lon0, "alt_offset": 0.0, "alt_scale": 1.0,
            "lat_scale": lat_scale, "lon_scale": lon_scale, "_width": int(width), "_height": int(height)}


# ---- images ----------------------------------------------------------------------------------------------------------------------------
def image_u8(height, width, channels, seed):
    """A smooth ramp plus noise, uint8 (H, W, C)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    base = 96 + 64 * np.sin(0.31 * xx + 0.1 * seed)[:, :, None] + 48 * np.cos(0.23 * yy)[:, :, None] + 8 * np.arange(channels)
    return np.clip(base + rng.normal(0, 12, (height, width, channels)), 0, 255).astype(np.uint8)


def image_f32(height, width, seed, nan_at=None):
    """A single-channel fp32 image (H, W) of values around 0.5, one pixel NaN."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    img = (0.5 + 0.3 * np.sin(0.4 * xx) * np.cos(0.3 * yy) + rng.normal(0, 0.05, (height, width))).astype(np.float32)
    if nan_at is not None:
        img[nan_at] = np.nan
    return img


# ---- the inputs the host and the GPU tests share --------------------------------------------------------------------------------------
# name -> (raster, (lat0, lon0, zone, letter), (seed, H, W, tan_theta), image kind).  The small rasters take a small lean: their heights
# (2 .. 30 m) are several times their extent, and a lean of 0.3 would carry every cell out of the image; the single cell, which the
# grid's whole-metre placement puts up to a metre from (lat0, lon0), also takes a wider span (a fifth camera value).
CASES = {
    "jax_0.3": ("37x53", (30.30, -81.66, 17, "R"), (1, 29, 37, 0.3), "u8x3"),
    "hole_0.8": ("37x53_hole", (30.30, -81.66, 17, "R"), (2, 29, 37, 0.8), "u8x3"),
    "big_cam": ("33x17", (30.30, -81.66, 17, "R"), (3, 64, 96, -0.3), "f32x1"),
    "four_ch": ("16x16", (30.30, -81.66, 17, "R"), (4, 64, 96, 0.1), "u8x4"),
    "one_cell": ("1x1", (30.30, -81.66, 17, "R"), (5, 29, 37, 0.05, 12.0), "u8x3"),
    "cape_town": ("37x53", (-33.90, 18.40, 34, "H"), (6, 29, 37, -0.3), "f32x1"),
}
SHARE_FLOOR = ("jax_0.3", "hole_0.8")  # each of visible, occluded, outside is at least 10 % of these


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(hgt, grid = (xoff, yoff, res), zone, letter, rpc, image): read-only inputs of one case."""
    raster, (lat0, lon0, zone, letter), (seed, height, width, tan_theta, *span), kind = CASES[name]
    hgt = H.raster(raster)
    ysize, xsize = hgt.shape
    g = R.scene(lat0, lon0, zone, xsize, ysize, res=H.RES)["grid"]
    rpc = camera(seed, height, width, xsize, ysize, H.RES, tan_theta, lat0, lon0, *span)
    if kind == "f32x1":
        image = image_f32(height, width, 100 + seed, nan_at=(height // 2, width // 2))
    else:
        image = image_u8(height, width, int(kind[-1]), 100 + seed)
    image.setflags(write=False)
    return dict(hgt=hgt, grid=(g[0], g[1], g[4]), zone=zone, letter=letter, rpc=rpc, image=image, width=width, height=height)


@functools.lru_cache(maxsize=None)
def truth(name, bias=0.0):
    """dict(status, col, row, cast_stable, eps) of a case: the reference, computed once."""
    c = case(name)
    status, col, row, stable = status_np(c["hgt"], c["grid"], c["zone"], c["rpc"], bias)
    for a in (status, col, row, stable):
        a.setflags(write=False)
    return dict(status=status, col=col, row=row, cast_stable=stable, eps=eps_px(c["hgt"], c["grid"], c["zone"], c["rpc"]))


def unstable(name, nearest=False):
    c, t = case(name), truth(name)
    return unstable_np(t["col"], t["row"], t["cast_stable"], c["width"], c["height"], t["eps"], nearest)


@functools.lru_cache(maxsize=None)
def mosaic_views(n=3):
    """``n`` cameras and uint8 RGB images over the "37x53" raster at Jacksonville, leaning different ways."""
    c = case("jax_0.3")
    ysize, xsize = c["hgt"].shape
    views = []
    for k, (tan_theta, hw) in enumerate(((0.3, (29, 37)), (-0.5, (64, 96)), (0.1, (29, 37)))[:n]):
        views.append((image_u8(hw[0], hw[1], 3, 200 + k), camera(20 + k, hw[0], hw[1], xsize, ysize, H.RES, tan_theta)))
    return tuple(views)


# ---- hand-built cases ---------------------------------------------------------------------------------------------------------------------
def hand_grid(xsize, ysize, res=H.RES):
    g = R.scene(30.30, -81.66, 17, xsize, ysize, res=res)["grid"]
    return (g[0], g[1], g[4])


TOWER_SHAPE, TOWER_AT, TOWER_GROUND, TOWER_HEIGHT, TOWER_TAN = (5, 31), (2, 15), 2.0, 6.0, 0.8


def tower_case():
    """A flat raster with one tower under an affine camera standing in the east (a higher point appears further west, by TOWER_TAN
    metres per metre): (hgt, grid, zone, rpc)."""
    ysize, xsize = TOWER_SHAPE
    hgt = np.full(TOWER_SHAPE, TOWER_GROUND, np.float32)
    hgt[TOWER_AT] = TOWER_GROUND + TOWER_HEIGHT
    grid = hand_grid(xsize, ysize)
    lean = -TOWER_TAN / grid[2]  # columns per metre of altitude: one column is one cell
    return hgt, grid, 17, affine_camera(grid, xsize, ysize, 17, xsize + 40, ysize + 40, 20, lean=lean)


def check_tower(status):
    """The tower hides the cells west of it in its own row over TOWER_HEIGHT * TOWER_TAN metres, to within a cell, and nothing else."""
    j, c = TOWER_AT
    occ = status == OCCLUDED
    assert not np.delete(occ, j, axis=0).any() and not occ[j, c:].any()
    run = np.flatnonzero(occ[j])
    assert run.size and run.max() == c - 1 and (np.diff(run) == 1).all()  # contiguous, from the tower's foot
    assert abs(run.size - TOWER_HEIGHT * TOWER_TAN / H.RES) <= 1.0, run.size
    assert status[j, c] == VISIBLE  # the global maximum
    assert ((status == VISIBLE) | occ).all()


def grid_camera_case(xsize=13, ysize=9, margin=2):
    """A flat raster under the affine camera whose pixel (c + margin, j + margin) is the centre of cell (j, c), and an image that is a
    function of (col, row): (hgt, grid, zone, rpc, image uint8 (H, W, 3)).  The nearest sampler must give image[j + margin, c + margin]."""
    hgt = np.full((ysize, xsize), 7.0, np.float32)
    grid = hand_grid(xsize, ysize)
    width, height = xsize + 2 * margin, ysize + 2 * margin
    rpc = affine_camera(grid, xsize, ysize, 17, width, height, margin)
    yy, xx = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    image = np.stack([(7 * xx + 3 * yy) % 256, (5 * yy + xx) % 256, (xx * yy) % 256], 2).astype(np.uint8)
    return hgt, grid, 17, rpc, image
