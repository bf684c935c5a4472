"""A vectorised fp64 numpy restatement of csrc/cloud_grid.hip (include/satrender.h, sr_cloud_grid): both cell
rules and the four modes.  tests/test_cloud_grid_host.py pins it to the fixtures the reference's project_cloud_into_utm_grid wrote
(rule "nearest") and to rasterize_np (rule "floor"); tests/test_hip_cloud_grid.py uses it on inputs no fixture covers."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cloud_grid")
FIXTURES = ("ties", "city", "counts", "metric")
MODES = ("min", "max", "avg", "med")


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def map_size(bb, definition):
    """(map_w, map_h) as eval_s2p.py:180-182 sizes the map (Python's round)."""
    return int(round((bb[1] - bb[0]) / definition)) + 1, int(round((bb[3] - bb[2]) / definition)) + 1


def cells_np(east, north, alt, x0, y0, d, map_w, map_h, rule):
    """(kept, cell): which points count, and the flat OUTPUT cell (row-major, row 0 north) of those that do."""
    ok = np.isfinite(east) & np.isfinite(north) & np.isfinite(alt)
    e, n = np.where(ok, east, 0.0), np.where(ok, north, 0.0)
    if rule == "nearest":
        c, r = np.round((e - x0) / d), np.round((n - y0) / d)
    elif rule == "floor":
        c, r = np.floor((e - x0) / d), np.floor((y0 - n) / d)
    else:
        raise ValueError(rule)
    ok &= (c >= 0) & (c < map_w) & (r >= 0) & (r < map_h)
    c, r = c[ok].astype(np.int64), r[ok].astype(np.int64)
    row = map_h - 1 - r if rule == "nearest" else r
    return ok, row * map_w + c


def segments_np(east, north, alt, x0, y0, d, map_w, map_h, rule):
    """(z, start, count): the kept altitudes sorted by (cell, altitude), and every cell's segment in them."""
    ok, cell = cells_np(east, north, alt, x0, y0, d, map_w, map_h, rule)
    z = alt[ok]
    order = np.lexsort((z, cell))
    count = np.bincount(cell, minlength=map_w * map_h)
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    return z[order], start, count


def cloud_grid_np(east, north, alt, x0, y0, d, map_w, map_h, rule="nearest", mode="med"):
    """(out, count): (map_h, map_w) fp64 raster (NaN where no point landed) and int32 points per cell."""
    z, start, count = segments_np(east, north, alt, x0, y0, d, map_w, map_h, rule)
    out = np.full(map_w * map_h, np.nan)
    has = count > 0
    s, c = start[has], count[has]
    if mode == "min":
        out[has] = z[s]
    elif mode == "max":
        out[has] = z[s + c - 1]
    elif mode == "med":
        out[has] = (z[s + (c - 1) // 2] + z[s + c // 2]) / 2  # an odd count gives (a + a) / 2 = a
    elif mode == "avg":
        out[has] = np.add.reduceat(z, s) / c
    else:
        raise ValueError(mode)
    return out.reshape(map_h, map_w), count.reshape(map_h, map_w).astype(np.int32)


def avg_bound_np(east, north, alt, x0, y0, d, map_w, map_h, rule="nearest"):
    """Per cell (2 n + 2) 2^-53 max|z| over its n altitudes: two fp64 summations of n terms in different orders, plus two divisions."""
    z, start, count = segments_np(east, north, alt, x0, y0, d, map_w, map_h, rule)
    top = np.zeros(map_w * map_h)
    has = count > 0
    top[has] = np.maximum.reduceat(np.abs(z), start[has])
    return ((2 * count + 2) * 2.0**-53 * top).reshape(map_h, map_w)


def same_bits(a, b):
    """fp64 rasters equal bit for bit over every cell, NaN cells in the same places."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != np.float64 or b.dtype != np.float64:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a[~na].view(np.uint64) == b[~nb].view(np.uint64)).all())
