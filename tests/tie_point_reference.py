"""numpy restatement of study_depth_supervision.py's interpolation (:18-103), the yardstick of csrc/tie_points.hip.  No scipy.

kNN by brute force: fp64 d^2 = dx*dx + dy*dy to every keypoint, the N smallest in (d^2, index) order.  IDW: ``z`` of the nearest when
N == 1 or its distance is < 1e-10, else w_i = 1 / d_i normalised by their sum and sum(w_i z_i), each sum in increasing distance.
Gaussian: scipy.ndimage.gaussian_filter's taps (``_gaussian_kernel1d``), reflect borders via ``np.pad(mode="symmetric")``, axis 0
then axis 1, each output summed as correlate1d does for a symmetric kernel (centre first, then the pairs from the outermost in).
"""
import numpy as np


def raster_queries(h, w):
    """Every pixel (col, row) in row-major order (:30-31)."""
    cols, rows = np.meshgrid(np.arange(w), np.arange(h))
    return np.vstack([cols.ravel(), rows.ravel()]).T.astype(np.float64)


def knn(pts, query, N, chunk=2048):
    """(idx (Q, N) int32, d2 (Q, N) fp64) of the N nearest keypoints of each query, in (d^2, index) order."""
    pts, query = np.asarray(pts, np.float64).reshape(-1, 2), np.asarray(query, np.float64).reshape(-1, 2)
    K, Q = pts.shape[0], query.shape[0]
    assert 1 <= N <= K
    out_i, out_d = np.empty((Q, N), np.int32), np.empty((Q, N))
    for a in range(0, Q, chunk):
        q = query[a:a + chunk]
        dx, dy = q[:, :1] - pts[None, :, 0], q[:, 1:] - pts[None, :, 1]
        d2 = dx * dx + dy * dy
        if N < K:  # everything below the N-th smallest value, then the lowest indices at that value
            t = np.partition(d2, N - 1, axis=1)[:, N - 1:N]
            lt, eq = d2 < t, d2 == t
            sel = lt | (eq & (np.cumsum(eq, axis=1) <= N - lt.sum(1, keepdims=True)))
        else:
            sel = np.ones_like(d2, dtype=bool)
        cols = np.nonzero(sel)[1].reshape(-1, N)  # ascending index in each row
        dsel = np.take_along_axis(d2, cols, 1)
        order = np.argsort(dsel, axis=1, kind="stable")
        out_i[a:a + q.shape[0]] = np.take_along_axis(cols, order, 1)
        out_d[a:a + q.shape[0]] = np.take_along_axis(dsel, order, 1)
    return out_i, out_d


def idw_values(z, idx, d2):
    """The IDW value of each query from its neighbours (idx, d2) in increasing distance."""
    zn = np.asarray(z, np.float32).astype(np.float64)[idx]
    if idx.shape[1] == 1:
        return zn[:, 0].copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / np.sqrt(d2)
        s = np.zeros(idx.shape[0])
        for j in range(idx.shape[1]):
            s = s + inv[:, j]
        acc = np.zeros(idx.shape[0])
        for j in range(idx.shape[1]):
            acc = acc + (inv[:, j] / s) * zn[:, j]
    hit = np.sqrt(d2[:, 0]) < 1e-10
    acc[hit] = zn[hit, 0]
    return acc


def idw_interpolation(pts2d, z, query, N=8):
    """(values (Q,) fp64, idx (Q, N) int32)."""
    idx, d2 = knn(pts2d, query, N)
    return idw_values(z, idx, d2), idx


def gaussian_taps(sigma, truncate=4.0):
    """scipy's reversed _gaussian_kernel1d(sigma, 0, int(truncate * sigma + 0.5)), or None when sigma <= 1e-15."""
    sd = float(sigma)
    if sd <= 1e-15:
        return None
    radius = int(truncate * sd + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    return (phi / phi.sum())[::-1].copy()


def filter_axis(x, taps, axis):
    r = taps.size // 2
    xm = np.moveaxis(np.asarray(x, np.float64), axis, -1)
    n = xm.shape[-1]
    xp = np.pad(xm, [(0, 0)] * (xm.ndim - 1) + [(r, r)], mode="symmetric")
    out = xp[..., r:r + n] * taps[r]
    for k in range(r, 0, -1):
        out = out + (xp[..., r - k:r - k + n] + xp[..., r + k:r + k + n]) * taps[r + k]
    return np.moveaxis(out, -1, axis)


def gaussian_filter(image, sigma, truncate=4.0):
    """scipy.ndimage.gaussian_filter(image, sigma, truncate=truncate), mode "reflect", fp64."""
    out = np.asarray(image, np.float64).copy()
    sig = list(sigma) if isinstance(sigma, (list, tuple)) else [sigma] * out.ndim
    for axis, s in enumerate(sig):
        taps = gaussian_taps(s, truncate)
        if taps is not None:
            out = filter_axis(out, taps, axis)
    return out


def interpolate_tie_points(h, w, pts2d, values, smooth=20, N=8):
    """save_heatmap_of_reprojection_error(h, w, pts2d, values, smooth, plot=False): (raster (h, w), IDW before smoothing (h, w),
    neighbour indices (h w, N) into the VALID keypoints, the valid mask)."""
    pts2d = np.asarray(pts2d, np.float64).reshape(-1, 2)
    cols, rows = pts2d.T
    valid = np.logical_and(cols < w, cols >= 0) & np.logical_and(rows < h, rows >= 0)
    vals, idx = idw_interpolation(pts2d[valid], np.asarray(values, np.float32)[valid], raster_queries(h, w), N)
    raw = vals.reshape(h, w)
    return gaussian_filter(raw, smooth), raw, idx, valid


def crop_index(h, w, c=16):
    """Flat row-major indices of the 4 corner blocks and the central block (c x c, clipped) of an h x w raster: the pixels the
    fixture keeps of each large raster, every border included."""
    rows, cols = [], []
    for r0 in (0, max(h - c, 0), max((h - c) // 2, 0)):
        for c0 in (0, max(w - c, 0), max((w - c) // 2, 0)):
            rr, cc = np.meshgrid(np.arange(r0, min(r0 + c, h)), np.arange(c0, min(c0 + c, w)), indexing="ij")
            rows.append(rr.ravel()), cols.append(cc.ravel())
    flat = np.concatenate(rows) * w + np.concatenate(cols)
    return np.unique(flat)
