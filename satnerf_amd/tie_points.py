"""Tie-point interpolation and tie-point DSMs on the GPU: ``study_depth_supervision.py`` without scipy,
plyflatten or GDAL.

``idw_interpolation`` (:64-103; scipy's cKDTree there) and ``gaussian_filter`` (``scipy.ndimage.gaussian_filter``, mode "reflect") are
the two numeric steps, both HIP kernels of csrc/tie_points.hip.  ``interpolate_tie_points`` is ``save_heatmap_of_reprojection_error(...,
plot=False)`` (:18-61): keypoints inside the image, IDW over every pixel, smoothing.  ``tie_point_dsms`` and
``tie_point_dsms_from_keypoints`` are ``check_depth_supervision_points`` (:105-203) without file I/O: per training image the tie-point
depth targets interpolated over every pixel, smoothed, and turned into a DSM by ``dsm.dsm_from_depth`` -- rasterised on the ROI grid
when ``roi`` is given (the reference crops its GeoTIFF with gdal instead), on the cloud's own grid otherwise.  The MAE against a
ground truth is ``dsm.dsm_mae``::

    dsms = tie_point_dsms(root_dir, roi=np.loadtxt(f"{gt_dir}/{aoi_id}_DSM.txt"))
    mae, err, rdsm, shift = dsm.dsm_mae(dsms[0], gt_dsm, gt_mask, register="z")   # "xyz": dsmr's XY + Z registration

Departures: fewer than N keypoints inside an image, an empty image, a negative or non-finite sigma and a Gaussian radius above
``MAX_RADIUS`` raise ``ValueError`` (the reference raises IndexError, or fails inside scipy); exact distance ties at the N-th
neighbour go to the lower keypoint index (cKDTree's order on ties is unspecified).
"""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch

from . import ops

MAX_RADIUS = 200  # Gaussian taps per side (csrc/tie_points.hip kMaxRadius): sigma up to 49.9 at truncate 4


def _gpu(t, name):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{name} must be a GPU tensor: satnerf_amd has no CPU path")
    return t


def _points(pts2d, z, N):
    pts = _gpu(pts2d, "pts2d").double().contiguous()
    z = _gpu(z, "z")
    if pts.dim() != 2 or pts.shape[1] != 2 or z.dim() != 1 or z.shape[0] != pts.shape[0]:
        raise ValueError(f"pts2d must be (K, 2) = (col, row) and z (K,), got {tuple(pts2d.shape)} and {tuple(z.shape)}")
    if z.dtype != torch.float32:
        raise ValueError(f"z must be float32 (the reference's depths and reprojection errors are; got {z.dtype})")
    if not (isinstance(N, numbers.Integral) and 1 <= N <= 32):
        raise ValueError(f"N must be an integer in 1..32, got {N!r}")
    if pts.shape[0] < N:
        raise ValueError(f"{pts.shape[0]} keypoints, but N = {N} nearest neighbours are needed")
    if not bool(torch.isfinite(pts).all()):
        raise ValueError("pts2d must be finite")
    return pts, z.contiguous()


def idw_interpolation(pts2d, z, pts2d_query, N=8, return_indices=False):
    """``study_depth_supervision.idw_interpolation`` (:64-103) on the GPU: the value at each (col, row) row of ``pts2d_query`` (Q, 2)
    from its N nearest of the K keypoints ``pts2d`` (K, 2) carrying ``z`` (K,) fp32 -- the N nearest exactly, by fp64 distance,
    ties to the lower index; ``z`` of the nearest when N == 1 or the nearest lies closer than 1e-10, else the inverse-distance
    weighted mean in fp64.  Returns (Q,) fp64, and with ``return_indices`` also the (Q, N) int32 neighbour indices nearest first."""
    pts, z = _points(pts2d, z, N)
    q = _gpu(pts2d_query, "pts2d_query").double().contiguous()
    if q.dim() != 2 or q.shape[1] != 2:
        raise ValueError(f"pts2d_query must be (Q, 2), got {tuple(pts2d_query.shape)}")
    return ops.idw_interpolate(pts, z, N, query=q, want_indices=return_indices)


def _taps(sigma, truncate):
    """scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, radius)[::-1] as gaussian_filter1d builds it, or None for sigma <= 1e-15."""
    sd, tr = float(sigma), float(truncate)
    if not (math.isfinite(sd) and sd >= 0 and math.isfinite(tr) and tr >= 0):
        raise ValueError(f"sigma and truncate must be finite and >= 0, got {sigma!r} and {truncate!r}")
    if sd <= 1e-15:
        return None
    radius = int(tr * sd + 0.5)
    if radius > MAX_RADIUS:
        raise ValueError(f"the Gaussian radius int({tr} * {sd} + 0.5) = {radius} exceeds MAX_RADIUS = {MAX_RADIUS}")
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    return (phi / phi.sum())[::-1].copy()


def gaussian_filter(image, sigma, truncate=4.0):
    """``scipy.ndimage.gaussian_filter(image, sigma, truncate=truncate)`` with mode "reflect" on a (H, W) GPU raster: fp64 out.
    ``sigma`` is one value or one per axis; an axis with sigma <= 1e-15 is left as it is."""
    img = _gpu(image, "image")
    if img.dim() != 2 or img.numel() == 0:
        raise ValueError(f"image must be a non-empty (H, W) raster, got {tuple(img.shape)}")
    sig = list(sigma) if isinstance(sigma, (list, tuple, np.ndarray)) else [sigma, sigma]
    if len(sig) != 2:
        raise ValueError(f"sigma must be one value or two, got {sigma!r}")
    img = img.double().contiguous()
    taps = [_taps(s, truncate) for s in sig]
    t0, t1 = (None if t is None else torch.from_numpy(t).to(img.device) for t in taps)
    return ops.gaussian_filter_f64(img, t0, t1)


def interpolate_tie_points(height, width, pts2d, values, smooth=20, N=8, name="the image"):
    """``save_heatmap_of_reprojection_error(height, width, pts2d, values, smooth, plot=False)`` (:18-61): the (height, width) fp64
    raster of the fp32 ``values`` of the keypoints with 0 <= col < width and 0 <= row < height, IDW-interpolated at every pixel and
    smoothed with ``gaussian_filter(., smooth)``.  ``name`` labels the image in errors."""
    h, w = int(height), int(width)
    if h < 1 or w < 1:
        raise ValueError(f"{name} is empty ({h} x {w})")
    pts = _gpu(pts2d, "pts2d").double()
    values = _gpu(values, "values")
    if pts.dim() != 2 or pts.shape[1] != 2 or values.dim() != 1 or values.shape[0] != pts.shape[0]:
        raise ValueError(f"pts2d must be (K, 2) and values (K,), got {tuple(pts.shape)} and {tuple(values.shape)}")
    cols, rows = pts[:, 0], pts[:, 1]
    valid = (cols < w) & (cols >= 0) & (rows < h) & (rows >= 0)
    pts, values = pts[valid], values[valid]
    if pts.shape[0] < N:
        raise ValueError(f"{name}: {pts.shape[0]} keypoints lie inside the {h} x {w} image, N = {N} are needed")
    pts, z = _points(pts, values, N)
    raster = ops.idw_interpolate(pts, z, N, height=h, width=w).view(h, w)
    return gaussian_filter(raster, smooth)


def tie_point_dsms_from_keypoints(images, tie_points, center, scene_range, roi=None, smooth=1, N=8, device="cuda", names=None,
                                  return_depths=False):
    """``check_depth_supervision_points`` (:105-203) on in-memory training JSON dicts (as ``data.depth_supervision_from_keypoints``
    takes them, each also with ``height`` and ``width``): one ``dsm.DSM`` per image in order.  The depth targets come from
    ``data.depth_supervision_from_keypoints``; per image they are interpolated (``interpolate_tie_points``, ``smooth`` = 1 as the
    study), cast to fp32 and rasterised with the rays of all pixels (``data.rays_from_rpc``) by ``dsm.dsm_from_depth(..., roi=roi)``.
    ``return_depths`` also returns the (h, w) fp32 depth rasters."""
    from . import data, dsm

    dev = torch.device(device)
    _, depths, _ = data.depth_supervision_from_keypoints(images, tie_points, center, scene_range, device=dev, names=names)
    out, rasters, off = [], [], 0
    for t, d in enumerate(images):
        name = names[t] if names is not None else f"image {t}"
        cr = np.asarray(d["keypoints"]["2d_coordinates"], dtype=np.float64).reshape(-1, 2)
        k = cr.shape[0]
        h, w = int(d["height"]), int(d["width"])
        with torch.cuda.device(dev):
            raster = interpolate_tie_points(h, w, torch.from_numpy(cr).to(dev), depths[off:off + k, 0].contiguous(), smooth=smooth, N=N,
                                            name=name)
            depth = raster.float()
            rays = data.rays_from_rpc(d["rpc"], h, w, float(d["min_alt"]), float(d["max_alt"]), center, scene_range,
                                      float(d["sun_elevation"]), float(d["sun_azimuth"]), device=dev)
            out.append(dsm.dsm_from_depth(rays, depth.reshape(-1), center, scene_range, roi=roi))
        rasters.append(depth)
        off += k
    return (out, rasters) if return_depths else out


def tie_point_dsms(root_dir, roi=None, smooth=1, N=8, device="cuda", return_depths=False):
    """``check_depth_supervision_points`` on the dataset under ``root_dir`` (``scene.loc``, ``train.txt``, the JSONs, ``pts3d.npy``; read
    by ``data.read_depth_dataset``): one ``dsm.DSM`` per training image in ``train.txt`` order (see
    ``tie_point_dsms_from_keypoints``)."""
    from . import data

    images, tie_points, center, scene_range, json_files = data.read_depth_dataset(root_dir)
    return tie_point_dsms_from_keypoints(images, tie_points, center, scene_range, roi=roi, smooth=smooth, N=N, device=device,
                                         names=json_files, return_depths=return_depths)
