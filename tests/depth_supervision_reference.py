"""numpy restatement of SatelliteDataset_depth's data (datasets/satellite_depth.py:51-129), the yardstick of the HIP path.

Rays: ``oracle.rpc_oracle.get_rays`` at the keypoints, normalised in fp32 with the sun appended.  Depth targets: the tie point cast
to fp32 first, then centred, scaled and measured in fp32 as the reference's tensor ops.  Keypoint weights: every reprojection error
in fp64 (sat_utils.ecef_to_latlon_custom, the RPC00B projection, the pixel distance), rounded to fp32 into an (n_pts, n_cams)
matrix where the last observation of a (point, camera) wins, then -- as the HIP kernels do, and unlike the reference's fp32 sums --
the per-point sum and the mean accumulated in fp64 and rounded once to fp32, and ``exp(-(e / e_mean)^2)`` in fp32.
"""
import numpy as np

from oracle import rpc_oracle as R


def ecef_to_latlon(x, y, z):
    """sat_utils.ecef_to_latlon_custom (sat_utils.py:76-95), fp64."""
    a, e = 6378137.0, 8.1819190842622e-2
    asq, esq = a ** 2, e ** 2
    b = np.sqrt(asq * (1 - esq))
    bsq = b ** 2
    ep = np.sqrt((asq - bsq) / bsq)
    p = np.sqrt(x ** 2 + y ** 2)
    th = np.arctan2(a * z, b * p)
    lon = np.arctan2(y, x)
    lat = np.arctan2(z + ep ** 2 * b * np.sin(th) ** 3, p - esq * a * np.cos(th) ** 3)
    n = a / np.sqrt(1 - esq * np.sin(lat) ** 2)
    alt = p / np.cos(lat) - n
    return lat * 180 / np.pi, lon * 180 / np.pi, alt


def reprojection_errors(rpc, colrow, pts3d):
    """fp64 |colrow - projection(ecef_to_latlon(pts3d))| per row (satellite_depth.py:116-122)."""
    lat, lon, alt = ecef_to_latlon(pts3d[:, 0], pts3d[:, 1], pts3d[:, 2])
    col, row = R.projection(rpc, lon, lat, alt)
    return np.sqrt((colrow[:, 0] - col) ** 2 + (colrow[:, 1] - row) ** 2)


def keypoint_weights(images, pts3d):
    """(errmat (n_pts, n_cams) fp32, e fp32, e_mean fp32, w fp32): fp64 sums rounded once."""
    n_pts, n_cams = pts3d.shape[0], len(images)
    errmat = np.zeros((n_pts, n_cams), np.float32)
    for t, d in enumerate(images):
        cr = np.asarray(d["keypoints"]["2d_coordinates"], np.float64).reshape(-1, 2)
        ix = np.asarray(d["keypoints"]["pts3d_indices"], np.int64)
        if ix.size:
            errmat[ix, t] = reprojection_errors(d["rpc"], cr, pts3d[ix])  # numpy keeps the last of repeated indices
    e64 = np.zeros(n_pts)
    for t in range(n_cams):  # camera order
        e64 += errmat[:, t].astype(np.float64)
    e = e64.astype(np.float32)
    e_mean = np.float32(np.sum(e.astype(np.float64)) / n_pts)
    w = np.exp(-(e / e_mean) ** 2).astype(np.float32)
    return errmat, e, e_mean, w


def rays_at(d, center, scene_range):
    """(K, 11) fp32: get_rays at the keypoints + normalize_rays + sun (satellite_depth.py:64-75)."""
    cr = np.asarray(d["keypoints"]["2d_coordinates"], np.float64).reshape(-1, 2)
    rays = R.get_rays(cr[:, 0], cr[:, 1], d["rpc"], float(d["min_alt"]), float(d["max_alt"]))
    for c in range(3):
        rays[:, c] -= np.float32(center[c])
        rays[:, c] /= np.float32(scene_range)
    rays[:, 6] /= np.float32(scene_range)
    rays[:, 7] /= np.float32(scene_range)
    el, az = np.radians(float(d["sun_elevation"])), np.radians(float(d["sun_azimuth"]))
    sun = np.array([np.sin(az) * np.cos(el), np.cos(az) * np.cos(el), np.sin(el)]).astype(np.float32)
    return np.hstack([rays, np.tile(sun, (rays.shape[0], 1))]).astype(np.float32)


def depth_targets(rays, pts3d_rows, center, scene_range):
    """|(fp32(p) - center) / range - origin| in fp32 (satellite_depth.py:77-88)."""
    p = pts3d_rows.astype(np.float32)
    for c in range(3):
        p[:, c] -= np.float32(center[c])
        p[:, c] /= np.float32(scene_range)
    d = p - rays[:, :3]
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])


def depth_supervision(images, pts3d, center, scene_range):
    """(rays (N, 11), depths (N, 2), ts (N,), e, e_mean, w, errmat) for the training images in order."""
    errmat, e, e_mean, w = keypoint_weights(images, pts3d)
    rays, depths, ts = [], [], []
    for t, d in enumerate(images):
        ix = np.asarray(d["keypoints"]["pts3d_indices"], np.int64)
        if not ix.size:
            continue
        r = rays_at(d, center, scene_range)
        rays.append(r)
        depths.append(np.stack([depth_targets(r, pts3d[ix], center, scene_range), w[ix]], 1))
        ts.append(np.full(ix.size, t, np.int64))
    return np.concatenate(rays), np.concatenate(depths), np.concatenate(ts), e, e_mean, w, errmat


def load_scene(root):
    """(images, pts3d, center fp32 (3,), scene_range fp32) of a dataset directory, as data.load_depth_supervision reads it."""
    import json
    import os

    with open(os.path.join(root, "scene.loc")) as f:
        loc = json.load(f)
    center = np.array([loc["X_offset"], loc["Y_offset"], loc["Z_offset"]], np.float32)
    scene_range = np.float32(max(np.float32(loc["X_scale"]), np.float32(loc["Y_scale"]), np.float32(loc["Z_scale"])))
    with open(os.path.join(root, "train.txt")) as f:
        names = [n for n in f.read().split("\n") if n.strip()]
    images = []
    for n in names:
        with open(os.path.join(root, n)) as f:
            images.append(json.load(f))
    return images, np.load(os.path.join(root, "pts3d.npy")), center, scene_range
