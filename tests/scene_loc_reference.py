"""numpy restatement of ``SatelliteDataset.init_scaling_params`` (datasets/satellite.py:135-156) for tests and the benchmark's stand-in:
``rpc_oracle.get_rays`` on each image's down-scaled pixel grid, near points o and far points o + far * d in float32, and
``sat_utils.rpc_scaling_params`` (sat_utils.py:30-37) in float32.  TEST INFRASTRUCTURE ONLY."""
import glob
import json
import os
import shutil

import numpy as np

from oracle import rpc_oracle as R

SCENE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_loc")
KEYS = ("X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset")


def load_images(root):
    """(images, paths): every *.json under root, sorted by name."""
    paths = sorted(glob.glob(os.path.join(root, "*.json")))
    images = []
    for p in paths:
        with open(p) as f:
            images.append(json.load(f))
    return images, paths


def image_points(d, img_downscale=1.0, pixels=None):
    """(2 HW, 3) float32: the near then the far points of one image's rays (``pixels``: flat pixel indices to keep, default all)."""
    s = float(img_downscale)
    h, w = int(d["height"] // s), int(d["width"] // s)
    cols, rows = np.meshgrid(np.arange(w), np.arange(h))
    cols, rows = cols.flatten(), rows.flatten()
    if pixels is not None:
        cols, rows = cols[pixels], rows[pixels]
    rpc = {k: (np.asarray(v, np.float64) if isinstance(v, list) else float(v)) for k, v in d["rpc"].items()}
    rays = R.get_rays(cols, rows, R.rescale_rpc(rpc, 1.0 / s), float(d["min_alt"]), float(d["max_alt"]))
    near = rays[:, :3]
    far = rays[:, :3] + rays[:, 7:8] * rays[:, 3:6]  # float32, multiply then add, like the reference's tensor ops (:149-150)
    return np.concatenate([near, far], 0)


def footprint(points):
    """[xmin, xmax, ymin, ymax, zmin, zmax] float32 of (n, 3) points; +inf / -inf for none."""
    if points.shape[0] == 0:
        return np.array([np.inf, -np.inf] * 3, np.float32)
    return np.stack([points.min(0), points.max(0)], 1).reshape(6).astype(np.float32)


def scaling_params(lo, hi):
    """``sat_utils.rpc_scaling_params`` on float32 extremes: (scale, offset), both float32."""
    scale = (np.float32(hi) - np.float32(lo)) / 2
    return np.float32(scale), np.float32(np.float32(lo) + scale)


def scene_bounds(images, img_downscale=1.0):
    """(loc dict of np.float32 under KEYS, per-image footprints (n_images, 6) float32, pixels)."""
    pts = [image_points(d, img_downscale) for d in images]
    per_image = np.stack([footprint(p) for p in pts])
    lo, hi = per_image[:, 0::2].min(0), per_image[:, 1::2].max(0)
    loc = {}
    for a, axis in enumerate("XYZ"):
        loc[axis + "_scale"], loc[axis + "_offset"] = scaling_params(lo[a], hi[a])
    return loc, per_image, sum(p.shape[0] for p in pts) // 2


def expected():
    z = np.load(os.path.join(SCENE, "expected.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def scene_copy(tmp_path, name="scene"):
    root = str(tmp_path / name)
    shutil.copytree(SCENE, root)
    os.remove(os.path.join(root, "expected.npz"))
    return root


def check_against_fixture(loc, exp, tag, lo=None, hi=None):
    """The gate of the GPU fixture test: per axis, min, max and offset within 2 fp32 ulps at that coordinate's magnitude (one for the
    origin's cast where two libms' sin / cos differ -- tests/test_rpc.py's allowance --, one for the rounding of the sum); the scale
    within the same absolute amount."""
    for a, axis in enumerate("XYZ"):
        tol = 2 * np.spacing(np.float32(max(abs(exp["min_" + tag][a]), abs(exp["max_" + tag][a]))))
        if lo is not None:
            assert abs(np.float64(lo[a]) - np.float64(exp["min_" + tag][a])) <= tol, (axis, "min", lo[a], exp["min_" + tag][a])
            assert abs(np.float64(hi[a]) - np.float64(exp["max_" + tag][a])) <= tol, (axis, "max", hi[a], exp["max_" + tag][a])
        assert abs(np.float64(loc[axis + "_offset"]) - np.float64(exp["offset_" + tag][a])) <= tol, (axis, "offset", loc[axis + "_offset"])
        assert abs(np.float64(loc[axis + "_scale"]) - np.float64(exp["scale_" + tag][a])) <= tol, (axis, "scale", loc[axis + "_scale"])
