#!/usr/bin/env python3
"""Generate tests/golden/tie_points/reference.npz by RUNNING THE REFERENCE's study_depth_supervision.idw_interpolation and
save_heatmap_of_reprojection_error(..., plot=False) (scipy's cKDTree and ndimage.gaussian_filter underneath).

Runs only in the build container (needs /root/reference, read-only, plus scipy and matplotlib).  The module is imported unmodified;
its absent imports (rpcm, rasterio, torchvision, kornia, PIL where absent) are stubbed as in make_depth_golden.py, and never called.
The neighbour indices cKDTree returns are recorded by a subclass installed as scipy.spatial.cKDTree for the duration of each call.

Cases: three images of the committed scene tests/golden/depth_supervision/ (read-only): their keypoints with the reference's own depth
targets (all_depths[:, 0], the study's call, smooth 1) and reprojection errors (errmat[pts3d_idx, t], the heatmap's default smooth
20); the rasters are kept at the pixels of tie_point_reference.crop_index (corner and central blocks) and the neighbours at 3000
seeded pixels.  Seeded synthetic cases: N in {1, 3, 8} with keypoints exactly on pixels and duplicated keypoints, explicit queries
outside the image, and the heatmap of a 23 x 17 image with keypoints outside it for sigma in {0, 0.5, 1, 3, 20} (radius > image).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_tie_point_golden.py            # rewrite the fixture
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_tie_point_golden.py --check    # regenerate and compare bit for bit
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "tie_points")
SCENE = os.path.join(HERE, "depth_supervision")
REF = "/root/reference"
SCENE_IMAGES = (0, 3, 7)
SIGMAS = (0.0, 0.5, 1.0, 3.0, 20.0)

sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
from make_depth_golden import _has, _Stub, npz_bytes  # noqa: E402


def import_study():
    sys.path.insert(0, REF)
    stubs = {"rpcm": types.ModuleType("rpcm")}
    for m in ("rasterio", "torchvision", "torchvision.transforms", "kornia") + (() if _has("PIL") else ("PIL", "PIL.Image")):
        stubs[m] = _Stub(m)
    for m, v in stubs.items():
        sys.modules.setdefault(m, v)
    import study_depth_supervision as S

    return S


def recorded(fn, *args, **kw):
    """fn(*args, **kw) with every cKDTree.query result recorded: (result, [nn_indices, ...])."""
    import scipy.spatial

    orig, rec = scipy.spatial.cKDTree, []

    class Spy(orig):
        def query(self, *a, **k):
            d, i = super().query(*a, **k)
            rec.append(np.asarray(i).reshape(len(d), -1).astype(np.int32))
            return d, i

    scipy.spatial.cKDTree = Spy
    try:
        return fn(*args, **kw), rec
    finally:
        scipy.spatial.cKDTree = orig


def generate():
    import json

    from tests import tie_point_reference as T

    S = import_study()
    out = {}
    ref = np.load(os.path.join(SCENE, "reference.npz"), allow_pickle=False)
    with open(os.path.join(SCENE, "train.txt")) as f:
        names = [n for n in f.read().split("\n") if n.strip()]
    ids = ref["all_ids"][:, 0]
    for t in SCENE_IMAGES:
        with open(os.path.join(SCENE, names[t])) as f:
            d = json.load(f)
        h, w = int(d["height"]), int(d["width"])
        pts2d = np.array(d["keypoints"]["2d_coordinates"], np.float64)
        depth = ref["all_depths"][ids == t, 0]
        err = ref["errmat"][np.asarray(d["keypoints"]["pts3d_indices"]), t]
        crop = T.crop_index(h, w)
        g = np.random.default_rng(1000 + t)
        sample = np.sort(g.choice(h * w, 3000, replace=False))
        heat, rec = recorded(S.save_heatmap_of_reprojection_error, h, w, pts2d, depth, smooth=1, plot=False)
        err_heat, _ = recorded(S.save_heatmap_of_reprojection_error, h, w, pts2d, err)
        cols, rows = pts2d.T
        valid = np.logical_and(cols < w, cols >= 0) & np.logical_and(rows < h, rows >= 0)
        raw, _ = recorded(S.idw_interpolation, pts2d[valid], depth[valid], T.raster_queries(h, w))
        p = f"scene{t}_"
        out.update({p + "hw": np.array([h, w], np.int64), p + "pts2d": pts2d, p + "depth": depth, p + "err": err, p + "crop": crop,
                    p + "idw_crop": raw[crop], p + "heat_crop": heat.ravel()[crop], p + "err_heat20_crop": err_heat.ravel()[crop],
                    p + "nn_sample": sample, p + "nn": rec[0][sample]})
    g = np.random.default_rng(20261016)
    for N, (h, w), k in ((1, (30, 40), 40), (3, (25, 35), 30), (8, (32, 28), 50)):
        pts = np.stack([g.uniform(0, w - 1, k), g.uniform(0, h - 1, k)], 1)
        pts[: k // 4] = np.stack([g.integers(0, w, k // 4), g.integers(0, h, k // 4)], 1)  # exactly on pixels
        z = g.normal(10.0, 3.0, k).astype(np.float32)
        dup = g.choice(k, 5, replace=False)
        pts, z = np.concatenate([pts, pts[dup]]), np.concatenate([z, z[dup]])  # duplicated keypoints carry the same z
        vals, rec = recorded(S.idw_interpolation, pts, z, T.raster_queries(h, w), N=N)
        out.update({f"syn{N}_hw": np.array([h, w], np.int64), f"syn{N}_pts2d": pts, f"syn{N}_z": z, f"syn{N}_idw": vals, f"syn{N}_nn": rec[0]})
    pts = np.stack([g.uniform(0, 60, 70), g.uniform(0, 45, 70)], 1)
    z = g.normal(0.0, 1.0, 70).astype(np.float32)
    q = np.concatenate([np.stack([g.uniform(-500, 560, 200), g.uniform(-400, 445, 200)], 1),
                        [[-1e5, 3.0], [2e5, -7e4], [30.5, 1e6], [-3e3, -3e3]]])
    vals, rec = recorded(S.idw_interpolation, pts, z, q)
    out.update({"out_pts2d": pts, "out_z": z, "out_query": q, "out_idw": vals, "out_nn": rec[0]})
    h, w = 23, 17
    pts = np.stack([g.uniform(-4, w + 4, 60), g.uniform(-4, h + 4, 60)], 1)  # some outside: the heatmap's valid filter
    vals = g.normal(2.0, 1.0, 60).astype(np.float32)
    out.update({"heat_pts2d": pts, "heat_values": vals})
    for s in SIGMAS:
        heat, _ = recorded(S.save_heatmap_of_reprojection_error, h, w, pts, vals, smooth=s, plot=False)
        out[f"heat_sigma{s:g}"] = heat
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--check", action="store_true", help="write nothing: regenerate and compare bit for bit")
    a = ap.parse_args()
    sys.dont_write_bytecode = True
    ref = generate()
    blob = npz_bytes(ref)
    path = os.path.join(OUT, "reference.npz")
    if a.check:
        z = np.load(path, allow_pickle=False)
        bad = sorted(set(z.files) ^ set(ref))
        for k in sorted(set(z.files) & set(ref)):
            x, y = np.asarray(ref[k]), z[k]
            if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
                bad.append(k)
        same = open(path, "rb").read() == blob
        print(f"tie_points  {'OK: ' + str(len(ref)) + ' arrays bit-equal' if not bad and same else 'MISMATCH: ' + ', '.join(bad or ['file bytes'])}")
        return 1 if bad or not same else 0
    os.makedirs(OUT, exist_ok=True)
    with open(path, "wb") as f:
        f.write(blob)
    print(f"tie_points  reference.npz ({len(blob) / 1024:.0f} KiB), {len(ref)} arrays")
    return 0


if __name__ == "__main__":
    sys.exit(main())
