"""Tie-point interpolation timings (HIP events, median of 10 after a warm-up): the IDW raster (grid build +
query kernel) at 1 Mpx x 10 k and 4 Mpx x 100 k keypoints, uniform and clustered, with the mean and maximum number of keypoints each
query examined; the clustered case also with explicit queries far outside the keypoints' box (the worst case of the grid); the
Gaussian at smooth 1 and 20 on 4 Mpx; one 2048^2 image end to end, split into rays, IDW, smoothing and DSM.  The reference's cKDTree +
gaussian_filter on one CPU core is timed as a LABELLED STAND-IN when scipy is importable, else the numpy restatement (tests/
tie_point_reference.py) at a reduced size.
Usage: bench_tie_point_dsm.py [--no-cpu]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import rpc_oracle as R  # noqa: E402
from satnerf_amd import data, dsm, ops, tie_points  # noqa: E402

dev = "cuda:0"


def timed(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    return float(np.median(t))


def keypoints(k, side, clustered, seed=0):
    g = np.random.default_rng(seed)
    if not clustered:
        return np.stack([g.uniform(0, side - 1, k), g.uniform(0, side - 1, k)], 1)
    centres = g.uniform(0.1 * side, 0.9 * side, (64, 2))  # 64 Gaussian blobs of sigma 1 % of the side
    return np.clip(centres[g.integers(0, 64, k)] + g.normal(0.0, 0.01 * side, (k, 2)), 0, side - 1)


def idw_rows():
    for side, k in ((1024, 10_000), (2048, 100_000)):
        for clustered in (False, True):
            pts = torch.from_numpy(keypoints(k, side, clustered)).to(dev)
            z = torch.rand(k, device=dev)
            scratch = torch.empty(ops.idw_grid_scratch(k, 8), dtype=torch.uint8, device=dev)
            out = torch.empty(side * side, dtype=torch.float64, device=dev)
            ms = timed(lambda: ops.idw_interpolate(pts, z, 8, height=side, width=side, out=out, scratch=scratch))
            _, seen = ops.idw_interpolate(pts, z, 8, height=side, width=side, want_visited=True)
            s = seen.double()
            print(f"IDW raster {side}x{side} px, {k} keypoints {'clustered' if clustered else 'uniform'}, N 8: {ms:.3f} ms; keypoints examined "
                  f"per query mean {s.mean().item():.1f}, max {int(s.max().item())} (of {k})", flush=True)
            if clustered:
                g = np.random.default_rng(1)
                far = torch.from_numpy(np.stack([g.uniform(-side, 2 * side, side * side // 64), g.uniform(-side, 2 * side, side * side // 64)],
                                                1)).to(dev)
                ms = timed(lambda: ops.idw_interpolate(pts, z, 8, query=far, scratch=scratch))
                _, seen = ops.idw_interpolate(pts, z, 8, query=far, want_visited=True)
                s = seen.double()
                print(f"  {far.shape[0]} explicit queries over 3x the keypoints' box: {ms:.3f} ms; examined mean {s.mean().item():.1f}, "
                      f"max {int(s.max().item())}", flush=True)


def gaussian_rows(side=2048):
    img = torch.rand(side, side, dtype=torch.float64, device=dev)
    for smooth in (1, 20):
        ms = timed(lambda: tie_points.gaussian_filter(img, smooth))
        print(f"Gaussian {side}x{side} fp64, smooth {smooth} (radius {int(4 * smooth + 0.5)}): {ms:.3f} ms", flush=True)


def one_image(side=2048, k=20_000):
    """One image end to end: rays of all pixels, IDW of the keypoint depths, smoothing 1, DSM on the cloud's grid."""
    rpc = R.synthetic_rpc(7, height=side, width=side)
    g = np.random.default_rng(3)
    pts = torch.from_numpy(np.stack([g.uniform(0, side - 1, k), g.uniform(0, side - 1, k)], 1)).to(dev)
    z = (1.0 + 0.01 * torch.rand(k, device=dev)).float()
    center, rng = [796912.4, -5453871.2, 3200310.9], 400.0
    t_rays = timed(lambda: data.rays_from_rpc(rpc, side, side, -30.0, 70.0, center, rng, 50.0, 150.0, device=dev))
    rays = data.rays_from_rpc(rpc, side, side, -30.0, 70.0, center, rng, 50.0, 150.0, device=dev)
    t_idw = timed(lambda: ops.idw_interpolate(pts, z, 8, height=side, width=side))
    raw = ops.idw_interpolate(pts, z, 8, height=side, width=side).view(side, side)
    t_g = timed(lambda: tie_points.gaussian_filter(raw, 1))
    depth = tie_points.gaussian_filter(raw, 1).float().reshape(-1)
    t_dsm = timed(lambda: dsm.dsm_from_depth(rays, depth, center, rng))
    print(f"one {side}x{side} image, {k} keypoints: rays {t_rays:.2f} ms, IDW {t_idw:.3f} ms, smoothing {t_g:.3f} ms, DSM {t_dsm:.2f} ms",
          flush=True)


def cpu_stand_in():
    try:
        from scipy.ndimage import gaussian_filter
        from scipy.spatial import cKDTree
    except ImportError:
        from tests import tie_point_reference as T

        side, k = 256, 2000
        pts = keypoints(k, side, False)
        t0 = time.perf_counter()
        raw, _ = T.idw_interpolation(pts, np.random.rand(k).astype(np.float32), T.raster_queries(side, side))
        T.gaussian_filter(raw.reshape(side, side), 1)
        print(f"  stand-in (numpy restatement, {side}x{side} px x {k} keypoints, one CPU core, not the reference): "
              f"{1e3 * (time.perf_counter() - t0):.0f} ms", flush=True)
        return
    side, k = 1024, 10_000
    pts = keypoints(k, side, False)
    q = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2).astype(np.float64)
    t0 = time.perf_counter()
    d, i = cKDTree(pts).query(q, k=8)
    t1 = time.perf_counter()
    gaussian_filter(np.random.rand(side, side), 1)
    t2 = time.perf_counter()
    print(f"  stand-in (scipy cKDTree k=8 + gaussian_filter, {side}x{side} px x {k} keypoints, one CPU core): kNN {1e3 * (t1 - t0):.0f} ms, "
          f"Gaussian {1e3 * (t2 - t1):.0f} ms", flush=True)


def main():
    print("device:", torch.cuda.get_device_name(0))
    idw_rows()
    gaussian_rows()
    one_image()
    if "--no-cpu" not in sys.argv:
        os.environ.setdefault("OMP_NUM_THREADS", "1")
        cpu_stand_in()


if __name__ == "__main__":
    main()
