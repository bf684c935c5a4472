"""Depth-supervision data timings (HIP events, median of 10 after a warm-up): the kernels alone (per image
sr_rpc_rays_at + sr_reprojection_errors, then sr_keypoint_weights and sr_tie_point_depths) and depth_supervision_from_keypoints end
to end (host parsing, the one upload, the kernels and the e_mean readback), over synthetic scenes of 20 images with ~100 k and ~1 M
observations.  The reference cannot run without rpcm: as a LABELLED STAND-IN, the numpy restatement (tests/
depth_supervision_reference.py, fp64 localisation + projection, single-threaded numpy) is timed once on the ~100 k scene.
Usage: bench_depth_supervision.py [--no-numpy]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import rpc_oracle as R  # noqa: E402
from satnerf_amd import data, ops  # noqa: E402

dev = "cuda:0"


def scene(n_obs, n_img=20, seed=0):
    """n_img images, each seeing n_obs / n_img of n_obs / 8 tie points (so ~2.5 images per point), keypoints = projection + 0.3 px."""
    g = np.random.default_rng(seed)
    n_pts, k = n_obs // 8, n_obs // n_img
    lat = 30.30 + g.uniform(-0.5, 0.5, n_pts) * 0.0035
    lon = -81.66 + g.uniform(-0.5, 0.5, n_pts) * 0.0040
    alt = g.uniform(-15.0, 45.0, n_pts)
    pts3d = np.stack(R.latlon_to_ecef(lat, lon, alt), 1)
    images = []
    for t in range(n_img):
        rpc = R.synthetic_rpc(300 + t, height=2048, width=2048)
        idx = g.choice(n_pts, k, replace=False)
        col, row = R.projection(rpc, lon[idx], lat[idx], alt[idx])
        cr = np.stack([col, row], 1) + g.normal(0.0, 0.3, (k, 2))
        images.append({"rpc": {a: (v.tolist() if isinstance(v, np.ndarray) else v) for a, v in rpc.items()}, "min_alt": -30.0,
                       "max_alt": 70.0, "sun_elevation": 50.0, "sun_azimuth": 150.0,
                       "keypoints": {"2d_coordinates": cr.tolist(), "pts3d_indices": idx.tolist()}})
    center = torch.tensor(pts3d.mean(0).tolist())
    return images, pts3d, center, 400.0


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


def kernels_alone(images, pts3d, center, rng):
    """Device-resident inputs; returns (ms rays + errors over all images, ms weights, ms depths)."""
    colrow = [torch.from_numpy(np.asarray(d["keypoints"]["2d_coordinates"], np.float64)).to(dev) for d in images]
    idx = [torch.tensor(d["keypoints"]["pts3d_indices"], dtype=torch.int64, device=dev) for d in images]
    p = torch.from_numpy(pts3d).to(dev)
    n = sum(c.shape[0] for c in colrow)
    rays = torch.empty(n, 11, device=dev)
    err = torch.empty(n, device=dev)
    offs = np.cumsum([0] + [c.shape[0] for c in colrow])

    def per_image():
        for t, d in enumerate(images):
            sl = slice(int(offs[t]), int(offs[t + 1]))
            ops.rpc_rays_at(d["rpc"], colrow[t], d["min_alt"], d["max_alt"], center, rng, d["sun_elevation"], d["sun_azimuth"], out=rays[sl])
            ops.reprojection_errors(d["rpc"], colrow[t], idx[t], p, out=err[sl])

    all_idx = torch.cat(idx)
    ts = torch.repeat_interleave(torch.arange(len(images), device=dev), torch.tensor([c.shape[0] for c in colrow], device=dev))
    scratch = torch.empty(ops.keypoint_weights_scratch(pts3d.shape[0], len(images)), dtype=torch.uint8, device=dev)
    t_img = timed(per_image)
    t_w = timed(lambda: ops.keypoint_weights(all_idx, ts, err, pts3d.shape[0], len(images), scratch=scratch))
    _, w, _ = ops.keypoint_weights(all_idx, ts, err, pts3d.shape[0], len(images), scratch=scratch)
    out = torch.empty(n, 2, device=dev)
    t_d = timed(lambda: ops.tie_point_depths(rays, p, all_idx, center, rng, w=w, out=out))
    return t_img, t_w, t_d


def main():
    print("device:", torch.cuda.get_device_name(0))
    for n_obs in (100_000, 1_000_000):
        images, pts3d, center, rng = scene(n_obs)
        t_img, t_w, t_d = kernels_alone(images, pts3d, center, rng)
        t_e2e = timed(lambda: data.depth_supervision_from_keypoints(images, pts3d, center, rng, dev), reps=5)
        print(f"{n_obs} observations, {len(images)} images, {pts3d.shape[0]} tie points: rays + reprojection errors (2 launches per image) "
              f"{t_img:.3f} ms, keypoint weights {t_w:.3f} ms, depth targets {t_d:.3f} ms; depth_supervision_from_keypoints end to end "
              f"{t_e2e:.1f} ms", flush=True)
        if n_obs == 100_000 and "--no-numpy" not in sys.argv:
            from tests import depth_supervision_reference as D

            t0 = time.perf_counter()
            D.depth_supervision(images, pts3d, center.numpy(), np.float32(rng))
            print(f"  stand-in (numpy restatement, one CPU core, not the reference): {1e3 * (time.perf_counter() - t0):.0f} ms", flush=True)


if __name__ == "__main__":
    main()
