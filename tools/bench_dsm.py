"""DSM extraction timings (HIP events, median of 10): dsm_from_depth over side x side points at radius 1 / 2, its three stages, the
XY + Z registration (compute_shift, and the whole dsm_mae(register="xyz")) of a side x side DSM pair, and render_dsm of a side x side
image at BASELINE configs[4]'s chunking (8192 rays x 128 samples).  Usage: bench_dsm.py [--registration-only] [side ...]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from satnerf_amd import data as O  # synthetic rays / default args
from satnerf_amd import dsm, ops
from satnerf_amd.models import load_model

dev = "cuda:0"
LAT0, LON0, RANGE = 30.3, -81.7, 600.0


def ecef(lat, lon, alt):
    a, e2 = 6378137.0, 6.69437999014e-3
    phi, lam = np.radians(lat), np.radians(lon)
    n = a / np.sqrt(1 - e2 * np.sin(phi) ** 2)
    return np.stack([(n + alt) * np.cos(phi) * np.cos(lam), (n + alt) * np.cos(phi) * np.sin(lam), (n * (1 - e2) + alt) * np.sin(phi)], -1)


def nadir_rays(side, res=0.5):
    """side^2 rays looking straight down at a 0.5 m local grid with a few metres of relief (one point per cell)."""
    center = ecef(LAT0, LON0, 0.0)
    phi, lam = np.radians(LAT0), np.radians(LON0)
    east = np.array([-np.sin(lam), np.cos(lam), 0.0])
    north = np.array([-np.sin(phi) * np.cos(lam), -np.sin(phi) * np.sin(lam), np.cos(phi)])
    up = np.cross(east, north)
    jj, cc = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    h = 10.0 + 3.0 * np.sin(cc / 17.0) * np.cos(jj / 23.0)
    target = (center + (cc.ravel()[:, None] - side / 2) * res * east - (jj.ravel()[:, None] - side / 2) * res * north
              + h.ravel()[:, None] * up)
    rays = np.zeros((side * side, 11), np.float32)
    rays[:, 0:3] = (target + 500.0 * up - center) / RANGE
    rays[:, 3:6] = -up
    depth = np.full(side * side, 500.0 / RANGE, np.float32)
    return torch.from_numpy(rays).to(dev), torch.from_numpy(depth).to(dev), center


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


def registration_pair(side, dx=13, dy=-11, dz=0.7):
    """A side x side DSM pair (boxes on a slope, a few NaN blobs) with v[j + dy, i + dx] = u[j, i] + dz, fp32 on the device."""
    rng = np.random.default_rng(side)
    pad = 32
    jj, ii = np.meshgrid(np.arange(side + 2 * pad), np.arange(side + 2 * pad), indexing="ij")
    f = 20.0 + 0.05 * ii - 0.03 * jj
    for _ in range(side * side // 1500):
        bh, bw = rng.integers(6, 40, size=2)
        y0, x0 = rng.integers(0, f.shape[0] - bh), rng.integers(0, f.shape[1] - bw)
        f[y0:y0 + bh, x0:x0 + bw] += rng.uniform(4.0, 40.0)
    u = f[pad:pad + side, pad:pad + side] + rng.normal(0, 0.05, (side, side))
    v = f[pad - dy:pad - dy + side, pad - dx:pad - dx + side] + dz + rng.normal(0, 0.05, (side, side))
    u[side // 4:side // 4 + 20, side // 3:side // 3 + 30] = np.nan
    return torch.from_numpy(u.astype(np.float32)).to(dev), torch.from_numpy(v.astype(np.float32)).to(dev)


def bench_registration(side):
    u, v = registration_pair(side)
    u64, v64 = u.double(), v.double()
    nbytes, levels = ops.dsm_register_plan(u.shape, v.shape, 5)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(9, dtype=torch.int64, device=dev)
    t_cs = timed(lambda: ops.dsm_compute_shift(u64, v64, irange=5, scaling=False, out=out, scratch=scratch))
    t_mae = timed(lambda: dsm.dsm_mae(v, u, register="xyz"))  # includes the fp64 widening, the apply, the MAE and its readback
    _, _, _, (dx, dy, _, b) = dsm.dsm_mae(v, u, register="xyz")
    print(f"registration {side}x{side}, {levels} levels, irange 5: compute_shift {t_cs:.3f} ms (device only), "
          f"dsm_mae(register='xyz') {t_mae:.3f} ms end to end; recovered ({dx}, {dy}), b = {b:.4f}", flush=True)


def main():
    argv = sys.argv[1:]
    registration_only = "--registration-only" in argv
    sides = [int(s) for s in argv if s != "--registration-only"] or [512, 2048]
    print("device:", torch.cuda.get_device_name(0))
    for side in sides:
        bench_registration(side)
    if registration_only:
        return
    for side in sides:
        rays, depth, center = nadir_rays(side)
        e, n, a, _ = ops.depth_to_utm(rays, depth, center, RANGE)
        b = ops.dsm_bounds(e, n, a).cpu().tolist()
        xoff, yoff, xsize, ysize = dsm.grid_from_bounds(*b, 0.5)
        t_utm = timed(lambda: ops.depth_to_utm(rays, depth, center, RANGE))
        t_bnd = timed(lambda: ops.dsm_bounds(e, n, a))
        for radius in (1, 2):
            t_ras = timed(lambda: ops.dsm_rasterize(e, n, a, xoff, yoff, 0.5, xsize, ysize, radius))
            t_all = timed(lambda: dsm.dsm_from_depth(rays, depth, center, RANGE, radius=radius))
            print(f"{side}x{side} points, grid {ysize}x{xsize}, radius {radius}: dsm_from_depth {t_all:.3f} ms "
                  f"(depth_to_utm {t_utm:.3f}, bounds {t_bnd:.3f}, rasterize {t_ras:.3f})", flush=True)
    # render_dsm at configs[4]'s chunking
    side = sides[0]
    args = O.default_args(mlp_mode="bf16", chunk=8192, n_samples=128)
    models = {"coarse": load_model(args).to(dev).eval(), "t": torch.nn.Embedding(30, 4).to(dev)}
    rays, ts = O.synthetic_rays(side * side, seed=9)
    rays, ts = rays.to(dev), ts.to(dev)
    center = ecef(LAT0, LON0, 0.0)
    from satnerf_amd import rendering

    t_rd = timed(lambda: dsm.render_dsm(models, rays, ts, args, center, RANGE, resolution=2.0), reps=3)
    t_img = timed(lambda: rendering.render_image_outputs(models, rays, ts, args), reps=3)
    print(f"render_dsm {side}x{side} image, chunk 8192 x 128 samples: {t_rd:.2f} ms (render_image_outputs alone {t_img:.2f} ms)")


if __name__ == "__main__":
    main()
