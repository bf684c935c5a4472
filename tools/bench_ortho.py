"""Nadir DSM timings, HIP events around windows of back-to-back calls, median and range over the windows:
sr_utm_to_latlon at 2^20 points; sr_ortho_rays at 512^2 and 2048^2 cells with sr_rpc_rays at the same pixel counts alternated beside it
in the same process (its nearest relative: one fp64 localisation per ray); render_ortho_dsm next to render_dsm on a random-initialised
width-256 model at 512^2.  Usage: bench_ortho.py [--no-render] [side ...]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.rpc_oracle import latlon_to_ecef, synthetic_rpc
from satnerf_amd import data, dsm, ops
from satnerf_amd.models import load_model

dev = "cuda:0"
LAT0, LON0, ZONE = 30.3, -81.66, 17
MIN_ALT, MAX_ALT, RANGE = -24.0, 49.0, 600.0
SUN = data.sun_direction(60.0, 140.0)
WINDOW_MS, WINDOWS = 100.0, 7


def windows(fns, window_ms=WINDOW_MS, n_windows=WINDOWS):
    """Per-call milliseconds of each fn: after a warm-up, n_windows windows of `reps` back-to-back calls between two events, the fns
    taking turns window by window; reps sized from a pilot so that a window lasts about window_ms.  Returns [(median, min, max, reps)]."""
    reps = []
    for fn in fns:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            fn()
        e1.record()
        torch.cuda.synchronize()
        reps.append(max(1, int(window_ms / max(e0.elapsed_time(e1) / 5, 1e-3))))
    times = [[] for _ in fns]
    for _ in range(n_windows):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps[k]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / reps[k])
    return [(float(np.median(t)), min(t), max(t), r) for t, r in zip(times, reps)]


def fmt(stat):
    return f"{stat[0]:.4f} ms (range {stat[1]:.4f} .. {stat[2]:.4f}, {WINDOWS} windows of {stat[3]} calls)"


def scene(side, res=0.5):
    e0, n0 = (t.item() for t in ops.utm_from_latlon(torch.tensor([LAT0], dtype=torch.float64, device=dev),
                                                   torch.tensor([LON0], dtype=torch.float64, device=dev), ZONE))
    grid = (float(np.floor(e0)) + 0.25 - side * res / 2, float(np.floor(n0)) + side * res / 2, side, side, res)
    return grid, np.array(latlon_to_ecef(LAT0, LON0, 0.5 * (MIN_ALT + MAX_ALT)))


def main():
    argv = sys.argv[1:]
    sides = [int(s) for s in argv if not s.startswith("--")] or [512, 2048]
    print("device:", torch.cuda.get_device_name(0), flush=True)

    n = 1 << 20
    rng = np.random.default_rng(0)
    east = torch.from_numpy(rng.uniform(2.0e5, 8.0e5, n)).to(dev)
    north = torch.from_numpy(rng.uniform(-6.0e6, 6.0e6, n)).to(dev)
    lat, lon = ops.utm_to_latlon(east, north, ZONE)
    out = torch.empty(2, n, dtype=torch.float64, device=dev)

    def inverse():
        ops._lib.call("sr_utm_to_latlon", ops._p(east), ops._p(north), n, ZONE, out[0].data_ptr(), out[1].data_ptr(), ops._stream())

    def forward():
        ops._lib.call("sr_utm_from_latlon", ops._p(lat), ops._p(lon), n, ZONE, out[0].data_ptr(), out[1].data_ptr(), ops._stream())

    inv, fwd = windows([inverse, forward])
    print(f"sr_utm_to_latlon, 2^20 points: {fmt(inv)}; sr_utm_from_latlon beside it: {fmt(fwd)}", flush=True)

    for side in sides:
        grid, center = scene(side)
        rpc = synthetic_rpc(seed=1, height=side, width=side)
        rays_o = torch.empty(side * side, 11, dtype=torch.float32, device=dev)
        rays_r = torch.empty(side * side, 11, dtype=torch.float32, device=dev)
        o, r = windows([lambda: ops.ortho_rays(*grid[:2], grid[4], side, side, ZONE, MIN_ALT, MAX_ALT, center, RANGE, SUN.tolist(), dev, out=rays_o),
                        lambda: ops.rpc_rays(rpc, side, side, MIN_ALT, MAX_ALT, center, RANGE, 60.0, 140.0, dev, out=rays_r)])
        print(f"{side}^2 rays: sr_ortho_rays {fmt(o)}; sr_rpc_rays {fmt(r)}", flush=True)

    if "--no-render" in argv:
        return
    side = 512
    grid, center = scene(side)
    args = data.default_args(mlp_mode="bf16", fc_units=256)
    torch.manual_seed(0)
    models = {"coarse": load_model(args).to(dev).eval(), "t": torch.nn.Embedding(30, 4).to(dev)}
    rays, ts = data.synthetic_rays(side * side, seed=9)
    rays, ts = rays.to(dev), ts.to(dev)
    a, b = windows([lambda: dsm.render_ortho_dsm(models, 3, args, center, RANGE, MIN_ALT, MAX_ALT, SUN, grid=grid, zone=ZONE),
                    lambda: dsm.render_dsm(models, rays, ts, args, center, RANGE, resolution=2.0)], window_ms=1000.0, n_windows=5)
    print(f"{side}^2 rays, width 256, {args.n_samples} samples, chunk {args.chunk}: render_ortho_dsm {a[0]:.2f} ms (range {a[1]:.2f} .. {a[2]:.2f}); "
          f"render_dsm {b[0]:.2f} ms (range {b[1]:.2f} .. {b[2]:.2f}); 5 windows of {a[3]} / {b[3]} calls", flush=True)


if __name__ == "__main__":
    main()
