"""Cloud-fusion timings (HIP events, median of 10 after a warm-up): sr_cloud_grid's five stages and the whole call
for "med" and "avg" on 1, 10 and 20 clouds of 512 x 512 points and one of 2048 x 2048 on a 0.5 m grid, then render_fused_dsm of 10 views
of 512 x 512 at BASELINE configs[4]'s chunking (8192 rays x 128 samples) beside render_dsm of one view.  A stage's time is the
difference of two runs cut after consecutive stages.  The numpy line is a labelled stand-in on one CPU core (the restatement of
tests/cloud_grid_reference.py), not the reference function's time.  Usage: bench_cloud_grid.py [--no-render] [--no-numpy]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from satnerf_amd import data as O  # synthetic rays / default args
from satnerf_amd import dsm, ops
from satnerf_amd.models import load_model

dev = "cuda:0"
STAGES = ("key+count", "scan", "scatter", "sort", "reduce")
LAT0, LON0, RANGE = 30.3, -81.7, 600.0


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


def clouds(side, views, res=0.5, seed=0):
    """`views` clouds of side^2 points over one side x side grid of `res` cells: view 0 hits every cell centre (a nadir view), the
    others are sheared by up to a few cells with height (oblique views), so cells hold about `views` points, some more, some fewer."""
    rng = np.random.default_rng(seed)
    jj, cc = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    h = 10.0 + 3.0 * np.sin(cc / 17.0) * np.cos(jj / 23.0) + 15.0 * ((cc // 40 + jj // 56) % 3 == 0)  # relief and boxes
    e, n, a = [], [], []
    for v in range(views):
        tx, ty = (rng.uniform(-0.35, 0.35, 2) if v else (0.0, 0.0))  # tan of the off-nadir angle, per axis
        e.append(435000.0 + (cc + 0.5) * res + tx * h + rng.uniform(-0.2, 0.2, h.shape) * (v > 0))
        n.append(3354000.0 - (jj + 0.5) * res + ty * h + rng.uniform(-0.2, 0.2, h.shape) * (v > 0))
        a.append(h + rng.normal(0, 0.05, h.shape))
    cat = lambda x: torch.from_numpy(np.concatenate([t.ravel() for t in x])).to(dev)
    return cat(e), cat(n), cat(a), (435000.0, 3354000.0, res, side, side)


def bench_grid(side, views, numpy_too):
    e, n, a, grid = clouds(side, views)
    npts = e.numel()
    scratch = torch.empty(ops.cloud_grid_scratch(npts, side, side), dtype=torch.uint8, device=dev)
    out = torch.empty(side, side, dtype=torch.float64, device=dev)
    count = torch.empty(side, side, dtype=torch.int32, device=dev)
    for mode in ("med", "avg"):
        cum = [timed(lambda k=k: ops.cloud_grid(e, n, a, *grid, rule="floor", mode=mode, scratch=scratch, out=out, count=count, stages=k))
               for k in (1, 2, 3, 4)]
        whole = timed(lambda: ops.cloud_grid(e, n, a, *grid, rule="floor", mode=mode, scratch=scratch, out=out, count=count))
        cum.append(whole)
        parts = [cum[0]] + [cum[k] - cum[k - 1] for k in range(1, 5)]
        c = count.cpu().numpy()
        print(f"{views:2d} x {side}x{side} points ({npts / 1e6:.2f} M), grid {side}x{side}, {mode}: whole {whole:.3f} ms = "
              + ", ".join(f"{s} {p:.3f}" for s, p in zip(STAGES, parts))
              + f"; scratch {scratch.numel() / 2**20:.1f} MiB; points per cell: mean {c.mean():.1f}, max {c.max()}, "
              f"cells > 64: {(c > 64).sum()}", flush=True)
    t_dsm = timed(lambda: dsm.dsm_from_clouds(e, n, a, roi=[435000.0, 3354000.0 - side * 0.5, side, 0.5]))
    print(f"{views:2d} x {side}x{side}: dsm_from_clouds(roi=, med) {t_dsm:.3f} ms (with the fp32 conversions)", flush=True)
    if numpy_too:
        sys.path.insert(0, ROOT)
        from tests import cloud_grid_reference as R

        en, nn, an = e.cpu().numpy(), n.cpu().numpy(), a.cpu().numpy()
        t0 = time.perf_counter()
        R.cloud_grid_np(en, nn, an, *grid, "floor", "med")
        print(f"{views:2d} x {side}x{side}: STAND-IN, not the reference function: the vectorised numpy restatement on one CPU core, med: "
              f"{(time.perf_counter() - t0) * 1e3:.0f} ms", flush=True)


def ecef(lat, lon, alt):
    a, e2 = 6378137.0, 6.69437999014e-3
    phi, lam = np.radians(lat), np.radians(lon)
    n = a / np.sqrt(1 - e2 * np.sin(phi) ** 2)
    return np.stack([(n + alt) * np.cos(phi) * np.cos(lam), (n + alt) * np.cos(phi) * np.sin(lam), (n * (1 - e2) + alt) * np.sin(phi)], -1)


def bench_render(side=512, n_views=10):
    from satnerf_amd import rendering

    args = O.default_args(mlp_mode="bf16", chunk=8192, n_samples=128)
    models = {"coarse": load_model(args).to(dev).eval(), "t": torch.nn.Embedding(30, 4).to(dev)}
    center = ecef(LAT0, LON0, 0.0)
    views = []
    for v in range(n_views):
        rays, ts = O.synthetic_rays(side * side, seed=9 + v)
        views.append((rays.to(dev), ts.to(dev)))
    t_one = timed(lambda: dsm.render_dsm(models, *views[0], args, center, RANGE, resolution=2.0), reps=3)
    t_img = timed(lambda: [rendering.render_image_outputs(models, r, t, args) for r, t in views], reps=3)
    t_fused = timed(lambda: dsm.render_fused_dsm(models, views, args, center, RANGE, resolution=2.0), reps=3)
    # the fusion alone on the clouds those views give (depth_to_utm of each view, bounds, sr_cloud_grid, conversions)
    with torch.no_grad():
        depths = [rendering.render_image_outputs(models, r, t, args)["depth"] for r, t in views]

    def fuse():
        cl = [ops.depth_to_utm(r, d, center, RANGE, 17)[:3] for (r, _), d in zip(views, depths)]
        return dsm.dsm_from_clouds([c[0] for c in cl], [c[1] for c in cl], [c[2] for c in cl], resolution=2.0)

    t_fuse = timed(fuse)
    out = fuse()
    w = out.weight.cpu().numpy()
    print(f"render_dsm, one {side}x{side} view, chunk 8192 x 128 samples: {t_one:.2f} ms", flush=True)
    print(f"render_fused_dsm, {n_views} views of {side}x{side}: {t_fused:.2f} ms; render_image_outputs of the {n_views} views alone {t_img:.2f} ms; "
          f"depth_to_utm x {n_views} + dsm_from_clouds alone {t_fuse:.3f} ms = {100 * t_fuse / t_fused:.2f} % of render_fused_dsm "
          f"(grid {tuple(out.dsm.shape)}, points per cell: mean {w.mean():.1f}, max {w.max():.0f})", flush=True)


def main():
    argv = sys.argv[1:]
    print("device:", torch.cuda.get_device_name(0))
    for side, views in ((512, 1), (512, 10), (512, 20), (2048, 1)):
        bench_grid(side, views, "--no-numpy" not in argv)
    if "--no-render" not in argv:
        bench_render()


if __name__ == "__main__":
    main()
