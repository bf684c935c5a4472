"""Evaluation image product timings (median of 10 rounds after a warm-up, the legs interleaved round by round):
  fill              visualize.fill_nans_nearest on a 2048 x 2048 DSM with 1 %, 10 % and 50 % of its cells empty at random, and on one
                    with a single 600 x 600 hole (HIP events around 200 calls, per call; each call is both passes and the allocation of
                    its output and scratch), and ops.nearest_fill with both preallocated beside it: the two launches and the wrapper
  griddata          the reference's host path for the same raster: the device-to-host copy, scipy's griddata(method="nearest") and
                    the upload (host clock; printed only where scipy is installed; one run without a warm-up, it takes seconds)
  colouring         visualize.visualize_depth for one 800 x 800 image (HIP events around 100 calls, per call), and the reference's
                    numpy lines with a table lookup on the host beside it (host clock, with the copies)
  strips            visualize.dsm_strip, sun_strip and rgb_strip over ten 800 x 800 images (HIP events around 20 calls, per call; the DSMs
                    carry 10 % empty cells), and hstack + (img * 255).astype(uint8) in numpy beside the latter two (host clock, with the
                    copies)
Usage: bench_image_products.py [--quick]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from satnerf_amd import ops, visualize  # noqa: E402

dev = "cuda:0"
QUICK = "--quick" in sys.argv
SIDE = 256 if QUICK else 2048
IMG = 100 if QUICK else 800
ROUNDS = 2 if QUICK else 10
FILL_REPS, STRIP_REPS = (5, 2) if QUICK else (200, 20)


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def rounds(legs, n=ROUNDS, warm=True):
    t = {k: [] for k in legs}
    for r in range(n + warm):  # with warm, round 0 warms every leg up
        for k, fn in legs.items():
            ms = fn()
            if r or not warm:
                t[k].append(ms)
    for k, v in t.items():
        print(f"  {k}: median {np.median(v):.4f} ms, min {min(v):.4f}, max {max(v):.4f}", flush=True)


def griddata_path(dsm):
    """The host's hole fill for a GPU-resident DSM: copy down, scipy's nearest-neighbour griddata over (column, row) points, copy up."""
    from scipy.interpolate import griddata

    out = dsm.cpu().numpy()
    valid = ~np.isnan(out)
    out[~valid] = griddata(np.argwhere(valid)[:, ::-1], out[valid], np.argwhere(~valid)[:, ::-1], method="nearest")
    return torch.from_numpy(out).to(dev)


def depth_host(depth, table):
    """The depth colouring in numpy for a GPU-resident image, with its copies."""
    d = np.nan_to_num(depth.cpu().numpy())
    lo, hi = d.min(), d.max()
    index = (255 * ((d - lo) / (hi - lo + 1e-8))).astype(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(np.transpose(table[index].astype(np.float32) / np.float32(255), (2, 0, 1)))).to(dev)


def strip_host(images, channels):
    """A byte strip in numpy for GPU-resident images, with their copies."""
    tiles = []
    for i in images:
        img = i.cpu().numpy()
        r0, r1, c0, c1 = visualize.crop_window(*img.shape[:2])
        tiles.append(img[r0:r1, c0:c1, :channels])
    return torch.from_numpy((np.hstack(tiles) * 255).astype(np.uint8)).to(dev)


def main():
    print("device:", torch.cuda.get_device_name(0), "| torch CPU threads:", torch.get_num_threads())
    try:
        import scipy

        print("scipy", scipy.__version__)
    except ImportError:
        scipy = None
        print("scipy is not installed: the griddata leg is not measured")
    rng = np.random.default_rng(13)
    base = (rng.standard_normal((SIDE, SIDE)) * 8 + 30).astype(np.float32)
    rasters = {}
    for frac in (0.01, 0.10, 0.50):
        d = base.copy()
        d[rng.random(d.shape) < frac] = np.nan
        rasters[f"{100 * frac:.0f} % empty at random"] = d
    d = base.copy()
    hole = SIDE * 600 // 2048
    d[SIDE // 3:SIDE // 3 + hole, SIDE // 4:SIDE // 4 + hole] = np.nan
    rasters[f"one {hole} x {hole} hole"] = d
    for name, d in rasters.items():
        t = torch.from_numpy(d).to(dev)
        print(f"fill, {SIDE} x {SIDE}, {name} ({int(np.isnan(d).sum())} cells):", flush=True)
        out, scratch = torch.empty_like(t), torch.empty(ops.nearest_fill_scratch(SIDE, SIDE), dtype=torch.uint8, device=dev)
        rounds({"fill_nans_nearest": lambda: event_ms(lambda: visualize.fill_nans_nearest(t), FILL_REPS),
                "ops.nearest_fill into a given out and scratch": lambda: event_ms(lambda: ops.nearest_fill(t, out=out, scratch=scratch), FILL_REPS)})
        if scipy is not None:
            rounds({"griddata on the host, with the copies": lambda: host_ms(lambda: griddata_path(t))}, n=1, warm=False)

    table = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    lut = torch.from_numpy(table).to(dev)
    depths = [torch.from_numpy((rng.random((IMG, IMG)) * 40 + 3).astype(np.float32)).to(dev) for _ in range(10)]
    dsms = []
    for k in range(10):
        d = (rng.standard_normal((IMG, IMG)) * 8 + 30).astype(np.float32)
        d[rng.random(d.shape) < 0.10] = np.nan
        dsms.append(torch.from_numpy(d).to(dev))
    suns = [torch.from_numpy(rng.random((IMG, IMG, 1)).astype(np.float32)).to(dev) for _ in range(10)]
    rgbs = [torch.from_numpy(rng.random((IMG, IMG, 3)).astype(np.float32)).to(dev) for _ in range(10)]
    print(f"colouring, one {IMG} x {IMG} image:", flush=True)
    rounds({"visualize_depth": lambda: event_ms(lambda: visualize.visualize_depth(depths[0], lut), 5 * STRIP_REPS),
            "numpy on the host, with the copies": lambda: host_ms(lambda: depth_host(depths[0], table))})
    print(f"strips, ten {IMG} x {IMG} images (cropped to {IMG // 2} x {IMG // 2} each):", flush=True)
    rounds({"dsm_strip (fill + colour)": lambda: event_ms(lambda: visualize.dsm_strip(dsms, lut), STRIP_REPS),
            "sun_strip": lambda: event_ms(lambda: visualize.sun_strip(suns), STRIP_REPS),
            "rgb_strip": lambda: event_ms(lambda: visualize.rgb_strip(rgbs), STRIP_REPS),
            "sun strip in numpy on the host, with the copies": lambda: host_ms(lambda: strip_host(suns, 1)),
            "rgb strip in numpy on the host, with the copies": lambda: host_ms(lambda: strip_host(rgbs, 3))})


if __name__ == "__main__":
    main()
