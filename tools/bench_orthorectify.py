"""Orthorectification onto a DSM raster, timings, on the 2048 x 2048 raster of bench_heightfield.py with a
2048 x 2048 uint8 RGB image, HIP events around windows of back-to-back calls as there, the arms of a comparison taking turns window by
window in one process, median (min .. max) over the windows:
  the projection launch of sr_orthorectify alone (stage "project");
  the walk + sample + accumulate launch alone (stage "sample") per sampler, plain and two-level walks alternated;
  dsm.shadow_mask of the same raster at the sun elevation that matches the camera's lean, plain and two-level, for scale;
  dsm.ortho_mosaic of 10 views.
The camera leans 30 degrees off nadir (a point 1 m higher appears tan 30 = 0.58 m further east), the shadow mask's sun stands at 60.
Usage: bench_orthorectify.py"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_heightfield import AZIMUTH, LAT0, LON0, RES, SIDE, ZONE, city, fmt, windows  # noqa: E402
from oracle.rpc_oracle import synthetic_rpc  # noqa: E402
from satnerf_amd import data, dsm, ops  # noqa: E402

dev = "cuda:0"
OFF_NADIR = 30.0
N_VIEWS = 10
MODES = ("nearest", "bilinear", "bicubic")


def camera(seed, tan_theta, side=SIDE):
    """rpc_oracle.synthetic_rpc aimed at the raster: its normalised range [-1, 1] spans 1.3 x the raster, altitudes normalised by
    offset 30 m and scale 60 m, and a point 1 m higher appears ``tan_theta`` metres further east."""
    rpc = {k: (np.array(v, np.float64) if np.ndim(v) else v) for k, v in synthetic_rpc(seed, height=side, width=side).items()}
    p = np.radians(LAT0)
    m_lat, m_lon = 111132.92 - 559.82 * np.cos(2 * p), 111412.84 * np.cos(p) - 93.5 * np.cos(3 * p)
    rpc["lat_offset"], rpc["lon_offset"], rpc["alt_offset"], rpc["alt_scale"] = LAT0, LON0, 30.0, 60.0
    rpc["lon_scale"] = 1.3 * SIDE * RES / (2.0 / rpc["col_num"][1]) / m_lon
    rpc["lat_scale"] = 1.3 * SIDE * RES / (2.0 / abs(rpc["row_num"][2])) / m_lat
    rpc["col_num"][3] = tan_theta * rpc["col_num"][1] * rpc["alt_scale"] / (rpc["lon_scale"] * m_lon)
    return rpc


def main():
    print("device:", torch.cuda.get_device_name(0), flush=True)
    out = {}
    e0, n0 = (t.item() for t in ops.utm_from_latlon(torch.tensor([LAT0], dtype=torch.float64, device=dev),
                                                   torch.tensor([LON0], dtype=torch.float64, device=dev), ZONE))
    xoff, yoff = float(np.floor(e0)) + 0.25 - SIDE * RES / 2, float(np.floor(n0)) + SIDE * RES / 2
    hgt = torch.as_tensor(city(SIDE)).to(dev)
    surface = dsm.DSM(hgt, torch.ones_like(hgt), xoff, yoff, RES, f"{ZONE}R")
    rng = np.random.default_rng(0)
    images = [torch.as_tensor(rng.integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8)).to(dev) for _ in range(N_VIEWS)]
    tan_theta = float(np.tan(np.radians(OFF_NADIR)))
    rpc = camera(0, tan_theta)

    maxima = ops.heightfield_blockmax(hgt)
    scratch = torch.empty(ops.orthorectify_scratch(SIDE, SIDE), dtype=torch.uint8, device=dev)
    color, status, colrow = ops.orthorectify(hgt, RES, xoff, yoff, ZONE, rpc, images[0], maxima=maxima, scratch=scratch)
    shares = {k: float((status == v).float().mean()) for k, v in (("empty", 0), ("visible", 1), ("occluded", 2), ("outside", 3))}
    out["shares"] = shares
    print(f"{SIDE} x {SIDE} raster, {SIDE} x {SIDE} x 3 uint8 image, {OFF_NADIR:.0f} degrees off nadir: {shares}", flush=True)

    def call(stage, mode="bilinear", accelerate=True):
        return ops.orthorectify(hgt, RES, xoff, yoff, ZONE, rpc, images[0], mode=mode, accelerate=accelerate, maxima=maxima, scratch=scratch,
                                color=color, status=status, colrow=colrow, stage=stage)

    p = windows([lambda: call("project")])[0]
    out["project_ms"] = p[:3]
    print(f"projection launch: {fmt(p)}", flush=True)
    out["sample_ms"] = {}
    for mode in MODES:
        plain, fast = windows([lambda: call("sample", mode, False), lambda: call("sample", mode, True)])
        out["sample_ms"][mode] = {"plain": plain[:3], "two_level": fast[:3]}
        print(f"walk + sample launch, {mode}: plain {fmt(plain)}; two-level {fmt(fast)}; {plain[0] / fast[0]:.2f} x", flush=True)

    sun = data.sun_direction(90.0 - OFF_NADIR, AZIMUTH)
    plain, fast = windows([lambda: dsm.shadow_mask(surface, sun, accelerate=False), lambda: dsm.shadow_mask(surface, sun, accelerate=True)])
    out["shadow_mask_ms"] = {"plain": plain[:3], "two_level": fast[:3]}
    print(f"shadow_mask, same raster, elevation {90.0 - OFF_NADIR:.0f}: plain {fmt(plain)}; two-level {fmt(fast)}", flush=True)

    views = [(images[k], camera(k, tan_theta * np.cos(0.6 * k) * (0.5 + 0.05 * k))) for k in range(N_VIEWS)]
    m = windows([lambda: dsm.ortho_mosaic(surface, views)], window_ms=300.0, n_windows=5)[0]
    count = dsm.ortho_mosaic(surface, views)["count"]
    out["mosaic_10_ms"] = m[:3]
    print(f"ortho_mosaic, {N_VIEWS} views, bilinear: {fmt(m)}; cells seen by at least one view {float((count > 0).float().mean()):.3f}, "
          f"mean views per cell {float(count.float().mean()):.2f}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
