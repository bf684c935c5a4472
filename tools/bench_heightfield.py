"""Ray casting against a DSM raster, timings, HIP events around windows of back-to-back calls, the arms of a
comparison taking turns window by window in one process, median (min .. max) over the windows:
  sr_heightfield_blockmax on a 2048 x 2048 raster (0.5 m cells: rolling ground with flat-roofed boxes of up to 60 m on it);
  dsm.cast_rays for an 800 x 800 oblique view of it (640 k rays), plain and two-level walks alternated;
  dsm.shadow_mask of the raster at sun elevations 60, 25 and 10 degrees, plain and two-level walks alternated;
  dsm.sun_visibility_from_dsm on the view's own hit points, and rendering.render_sun_visibility(depth=given) on the same view beside it
  (width 256, 64 samples, bf16, procedural weights: the learned shadows' cost for the same pixels);
  cells visited per ray, counted on the CPU by a slab test at a reduced size (a 256 x 256 corner of the raster, 64 rays per case), and
  the bytes of raster they imply.
Usage: bench_heightfield.py [--no-render]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import satnerf_oracle as O  # noqa: E402
from oracle.rpc_oracle import latlon_to_ecef  # noqa: E402
from satnerf_amd import data, dsm, ops, rendering  # noqa: E402
from satnerf_amd.models import load_model  # noqa: E402

dev = "cuda:0"
LAT0, LON0, ZONE = 30.3, -81.66, 17
MIN_ALT, MAX_ALT = -24.0, 80.0
SIDE, RES, VIEW = 2048, 0.5, 800
RANGE = 0.75 * SIDE * RES
ELEVATIONS = (60.0, 25.0, 10.0)
AZIMUTH = 140.0
WINDOW_MS, WINDOWS = 100.0, 7


def windows(fns, window_ms=WINDOW_MS, n_windows=WINDOWS):
    """Per-call milliseconds of each fn: after a warm-up, n_windows windows of `reps` back-to-back calls between two events, the fns
    taking turns window by window; reps sized from a pilot so that a window lasts about window_ms.  Returns [(median, min, max, reps)]."""
    reps = []
    for fn in fns:
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            fn()
        e1.record()
        torch.cuda.synchronize()
        reps.append(max(1, int(window_ms / max(e0.elapsed_time(e1) / 3, 1e-3))))
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
    return f"{stat[0]:.4f} ms ({stat[1]:.4f} .. {stat[2]:.4f}; {stat[3]} calls per window)"


def city(side, seed=0):
    """(side, side) fp32: rolling ground of 0 .. 6 m, one flat-roofed box per 1,500 cells (8 .. 80 cells on a side, 5 .. 60 m high),
    0.5 % of the cells NaN."""
    rng = np.random.default_rng(seed)
    jj, cc = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    h = (3.0 + 2.0 * np.sin(jj / 97.0) + np.cos(cc / 61.0)).astype(np.float32)
    for _ in range(side * side // 1500):
        j, c, dj, dc = rng.integers(0, side), rng.integers(0, side), rng.integers(8, 81), rng.integers(8, 81)
        h[j:j + dj, c:c + dc] = np.float32(rng.uniform(5.0, 60.0))
    h[rng.random((side, side)) < 0.005] = np.nan
    return h


def visited_cells(hgt, r, A, B, start):
    """(cells crossed before the walk ends, per ray) by a slab test of every column's footprint, numpy on the CPU: the columns whose
    footprint the segment crosses at an s no larger than the s of its first hit (all it crosses, on a miss).  ``start``: per ray the
    (row, column) of the cell it leaves, which cannot stop it."""
    ys, xs = hgt.shape
    out = []
    for a, b, (j0, c0) in zip(A, B, start):
        d = b - a
        with np.errstate(all="ignore"):
            tx = (np.arange(xs + 1) * r - a[0]) / d[0] if d[0] != 0 else np.where(np.arange(xs + 1) * r <= a[0], -np.inf, np.inf)
            ty = (np.arange(ys + 1) * r - a[1]) / d[1] if d[1] != 0 else np.where(np.arange(ys + 1) * r <= a[1], -np.inf, np.inf)
        lox, hix = np.minimum(tx[:-1], tx[1:]), np.maximum(tx[:-1], tx[1:])
        loy, hiy = np.minimum(ty[:-1], ty[1:]), np.maximum(ty[:-1], ty[1:])
        lo = np.maximum(np.maximum(lox[None, :], loy[:, None]), 0.0)
        hi = np.minimum(np.minimum(hix[None, :], hiy[:, None]), 1.0)
        crossed = lo < hi
        z_in, z_out = a[2] + lo * d[2], a[2] + hi * d[2]
        hit = crossed & np.isfinite(hgt) & (np.minimum(z_in, z_out) <= hgt)
        hit[j0, c0] = False
        s_hit = lo[hit].min() if hit.any() else np.inf
        out.append(int((crossed & (lo <= s_hit)).sum()))
    return np.array(out)


def oblique_view(grid, center, side, off_nadir_deg=30.0):
    """(side * side, 11) fp32 rays looking at the cell centres of ``grid`` from ``off_nadir_deg`` off the vertical, towards the north-east:
    the nadir rays of data.ortho_rays, turned about their points at mid altitude (fp64 on the device, rounded once)."""
    nadir = data.ortho_rays(grid, ZONE, MIN_ALT, MAX_ALT, center, RANGE, data.sun_direction(ELEVATIONS[0], AZIMUTH), device=dev).double()
    o, d, far = nadir[:, 0:3], nadir[:, 3:6], nadir[:, 7:8]
    lam = np.radians(LON0)
    east = torch.tensor([-np.sin(lam), np.cos(lam), 0.0], dtype=torch.float64, device=dev)
    north = torch.linalg.cross(-d, east.expand_as(d))
    t = np.radians(off_nadir_deg)
    look = np.cos(t) * d + np.sin(t) * (0.6 * east + 0.8 * north)
    look = look / look.norm(dim=1, keepdim=True)
    mid = o + d * (0.5 * far)
    rays = nadir.clone()
    rays[:, 0:3] = mid - look * (0.5 * far / np.cos(t))
    rays[:, 3:6] = look
    rays[:, 7:8] = far / np.cos(t)
    return rays.float().contiguous()


def main():
    argv = sys.argv[1:]
    print("device:", torch.cuda.get_device_name(0), flush=True)
    out = {}
    e0, n0 = (t.item() for t in ops.utm_from_latlon(torch.tensor([LAT0], dtype=torch.float64, device=dev),
                                                   torch.tensor([LON0], dtype=torch.float64, device=dev), ZONE))
    xoff, yoff = float(np.floor(e0)) + 0.25 - SIDE * RES / 2, float(np.floor(n0)) + SIDE * RES / 2
    center = np.array(latlon_to_ecef(LAT0, LON0, 0.5 * (MIN_ALT + MAX_ALT)))
    hgt_np = city(SIDE)
    hgt = torch.as_tensor(hgt_np).to(dev)
    surface = dsm.DSM(hgt, torch.ones_like(hgt), xoff, yoff, RES, f"{ZONE}R")

    b = windows([lambda: ops.heightfield_blockmax(hgt)])[0]
    out["blockmax_2048"] = b[:3]
    print(f"sr_heightfield_blockmax, {SIDE} x {SIDE}: {fmt(b)}  ({hgt.numel() * 4 / b[0] / 1e9:.2f} TB/s of raster)", flush=True)

    step = SIDE * RES / VIEW
    view = oblique_view((xoff, yoff, VIEW, VIEW, step), center, VIEW)
    plain, fast = windows([lambda: dsm.cast_rays(surface, view, center, RANGE, accelerate=False),
                           lambda: dsm.cast_rays(surface, view, center, RANGE, accelerate=True)])
    res = dsm.cast_rays(surface, view, center, RANGE)
    out["cast_rays_800"] = {"plain_ms": plain[:3], "two_level_ms": fast[:3], "hit_fraction": float(res["hit"].float().mean())}
    print(f"cast_rays, {VIEW} x {VIEW} view at 30 degrees off nadir ({float(res['hit'].float().mean()):.3f} of the rays hit): plain {fmt(plain)}; "
          f"two-level {fmt(fast)}; {plain[0] / fast[0]:.2f} x", flush=True)

    out["shadow_mask_2048"] = {}
    for el in ELEVATIONS:
        sun = data.sun_direction(el, AZIMUTH)
        plain, fast = windows([lambda: dsm.shadow_mask(surface, sun, accelerate=False), lambda: dsm.shadow_mask(surface, sun, accelerate=True)])
        lit = float(torch.nanmean(dsm.shadow_mask(surface, sun)))
        out["shadow_mask_2048"][el] = {"plain_ms": plain[:3], "two_level_ms": fast[:3], "lit_fraction": lit}
        print(f"shadow_mask, {SIDE} x {SIDE}, elevation {el:.0f} ({lit:.3f} lit): plain {fmt(plain)}; two-level {fmt(fast)}; "
              f"{plain[0] / fast[0]:.2f} x", flush=True)

    # cells per ray on the CPU at a reduced size: a corner of the raster, the mask's own segments from 64 of its cells
    small = hgt_np[:256, :256]
    rng = np.random.default_rng(1)
    top = np.nanmax(small)
    out["cells_per_ray_256"] = {}
    for el in ELEVATIONS:
        u = data.sun_direction(el, AZIMUTH).double().numpy()
        jj, cc = rng.integers(0, 256, 64), rng.integers(0, 256, 64)
        keep = np.isfinite(small[jj, cc])
        A = np.stack([(cc + 0.5) * RES, (jj + 0.5) * RES, small[jj, cc].astype(np.float64)], 1)[keep]
        t = (top - A[:, 2]) / u[2]
        B = np.stack([A[:, 0] + t * u[0], A[:, 1] - t * u[1], np.full(len(A), top)], 1)
        n = visited_cells(small, RES, A, B, np.stack([jj, cc], 1)[keep])
        out["cells_per_ray_256"][el] = {"mean": float(n.mean()), "max": int(n.max())}
        print(f"cells crossed per shadow ray on a 256 x 256 corner, elevation {el:.0f}: mean {n.mean():.1f}, max {n.max()} "
              f"({4 * n.mean():.0f} bytes of raster per ray; a ray that leaves the corner is cut short)", flush=True)

    if "--no-render" in argv:
        print(json.dumps(out))
        return
    args = O.default_args(fc_units=256, t_embbeding_tau=4, n_samples=64, mlp_mode="bf16", chunk=8192)
    m = load_model(args)
    m.load_state_dict(O.procedural_satnerf_params(256, 4, seed=1))
    emb = torch.nn.Embedding(args.t_embbeding_vocab, 4)
    emb.load_state_dict({"weight": O.procedural_uniform((args.t_embbeding_vocab, 4), 1.0, 7)})
    models = {"coarse": m.to(dev).eval(), "t": emb.to(dev)}
    ts = torch.full((VIEW * VIEW,), 3, dtype=torch.int64, device=dev)
    depth = torch.where(res["hit"], res["depth"], view[:, 7])  # the DSM's own depth in the view's pixels
    sun = data.sun_direction(25.0, AZIMUTH)
    with torch.no_grad():
        geo, learned = windows([lambda: dsm.sun_visibility_from_dsm(surface, view, depth, center, RANGE, MAX_ALT, sun_d=sun, n_samples=64),
                                lambda: rendering.render_sun_visibility(models, view, ts, args, center, RANGE, MAX_ALT, sun_d=sun, depth=depth)],
                               window_ms=300.0, n_windows=5)
    out["view_shadows_800"] = {"sun_visibility_from_dsm_ms": geo[:3], "render_sun_visibility_ms": learned[:3]}
    print(f"shadows in the view's pixels, {VIEW} x {VIEW}, elevation 25: sun_visibility_from_dsm {fmt(geo)}; "
          f"render_sun_visibility(depth=given), width 256 x 64 samples {fmt(learned)}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
