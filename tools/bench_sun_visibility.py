"""Geometric sun visibility timings, HIP events around windows of back-to-back calls, the arms of a comparison
taking turns window by window in one process, median (min .. max) over the windows:
  sr_sun_rays at 512^2 and 2048^2 rays with sr_ortho_rays at the same counts beside it (its nearest relative: one fp64 geodetic
  conversion per ray);
  rendering.render_sun_visibility(depth=given) beside rendering.render_depth on one 8,192-ray chunk x 128 / 64 samples at widths 256
  and 512 (bf16, procedural weights): the sun pass is the same kernel on the same shapes, plus sr_sun_rays and the NaN fill;
  evaluate.sun_interp beside evaluate.sun_interp_shadows(shadows="geometry") on a 256 x 256 view (10 directions, width 256, 64 samples).
Usage: bench_sun_visibility.py [--no-render]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import satnerf_oracle as O  # noqa: E402
from oracle.rpc_oracle import latlon_to_ecef  # noqa: E402
from satnerf_amd import data, evaluate, ops, rendering  # noqa: E402
from satnerf_amd.models import load_model  # noqa: E402

dev = "cuda:0"
LAT0, LON0, ZONE = 30.3, -81.66, 17
MIN_ALT, MAX_ALT, RANGE = -24.0, 49.0, 210.0
SUN = data.sun_direction(35.0, 140.0)
N_RAYS = 8192
CONFIGS = [(256, 128), (256, 64), (512, 128), (512, 64)]
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
    return f"{stat[0]:.4f} ms ({stat[1]:.4f} .. {stat[2]:.4f}; {stat[3]} calls per window)"


def scene(side, res=0.5):
    e0, n0 = (t.item() for t in ops.utm_from_latlon(torch.tensor([LAT0], dtype=torch.float64, device=dev),
                                                   torch.tensor([LON0], dtype=torch.float64, device=dev), ZONE))
    grid = (float(np.floor(e0)) + 0.25 - side * res / 2, float(np.floor(n0)) + side * res / 2, side, side, res)
    return grid, np.array(latlon_to_ecef(LAT0, LON0, 0.5 * (MIN_ALT + MAX_ALT)))


def tau_of(feat):
    return 16 if feat == 512 else 4


def build(feat, s, chunk=N_RAYS):
    args = O.default_args(fc_units=feat, t_embbeding_tau=tau_of(feat), n_samples=s, mlp_mode="bf16", chunk=chunk)
    m = load_model(args)
    m.load_state_dict(O.procedural_satnerf_params(feat, tau_of(feat), seed=1))
    emb = torch.nn.Embedding(args.t_embbeding_vocab, tau_of(feat))
    emb.load_state_dict({"weight": O.procedural_uniform((args.t_embbeding_vocab, tau_of(feat)), 1.0, 7)})
    return args, {"coarse": m.to(dev).eval(), "t": emb.to(dev)}


def main():
    argv = sys.argv[1:]
    print("device:", torch.cuda.get_device_name(0), flush=True)
    out = {"sun_rays": {}, "sun_pass": {}}
    for side in (512, 2048):
        grid, center = scene(side)
        n = side * side
        rays = torch.empty(n, 11, dtype=torch.float32, device=dev)
        srays = torch.empty(n, 11, dtype=torch.float32, device=dev)

        def ortho():
            ops.ortho_rays(*grid[:2], grid[4], side, side, ZONE, MIN_ALT, MAX_ALT, center, RANGE, SUN.tolist(), dev, out=rays)

        ortho()
        depth = torch.rand(n, device=dev) * float(rays[0, 7])
        s, o = windows([lambda: ops.sun_rays(rays, depth, center, RANGE, MAX_ALT, None, 0.0, 1 / 64, out=srays), ortho])
        out["sun_rays"][side] = {"sr_sun_rays_ms": s[:3], "sr_ortho_rays_ms": o[:3]}
        print(f"{side}^2 rays: sr_sun_rays {fmt(s)}; sr_ortho_rays {fmt(o)}", flush=True)
    if "--no-render" in argv:
        print(json.dumps(out))
        return

    grid, center = scene(128)
    view = data.ortho_rays(grid, ZONE, MIN_ALT, MAX_ALT, center, RANGE, SUN, device=dev)[:N_RAYS].contiguous()
    ts = torch.full((N_RAYS,), 3, dtype=torch.int64, device=dev)
    with torch.no_grad():
        for feat, s in CONFIGS:
            args, models = build(feat, s)
            torch.manual_seed(0)
            depth = rendering.render_depth(models, view, ts, args)["depth"]
            sun, dep = windows([lambda: rendering.render_sun_visibility(models, view, ts, args, center, RANGE, MAX_ALT, depth=depth),
                                lambda: rendering.render_depth(models, view, ts, args)])
            out["sun_pass"][f"{feat}x{s}"] = {"sun_visibility_ms": sun[:3], "render_depth_ms": dep[:3], "ratio": sun[0] / dep[0]}
            print(f"width {feat}, {N_RAYS} rays x {s} samples: render_sun_visibility(depth=given) {fmt(sun)}; render_depth {fmt(dep)}; "
                  f"{sun[0] / dep[0]:.2f} x", flush=True)

        side = 256
        grid, center = scene(side)
        args, models = build(256, 64, chunk=N_RAYS)
        view = data.ortho_rays(grid, ZONE, MIN_ALT, MAX_ALT, center, RANGE, SUN, device=dev)
        ts = torch.full((side * side,), 3, dtype=torch.int64, device=dev)
        upper, lower = data.sun_direction(70.0, 120.0).numpy().astype(np.float64), data.sun_direction(30.0, 150.0).numpy().astype(np.float64)
        sweep = (models, view, ts, args, side, side, upper, lower, center, RANGE)
        geo, head = windows([lambda: evaluate.sun_interp_shadows(*sweep, shadows="geometry", max_alt=MAX_ALT), lambda: evaluate.sun_interp(*sweep)],
                            window_ms=1000.0, n_windows=5)
        out["sun_interp_256"] = {"geometry_ms": geo[:3], "head_ms": head[:3], "ratio": geo[0] / head[0]}
        print(f"sun_interp, {side} x {side} view, 10 directions, width 256, 64 samples: shadows='geometry' {geo[0]:.2f} ms ({geo[1]:.2f} .. {geo[2]:.2f}); "
              f"shadows='head' {head[0]:.2f} ms ({head[1]:.2f} .. {head[2]:.2f}); {geo[0] / head[0]:.2f} x (5 windows of {geo[3]} / {head[3]} calls)",
              flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
