"""Depth-only rendering against the full renders: procedural sat-nerf models in ``bf16``, no grad, one process,
every shape warmed up.  Per configuration -- 8,192-ray chunks x 128 samples (BASELINE configs[4]) and x 64 samples, widths 256 and
512 -- three arms on the same rays:
  depth    rendering.render_depth          one launch of the trunk-and-sigma core per chunk
  image    rendering.render_image_outputs  ray_sample -> the full fused MLP -> composite_image (what the DSM paths ran before)
  rays     rendering.render_rays           the one-launch full render pass
The arms alternate for ROUNDS windows of at least MIN_SECONDS each; a host clock is taken around a device synchronise.  Then
dsm.render_ortho_dsm on a 512 x 512 grid with and without geometry_only, whole calls alternating.  Prints median (min .. max) per arm,
the ratios, and the MFMA counts of the geometry and full streams from the generators' own stats.
Usage: bench_depth.py                                    the tables
       bench_depth.py --depth-only K [FEAT S]            K render_depth calls on one 8,192-ray chunk and nothing else (a kernel-trace run)
       bench_depth.py --kernel-us T [FEAT S]             the geometry kernel's share of the dense bf16 MFMA peak for a kernel time T (us)"""
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import satnerf_oracle as O  # noqa: E402
from satnerf_amd import dsm, packing, rendering  # noqa: E402
from satnerf_amd.models import load_model  # noqa: E402

dev = "cuda:0"
N_RAYS = 8192
CONFIGS = [(256, 128), (256, 64), (512, 128), (512, 64)]
ROUNDS, MIN_SECONDS = 7, 0.3
ORTHO_SIDE, ORTHO_ROUNDS = 512, 5
MFMA_PEAK_TFLOPS = 2500.0  # dense bf16 MFMA of the MI355X (bench.py)


def tau_of(feat):
    return 16 if feat == 512 else 4


def flops_per_point(feat):
    """2 x fan_in x fan_out over the nn.Linear layers a depth-only pass needs: fc_net and sigma_from_xyz (models/satnerf.py:183-185)."""
    return sum(2 * shp[0] * shp[1] for name, shp in packing.satnerf_param_shapes(feat, tau_of(feat)).items()
               if name.endswith(".weight") and name.startswith(("fc_net.", "sigma_from_xyz.")))


def stream_mfmas():
    """MFMAs per 32-point tile of the geometry and the full stream, from the generators (csrc/gen/fwd_core*.py stats)."""
    out = {}
    for feat, mod, cls in ((256, "fwd_core", "Core"), (512, "fwd_core512", "Core512")):
        spec = importlib.util.spec_from_file_location(mod + "_gen", os.path.join(ROOT, "satnerf_amd", "csrc", "gen", mod + ".py"))
        g = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(g)
        auxs = g.aux_steps(tau_of(feat))
        out[feat] = {"auxs": auxs, "geometry": getattr(g, cls)(auxs, heads=False).stats["mfma"], "full": getattr(g, cls)(auxs).stats["mfma"]}
    return out


def build(feat, s):
    args = O.default_args(fc_units=feat, t_embbeding_tau=tau_of(feat), n_samples=s, mlp_mode="bf16", chunk=N_RAYS)
    m = load_model(args)
    m.load_state_dict(O.procedural_satnerf_params(feat, tau_of(feat), seed=1))
    emb = torch.nn.Embedding(args.t_embbeding_vocab, tau_of(feat))
    emb.load_state_dict({"weight": O.procedural_uniform((args.t_embbeding_vocab, tau_of(feat)), 1.0, 7)})
    return args, {"coarse": m.to(dev).eval(), "t": emb.to(dev)}


def ortho_scene(side, res=0.5, lat0=30.3, lon0=-81.7, zone=17, min_alt=-24.0, max_alt=49.0, scene_range=210.0):
    """a side x side DSM grid around (lat0, lon0) and its scene normalisation: the ECEF point (WGS84) under the grid's middle at the mean
    altitude is the centre"""
    import math

    e0, n0 = (float(v[0]) for v in dsm.utm_from_latlon(torch.tensor([lat0], device=dev), torch.tensor([lon0], device=dev), zone))
    grid = (math.floor(e0) + 0.25 - math.floor(side * res / 2), math.floor(n0) + math.ceil(side * res / 2), side, side, res)
    a, e2, h = 6378137.0, 6.69437999014e-3, 0.5 * (min_alt + max_alt)
    phi, lam = math.radians(lat0), math.radians(lon0)
    nu = a / math.sqrt(1.0 - e2 * math.sin(phi) ** 2)
    center = np.array([(nu + h) * math.cos(phi) * math.cos(lam), (nu + h) * math.cos(phi) * math.sin(lam), (nu * (1.0 - e2) + h) * math.sin(phi)])
    return dict(grid=grid, zone=zone, center=center, scene_range=scene_range, min_alt=min_alt, max_alt=max_alt,
                sun_d=np.array([0.3213938, 0.3830222, 0.8660254], np.float32))


def window(fn):
    """calls/s over a window of calls lasting at least MIN_SECONDS, the clock stopped behind a device synchronise."""
    torch.cuda.synchronize()
    t0, calls = time.perf_counter(), 0
    while True:
        for _ in range(4):
            fn()
        calls += 4
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= MIN_SECONDS:
            return dt / calls


def summary(times_s):
    return {"median_us": statistics.median(times_s) * 1e6, "min_us": min(times_s) * 1e6, "max_us": max(times_s) * 1e6}


def feat_s_args(argv, at):
    return (int(argv[at]), int(argv[at + 1])) if len(argv) > at + 1 else CONFIGS[0]


def main():
    argv = sys.argv
    if len(argv) >= 3 and argv[1] == "--kernel-us":
        t, (feat, s) = float(argv[2]), feat_s_args(argv, 3)
        pts = N_RAYS * s
        print(json.dumps({"feat": feat, "samples": s, "flops_per_point": flops_per_point(feat), "kernel_us": t, "points": pts,
                          "mfma_share": flops_per_point(feat) * pts / (t * 1e-6) / 1e12 / MFMA_PEAK_TFLOPS}))
        return
    rays, ts = O.synthetic_rays(N_RAYS, seed=9)
    rays, ts = rays.to(dev), ts.to(dev)
    torch.manual_seed(0)
    if len(argv) >= 3 and argv[1] == "--depth-only":
        args, models = build(*feat_s_args(argv, 3))
        for _ in range(int(argv[2])):
            rendering.render_depth(models, rays, ts, args)
        torch.cuda.synchronize()
        return
    out = {"mfma_per_tile": stream_mfmas(), "configs": {}}
    print("MFMAs per 32-point tile:", out["mfma_per_tile"])
    with torch.no_grad():
        for feat, s in CONFIGS:
            args, models = build(feat, s)
            arms = {"depth": lambda: rendering.render_depth(models, rays, ts, args),
                    "image": lambda: rendering.render_image_outputs(models, rays, ts, args),
                    "rays": lambda: rendering.render_rays(models, args, rays, ts)}
            for fn in arms.values():  # warm-up: lazy initialisation, streams packed, allocator filled
                for _ in range(3):
                    fn()
            t = {k: [] for k in arms}
            for _ in range(ROUNDS):
                for k, fn in arms.items():
                    t[k].append(window(fn))
            res = {k: summary(v) for k, v in t.items()}
            res["image_over_depth"] = res["image"]["median_us"] / res["depth"]["median_us"]
            res["rays_over_depth"] = res["rays"]["median_us"] / res["depth"]["median_us"]
            # "faster by more than the spread": the slowest depth window against the fastest window of each comparison arm
            res["depth_faster_than_both_beyond_spread"] = res["depth"]["max_us"] < min(res["image"]["min_us"], res["rays"]["min_us"])
            out["configs"][f"{feat}x{s}"] = res
            print(f"width {feat}, {N_RAYS} rays x {s} samples, us per chunk, median (min .. max):")
            for k in arms:
                print(f"  {k:6s} {res[k]['median_us']:9.1f}  ({res[k]['min_us']:.1f} .. {res[k]['max_us']:.1f})")
            print(f"  image / depth {res['image_over_depth']:.2f} x, rays / depth {res['rays_over_depth']:.2f} x, "
                  f"beyond the spread: {res['depth_faster_than_both_beyond_spread']}")
    # render_ortho_dsm on a 512 x 512 grid (64 samples, width 256), whole calls
    args, models = build(256, 64)
    sc = ortho_scene(ORTHO_SIDE)
    common = (sc["center"], sc["scene_range"], sc["min_alt"], sc["max_alt"], sc["sun_d"])
    t = {False: [], True: []}
    for geometry_only in (False, True):
        dsm.render_ortho_dsm(models, 3, args, *common, grid=sc["grid"], zone=17, geometry_only=geometry_only)
    for _ in range(ORTHO_ROUNDS):
        for geometry_only in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dsm.render_ortho_dsm(models, 3, args, *common, grid=sc["grid"], zone=17, geometry_only=geometry_only)
            torch.cuda.synchronize()
            t[geometry_only].append(time.perf_counter() - t0)
    full, geo = summary(t[False]), summary(t[True])
    out["ortho_512"] = {"full_ms": {k[:-3]: v / 1e3 for k, v in full.items()}, "geometry_only_ms": {k[:-3]: v / 1e3 for k, v in geo.items()},
                        "ratio": full["median_us"] / geo["median_us"]}
    print(f"render_ortho_dsm {ORTHO_SIDE} x {ORTHO_SIDE}: full {full['median_us'] / 1e3:.2f} ms ({full['min_us'] / 1e3:.2f} .. {full['max_us'] / 1e3:.2f}), "
          f"geometry_only {geo['median_us'] / 1e3:.2f} ms ({geo['min_us'] / 1e3:.2f} .. {geo['max_us'] / 1e3:.2f}), {out['ortho_512']['ratio']:.2f} x")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
