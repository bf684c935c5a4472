"""Classic-NeRF rendering throughput: ``render_rays`` on 16,384 classic rays, n_samples = 64 coarse +
n_importance = 64, two procedural models, no grad, in one process with every shape warmed up:
  bf16     each pass one fused launch (csrc/nerf_fwd.inc: sr_nerf_render_fwd)
  bf16x3   the layer-by-layer path (satnerf_amd/generic.py: one csrc/linear.hip launch per nn.Linear, three MFMA passes)
The two alternate for 7 rounds of at least 0.5 s each; a host clock is taken around a device synchronise.  Prints the median and range
of rays/s for both, their ratio, and what the fused kernel's share of the dense bf16 MFMA peak is for a given kernel time (FLOPs per point
from the layer shapes).
Usage: bench_nerf.py                 the table
       bench_nerf.py --fused-only K  K fused render_rays calls and nothing else (the program of a kernel-trace run)
       bench_nerf.py --kernel-us T   the MFMA share for a measured kernel time T (microseconds per 16,384 x 128-point fine pass)"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import satnerf_oracle as O  # noqa: E402
from satnerf_amd import packing, rendering  # noqa: E402
from satnerf_amd.models import load_model  # noqa: E402

dev = "cuda:0"
N_RAYS, S, I = 16384, 64, 64
ROUNDS, MIN_SECONDS = 7, 0.5
MFMA_PEAK_TFLOPS = 2500.0  # dense bf16 MFMA of the MI355X (bench.py)


def flops_per_point(feat=256):
    """2 x fan_in x fan_out over the nn.Linear layers of the classic NeRF (models/nerf.py:156-177)."""
    return sum(2 * shp[0] * shp[1] for name, shp in packing.nerf_param_shapes(feat).items() if name.endswith(".weight"))


def mfma_share(kernel_us, points):
    return flops_per_point() * points / (kernel_us * 1e-6) / 1e12 / MFMA_PEAK_TFLOPS


def window(fn):
    """rays/s over a window of calls lasting at least MIN_SECONDS, the clock stopped behind a device synchronise."""
    torch.cuda.synchronize()
    t0, calls = time.perf_counter(), 0
    while True:
        for _ in range(4):
            fn()
        calls += 4
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= MIN_SECONDS:
            return calls * N_RAYS / dt


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--kernel-us":
        t = float(sys.argv[2])
        print(json.dumps({"flops_per_point": flops_per_point(), "kernel_us": t, "points": N_RAYS * (S + I), "mfma_share": mfma_share(t, N_RAYS * (S + I))}))
        return
    args = {m: O.default_args(model="nerf", n_samples=S, n_importance=I, mlp_mode=m, chunk=N_RAYS) for m in ("bf16", "bf16x3")}
    models = {}
    for typ, seed in (("coarse", 1), ("fine", 2)):
        m = load_model(args["bf16"])
        m.load_state_dict(O.procedural_nerf_params(256, seed=seed))
        models[typ] = m.to(dev).eval()
    rays = O.synthetic_rays(N_RAYS, seed=9, classic=True)[0].to(dev)
    torch.manual_seed(0)
    run = {m: (lambda a=a: rendering.render_rays(models, a, rays, None)) for m, a in args.items()}
    with torch.no_grad():
        if len(sys.argv) == 3 and sys.argv[1] == "--fused-only":
            for _ in range(int(sys.argv[2])):
                run["bf16"]()
            torch.cuda.synchronize()
            return
        for fn in run.values():  # warm-up: lazy initialisation, streams packed, allocator filled
            for _ in range(2):
                fn()
        rates = {m: [] for m in run}
        for _ in range(ROUNDS):
            for m, fn in run.items():
                rates[m].append(window(fn))
    out = {m: {"median_rays_per_s": statistics.median(r), "min": min(r), "max": max(r)} for m, r in rates.items()}
    out["ratio"] = out["bf16"]["median_rays_per_s"] / out["bf16x3"]["median_rays_per_s"]
    out["flops_per_point"] = flops_per_point()
    for m in run:
        o = out[m]
        print(f"{m:7s} {o['median_rays_per_s'] / 1e6:7.3f} M rays/s  ({o['min'] / 1e6:.3f} .. {o['max'] / 1e6:.3f})")
    print(f"fused / layer path: {out['ratio']:.2f} x")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
