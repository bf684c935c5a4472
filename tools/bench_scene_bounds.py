"""scene.loc timings (HIP events, median of 10 after a warm-up, the legs interleaved round by round):
sr_rpc_scene_bounds on one 2048 x 2048 synthetic camera, sr_rpc_rays on the same image (the same arithmetic plus 180 MB of stores: the
yardstick that already exists), and data.scene_bounds end to end for 20 such images (host RPC packing, 60 launches, the one
readback; a host clock around it, since it ends in that copy).  The reference cannot run without rpcm: as a LABELLED STAND-IN, the
numpy restatement (tests/scene_loc_reference.py, fp64 localisation, single-threaded numpy) is timed on a 1/64 subsample of one image
and scaled to the scene.
Usage: bench_scene_bounds.py [--no-numpy]"""
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
H = W = 2048
N_IMG, ROUNDS = 20, 10


def image(seed):
    rpc = R.synthetic_rpc(seed, height=H, width=W)
    return {"rpc": {a: (v.tolist() if isinstance(v, np.ndarray) else v) for a, v in rpc.items()}, "height": H, "width": W, "min_alt": -30.0,
            "max_alt": 70.0}


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    print("device:", torch.cuda.get_device_name(0))
    images = [image(300 + t) for t in range(N_IMG)]
    d = images[0]
    out, n_bad = torch.empty(6, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
    rays = torch.empty(H * W, 11, device=dev)
    center = [796912.4, -5453871.2, 3200310.9]
    legs = {
        "sr_rpc_scene_bounds": lambda: event_ms(lambda: ops.rpc_scene_bounds(d["rpc"], W, H, -30.0, 70.0, dev, out=out, n_bad=n_bad)),
        "sr_rpc_rays": lambda: event_ms(lambda: ops.rpc_rays(d["rpc"], W, H, -30.0, 70.0, center, 400.0, 50.0, 150.0, dev, out=rays)),
        "scene_bounds x20": lambda: host_ms(lambda: data.scene_bounds(images, device=dev)),
    }
    t = {k: [] for k in legs}
    for r in range(ROUNDS + 1):  # round 0 warms every leg up
        for k, fn in legs.items():
            ms = fn()
            if r:
                t[k].append(ms)
    for k, v in t.items():
        print(f"{k}: median {np.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f} ({H} x {W}" + (f", {N_IMG} images)" if "x20" in k else ")"),
              flush=True)
    print(f"bounds / rays = {np.median(t['sr_rpc_scene_bounds']) / np.median(t['sr_rpc_rays']):.3f}; n_bad = {n_bad.item()}", flush=True)
    if "--no-numpy" not in sys.argv:
        from tests import scene_loc_reference as S

        pixels = np.arange(0, H * W, 64)
        t0 = time.perf_counter()
        S.footprint(S.image_points(d, pixels=pixels))
        dt = time.perf_counter() - t0
        print(f"stand-in (numpy restatement, one CPU core, not the reference): {1e3 * dt:.0f} ms for {pixels.size} pixels of one image, "
              f"i.e. ~{dt * 64 * N_IMG:.0f} s for the {N_IMG}-image scene", flush=True)


if __name__ == "__main__":
    main()
