"""Colour loading timings (median of 10 rounds after a warm-up, the legs interleaved round by round) for one
2048 x 2048 x 3 8-bit image at img_downscale 1, 2 and 4:
  kernel            sr_image_colors alone, the bytes already on the device (HIP events around 20 launches, per launch)
  colors_from_image the host array to the finished (h*w, 3) device rows: the 3-byte-per-pixel upload and the kernel (host clock)
  reference path    datasets/satellite.py:67-80 restated with torch on the host: / 255. in fp64, torch.Tensor, CPU F.interpolate(bicubic)
                    when the factor is > 1, the (h*w, 3) fp32 rows, and their upload (host clock; torch's CPU threads as configured)
  F.interpolate GPU torch's own bicubic kernel on the fp32 CHW image already on the device, for information (HIP events, per launch)
Usage: bench_colors.py"""
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from satnerf_amd import data, ops  # noqa: E402

dev = "cuda:0"
H = W = 2048
ROUNDS, REPS = 10, 20


def event_ms(fn, reps=REPS):
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


def reference_path(img, h, w):
    """load_tensor_from_rgb_geotiff after the file read, then the upload its DataLoader would do row by row."""
    x = img / 255.  # (H, W, 3) float64
    if (h, w) != img.shape[:2]:
        x = F.interpolate(torch.Tensor(np.transpose(x, (2, 0, 1)))[None], size=(h, w), mode="bicubic", align_corners=False)[0]
        x = np.transpose(x.numpy(), (1, 2, 0))
    rgbs = torch.from_numpy(np.ascontiguousarray(x)).reshape(-1, 3).type(torch.FloatTensor)
    return rgbs.to(dev)


def main():
    print("device:", torch.cuda.get_device_name(0), "| torch CPU threads:", torch.get_num_threads())
    img = np.random.default_rng(11).integers(0, 256, (H, W, 3), dtype=np.uint8)
    on_dev = torch.from_numpy(img).to(dev)
    chw32 = (on_dev.permute(2, 0, 1).float() / 255.0).contiguous()[None]
    for s in (1, 2, 4):
        h, w = int(H // s), int(W // s)
        out = torch.empty(h * w, 3, device=dev)
        legs = {
            "kernel": lambda: event_ms(lambda: ops.image_colors(on_dev, h, w, out=out)),
            "colors_from_image": lambda: host_ms(lambda: data.colors_from_image(img, h, w, device=dev, out=out)),
            "reference path": lambda: host_ms(lambda: reference_path(img, h, w)),
        }
        if s > 1:
            legs["F.interpolate GPU"] = lambda: event_ms(lambda: F.interpolate(chw32, size=(h, w), mode="bicubic", align_corners=False))
        t = {k: [] for k in legs}
        for r in range(ROUNDS + 1):  # round 0 warms every leg up
            for k, fn in legs.items():
                ms = fn()
                if r:
                    t[k].append(ms)
        moved = 3 * H * W + 12 * h * w  # every source byte once, every output float once
        print(f"img_downscale {s}: {H} x {W} -> {h} x {w}, {moved / 1e6:.1f} MB moved by the kernel", flush=True)
        for k, v in t.items():
            extra = f", {moved / (1e6 * np.median(v)):.0f} GB/s" if k == "kernel" else ""
            print(f"  {k}: median {np.median(v):.4f} ms, min {min(v):.4f}, max {max(v):.4f}{extra}", flush=True)
        if s > 1:
            theirs = F.interpolate(chw32, size=(h, w), mode="bicubic", align_corners=False)[0].reshape(3, -1).t()
            print(f"  max |kernel - F.interpolate GPU| = {(ops.image_colors(on_dev, h, w) - theirs).abs().max().item():.2e}", flush=True)


if __name__ == "__main__":
    main()
