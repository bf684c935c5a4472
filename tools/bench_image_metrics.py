"""Image-metric timings (HIP events, median of 20 after a warm-up): metrics.psnr and metrics.ssim of 3 x side x side fp32 images, the
whole call (validation, launches, the fp64 -> fp32 tail) and the two launches alone (ops.image_sse / ops.ssim_sum with preallocated
output and scratch), with the rate at which the two images are read (2 x 4 B x 3 x side^2 per call).  "rotating" cycles through enough
image pairs (>= 512 MiB) that each call reads HBM rather than the 256 MiB Infinity Cache.  Usage: bench_image_metrics.py [side ...]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from satnerf_amd import metrics, ops

dev = "cuda:0"


def timed(fn, reps=20):
    for _ in range(3):
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


def pairs(side, count):
    g = torch.Generator(device=dev).manual_seed(side)
    out = []
    for _ in range(count):
        x = torch.rand(1, 3, side, side, device=dev, generator=g)
        out.append((x, (x + 0.05 * torch.randn(x.shape, device=dev, generator=g)).clamp(0, 1)))
    return out


def main():
    sides = [int(s) for s in sys.argv[1:]] or [512, 2048]
    print(torch.cuda.get_device_name(0), flush=True)
    for side in sides:
        nbytes = 2 * 4 * 3 * side * side
        rot = max(1, -(-(512 << 20) // nbytes))  # pairs that together exceed the Infinity Cache twice over
        ps = pairs(side, rot)
        x, y = ps[0]
        px, py = x.view(-1, 3), y.view(-1, 3)  # the reference's (N, 3) images
        out = torch.empty(2, dtype=torch.float64, device=dev)
        scratch = torch.empty(ops.image_metrics_scratch(n=px.numel(), planes=3, h=side, w=side), dtype=torch.uint8, device=dev)
        k = [0]

        def rotating(fn):
            def call():
                a, b = ps[k[0] % rot]
                k[0] += 1
                fn(a, b)
            return call

        rows = [
            ("psnr", lambda: metrics.psnr(px, py)),
            ("ssim", lambda: metrics.ssim(x, y)),
            ("sse launches", lambda: ops.image_sse(px, py, out=out, scratch=scratch)),
            ("ssim launches", lambda: ops.ssim_sum(x, y, out=out, scratch=scratch)),
            ("sse launches, rotating", rotating(lambda a, b: ops.image_sse(a.view(-1), b.view(-1), out=out, scratch=scratch))),
            ("ssim launches, rotating", rotating(lambda a, b: ops.ssim_sum(a, b, out=out, scratch=scratch))),
        ]
        for name, fn in rows:
            ms = timed(fn)
            print(f"3x{side}x{side} {name}: {ms * 1e3:.1f} us, {nbytes / (ms * 1e-3) / 1e9:.0f} GB/s of image reads", flush=True)
        # the values, so a run also shows what was timed
        print(f"3x{side}x{side} psnr {metrics.psnr(px, py).item():.4f} ssim {metrics.ssim(x, y).item():.6f}", flush=True)


if __name__ == "__main__":
    main()
