"""Blender loading timings (median of 10 rounds after a warm-up, the legs interleaved round by round) for one
procedurally generated 800 x 800 RGBA image resized to 400 x 400, the reference's default img_wh:
  horizontal pass   sr_blender_colors stopped after its first launch (stages = 1), the bytes already on the device (HIP events around 500
                    back-to-back calls, per call)
  both passes       sr_blender_colors, everything: horizontal, vertical + un-premultiply + blend (the same; vertical = the difference)
  pinhole rays      sr_pinhole_rays for the 400 x 400 grid (the same)
  blender_colors_from_image  the host array to the finished device rows: the 4-byte-per-pixel upload, the scratch and output
                    allocations and both launches (host clock over 50 calls, each ending in a device synchronise)
  blender_rays      the same for data.blender_rays
  reference path    what the reference does on the host after the PNG decode (datasets/blender.py:136-139), restated: Pillow's
                    resize(LANCZOS), the bytes scaled to fp32 [0, 1], the blend onto white in torch on the CPU, and the upload of the
                    (h*w, 3) rows (host clock over 5 calls; torch's CPU threads as configured)
  perturb ...       sr_blender_perturb on the 800 x 800 frame in place, the bytes already on the device (HIP events, as above): the colour
                    table alone, the ten occluders alone, both (seed 3: the strip lies inside, 40,401 pixels)
  blender_colors_from_image perturbed  the same as blender_colors_from_image with perturb = both: one more launch on the uploaded bytes
  reference perturbation  add_perturbation (datasets/blender.py:61-79) on the host, restated with the draws made beforehand: numpy's
                    fp64 scale, clip and cast of the whole frame, then Pillow's ten rectangles (host clock over 5 calls)
  reference rays    its rays (:51-59,142-149), restated: fp32 torch on the CPU rotates and normalises precomputed camera-frame
                    directions, attaches origin, near and far, and uploads the rows (host clock over 50 calls)
Usage: bench_blender.py"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from satnerf_amd import _lib, data, ops  # noqa: E402

dev = "cuda:0"
SRC, OUT = 800, 400
ROUNDS, REPS = 10, 500  # a kernel window is 500 back-to-back calls (4-8 ms)
HOST_REPS = {"fast": 50, "slow": 5}  # calls per host-clock window: 2-8 ms for the package's legs, ~40 ms for the host path


def event_ms(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def host_ms(fn, reps):
    """Per call, over ``reps`` calls each ending in a device synchronise (a load hands finished rows back)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def scene_image(n):
    """A rendered-object look-alike: a shaded disc with a soft edge on a transparent background, plus texture noise."""
    y, x = np.mgrid[0:n, 0:n].astype(np.float64) / n - 0.5
    r = np.hypot(x, y)
    g = np.random.default_rng(3)
    rgb = np.clip(128 + 100 * np.stack([np.sin(9 * x), np.cos(7 * y), np.sin(5 * (x + y))], -1) + g.normal(0, 12, (n, n, 3)), 0, 255)
    alpha = np.clip((0.35 - r) / 0.01, 0, 1) * 255
    return np.concatenate([rgb, alpha[..., None]], -1).astype(np.uint8)


def host_colors(pil_img):
    """The host's way to the same rows: Pillow resizes, torch on the CPU scales the bytes to [0, 1] and composites over white."""
    from PIL import Image

    resized = np.asarray(pil_img.resize((OUT, OUT), Image.LANCZOS))
    rgba = torch.from_numpy(resized.copy()).movedim(2, 0).contiguous().to(torch.float32).div(255)  # planar fp32, as ToTensor leaves it
    rows = rgba.reshape(4, OUT * OUT).t()
    alpha = rows[:, 3:]
    return (rows[:, :3] * alpha + (1 - alpha)).to(dev)


def host_perturbation(pil_img, s, b, rects, fills):
    """The host's way to the perturbed frame: numpy scales, clips and casts in fp64, Pillow draws the rectangles."""
    from PIL import Image, ImageDraw

    x = np.array(pil_img) / 255.0
    x[..., :3] = np.clip(s * x[..., :3] + b, 0, 1)
    img = Image.fromarray((255 * x).astype(np.uint8))
    draw = ImageDraw.Draw(img)
    for (x0, y0, x1, y1), fill in zip(rects, fills):
        draw.rectangle(((x0, y0), (x1, y1)), fill=tuple(fill[:3]))
    return img


def host_rays(cam_dirs, pose):
    """The host's way to the same rows in fp32 torch: rotate the camera-frame directions, normalise, attach origin, near and far."""
    rot, origin = pose[:, :3], pose[:, 3]
    world = torch.nn.functional.normalize(torch.matmul(cam_dirs, rot.t()), dim=-1).reshape(-1, 3)
    n = world.shape[0]
    return torch.cat([origin.expand(n, 3), world, torch.full((n, 1), 2.0), torch.full((n, 1), 6.0)], 1).to(dev)


def main():
    print("device:", torch.cuda.get_device_name(0), "| torch CPU threads:", torch.get_num_threads(), f"| {ROUNDS} rounds; {REPS} calls per kernel window, {HOST_REPS} per host window")
    img = scene_image(SRC)
    on_dev = torch.from_numpy(img).to(dev)
    coef, ksize = ops._lanczos_device(SRC, OUT, on_dev.device)
    nbytes = ops.blender_colors_scratch(SRC, SRC, OUT, OUT)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rgbs = torch.empty(OUT * OUT, 3, device=dev)
    mask = torch.empty(OUT * OUT, dtype=torch.bool, device=dev)
    rays = torch.empty(OUT * OUT, 8, device=dev)
    focal = 400.0 / np.tan(0.6911112070083618 / 2) * (OUT / 800)  # the Lego scene's camera angle
    c2w = np.array([[-0.9999, 0.0042, -0.0133, -0.0538], [-0.0140, -0.2997, 0.9539, 3.8455], [0.0, 0.9540, 0.2997, 1.2081]], np.float32)
    c2w_c = c2w.ctypes.data_as(C.POINTER(C.c_float))
    pix = torch.arange(OUT, dtype=torch.float32)  # the camera-frame directions, made once per scene and not timed
    directions = torch.empty(OUT, OUT, 3)
    directions[..., 0] = ((pix - OUT / 2) / focal)[None, :]
    directions[..., 1] = (-(pix - OUT / 2) / focal)[:, None]
    directions[..., 2] = -1.0
    c2w_t = torch.from_numpy(c2w)

    def colors(stages):
        _lib.call("sr_blender_colors", ops._p(on_dev), SRC, SRC, 4 * SRC, 4, 1, OUT, OUT, ops._p(coef), ksize, ops._p(coef), ksize,
                  ops._p(scratch), nbytes, ops._p(rgbs), ops._p(mask), None, stages, ops._stream())

    def pinhole():
        _lib.call("sr_pinhole_rays", OUT, OUT, focal, focal, OUT / 2, OUT / 2, c2w_c, 2.0, 6.0, ops._p(rays), ops._stream())

    lut, rects, fills = data.blender_perturbation(3, ["color", "occ"])
    frame = on_dev.clone()  # perturbed in place over and over: the time does not depend on the bytes

    def perturb(lut, rects, fills):
        _lib.call("sr_blender_perturb", ops._p(frame), ops._p(frame), SRC, SRC, 4 * SRC, 4, 1, None if lut is None else lut.ctypes.data,
                  None if rects is None else rects.ctypes.data, None if rects is None else fills.ctypes.data, 0 if rects is None else len(rects),
                  ops._stream())

    legs = {
        "horizontal pass": lambda: event_ms(lambda: colors(1)),
        "both passes": lambda: event_ms(lambda: colors(0)),
        "pinhole rays": lambda: event_ms(pinhole),
        "perturb colour": lambda: event_ms(lambda: perturb(lut, None, None)),
        "perturb occluders": lambda: event_ms(lambda: perturb(None, rects, fills)),
        "perturb both": lambda: event_ms(lambda: perturb(lut, rects, fills)),
        "blender_colors_from_image perturbed": lambda: host_ms(
            lambda: data.blender_colors_from_image(img, OUT, OUT, device=dev, out=rgbs, perturb=(lut, rects, fills)), HOST_REPS["fast"]),
        "blender_colors_from_image": lambda: host_ms(lambda: data.blender_colors_from_image(img, OUT, OUT, device=dev, out=rgbs), HOST_REPS["fast"]),
        "blender_rays": lambda: host_ms(lambda: data.blender_rays(OUT, OUT, focal, c2w, device=dev, out=rays), HOST_REPS["fast"]),
    }
    try:
        from PIL import Image

        pil_img = Image.fromarray(img, "RGBA")
        legs["reference path"] = lambda: host_ms(lambda: host_colors(pil_img), HOST_REPS["slow"])
        g = np.random.RandomState(3)
        s, b = g.uniform(0.8, 1.2, size=3), g.uniform(-0.2, 0.2, size=3)
        legs["reference perturbation"] = lambda: host_ms(lambda: host_perturbation(pil_img, s, b, rects.tolist(), fills.tolist()), HOST_REPS["slow"])
    except ImportError:
        print("Pillow is not installed: the reference's colour path is not timed")
    legs["reference rays"] = lambda: host_ms(lambda: host_rays(directions, c2w_t), HOST_REPS["fast"])
    t = {k: [] for k in legs}
    for r in range(ROUNDS + 1):  # round 0 warms every leg up
        for k, fn in legs.items():
            ms = fn()
            if r:
                t[k].append(ms)
    print(f"{SRC} x {SRC} RGBA -> {OUT} x {OUT}: {4 * SRC * SRC / 1e6:.2f} MB in, {nbytes / 1e6:.2f} MB scratch written and read, "
          f"{(12 + 1) * OUT * OUT / 1e6:.2f} MB out; rays {32 * OUT * OUT / 1e6:.2f} MB out", flush=True)
    for k, v in t.items():
        print(f"  {k}: median {np.median(v):.4f} ms, min {min(v):.4f}, max {max(v):.4f}", flush=True)
    print(f"  vertical pass (both - horizontal, medians): {np.median(t['both passes']) - np.median(t['horizontal pass']):.4f} ms", flush=True)
    if "reference path" in legs:
        theirs = host_colors(pil_img)
        ours, _ = data.blender_colors_from_image(img, OUT, OUT, device=dev)
        print(f"  colours equal to the reference path bit for bit: {torch.equal(ours, theirs)}", flush=True)
        theirs = torch.from_numpy(np.asarray(host_perturbation(pil_img, s, b, rects.tolist(), fills.tolist())).copy())
        ours = ops.blender_perturb(on_dev, lut, rects, fills).cpu()
        print(f"  perturbed bytes equal to the reference perturbation: {torch.equal(ours, theirs)} "
              f"({SRC} x {SRC}: {8 * SRC * SRC / 1e6:.2f} MB read and written per launch)", flush=True)
    print(f"  max |rays - reference rays| = {(data.blender_rays(OUT, OUT, focal, c2w, device=dev) - host_rays(directions, c2w_t)).abs().max().item():.2e}",
          flush=True)


if __name__ == "__main__":
    main()
