"""Restatements for the Blender loader, written from the definitions in include/satrender.h:

* ``resize_rgba``: Pillow's 8-bit Lanczos resize of an RGBA image in integer arithmetic -- premultiply, one pass per axis (horizontal
  first) with 22-bit fixed-point coefficients and an 8-bit intermediate, un-premultiply.  The tables are built tap by tap with
  Python floats (``math.sin``), independently of ``ops.lanczos_tables``' vectorised builder.
* ``blend``: the reference's fp32 ``ToTensor`` and alpha blend onto white (datasets/blender.py:136-139,181-183).
* ``pinhole_rays``: get_ray_directions / get_rays (datasets/blender.py:12-59) in fp64 from the fp32 inputs, rounded once.
"""
import math

import numpy as np

PRECISION_BITS = 22

# (src_h, src_w, out_h, out_w): the shapes whose Pillow bytes tests/golden/blender/reference.npz stores
FIXTURE_SHAPES = [(16, 16, 8, 8), (37, 53, 11, 17), (9, 13, 18, 26), (64, 64, 64, 32), (33, 47, 5, 47)]


def _sinc(x):
    return 1.0 if x == 0.0 else math.sin(math.pi * x) / (math.pi * x)


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


def tables(n_in, n_out):
    """(bounds (n_out, 2) int32 = [xmin, count], coef (n_out, ksize) int32) of one axis."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = 2 * int(math.ceil(support)) + 1
    bounds = np.zeros((n_out, 2), np.int32)
    coef = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), n_in) - xmin
        w = [_lanczos((x + xmin - center + 0.5) / fs) for x in range(count)]
        total = 0.0
        for v in w:
            total += v
        for x, v in enumerate(w):
            v = v / total if total != 0.0 else v
            coef[xx, x] = int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5)
        bounds[xx] = xmin, count
    return bounds, coef


def _resample_axis0(img, n_out):
    """One pass along axis 0 of an (n_in, m, 4) uint8 image: clamp((2^21 + sum pixel * k) >> 22, 0, 255)."""
    bounds, coef = tables(img.shape[0], n_out)
    src = img.astype(np.int64)
    out = np.empty((n_out,) + img.shape[1:], np.uint8)
    for xx in range(n_out):
        xmin, count = bounds[xx]
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(coef[xx, :count].astype(np.int64), src[xmin:xmin + count], 1)
        assert np.abs(acc).max() < 2 ** 31  # what the kernel's int32 accumulators rely on
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def premultiply(rgba):
    a = rgba[..., 3:4].astype(np.int64)
    t = rgba[..., :3].astype(np.int64) * a + 128
    return np.concatenate([(((t >> 8) + t) >> 8).astype(np.uint8), rgba[..., 3:4]], -1)


def unpremultiply(rgba):
    a = rgba[..., 3:4].astype(np.int64)
    c = rgba[..., :3].astype(np.int64)
    q = np.minimum(255 * c // np.maximum(a, 1), 255)
    keep = (a == 0) | (a == 255)
    return np.concatenate([np.where(keep, c, q).astype(np.uint8), rgba[..., 3:4]], -1)


def resize_rgba(rgba, out_h, out_w):
    """(out_h, out_w, 4) uint8: ``Image.fromarray(rgba, "RGBA").resize((out_w, out_h), Image.LANCZOS)``."""
    rgba = np.asarray(rgba)
    assert rgba.dtype == np.uint8 and rgba.ndim == 3 and rgba.shape[2] == 4
    h, w = rgba.shape[:2]
    if (out_h, out_w) == (h, w):
        return rgba.copy()
    img = premultiply(rgba)
    if out_w != w:
        img = np.swapaxes(_resample_axis0(np.swapaxes(img, 0, 1), out_w), 0, 1)
    if out_h != h:
        img = _resample_axis0(img, out_h)
    return unpremultiply(np.ascontiguousarray(img))


def blend(rgba):
    """((n, 3) fp32 colours, (n,) bool valid_mask) of an (h, w, 4) uint8 image: v = u8 / 255 in fp32, v_c * v_a + (1 - v_a) with
    every operation rounded to fp32."""
    v = rgba.reshape(-1, 4).astype(np.float32) / np.float32(255)
    a = v[:, 3:4]
    rgbs = v[:, :3] * a + (np.float32(1) - a)
    assert rgbs.dtype == np.float32
    return rgbs, rgba.reshape(-1, 4)[:, 3] > 0


def pinhole_rays(h, w, fx, fy, cx, cy, c2w, near, far):
    """(h * w, 8) fp32 rows [o, d, near, far]: the direction in fp64 from the fp32 inputs, rounded to fp32 once."""
    fx, fy, cx, cy = (float(np.float32(v)) for v in (fx, fy, cx, cy))
    m = np.asarray(c2w, np.float32).reshape(3, 4).astype(np.float64)
    r, c = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    dx, dy = (c - cx) / fx, -((r - cy) / fy)
    wk = [(dx * m[k, 0] + dy * m[k, 1]) + (-1.0) * m[k, 2] for k in range(3)]
    n = np.sqrt((wk[0] * wk[0] + wk[1] * wk[1]) + wk[2] * wk[2])
    out = np.empty((h * w, 8), np.float32)
    out[:, :3] = m[:, 3].astype(np.float32)
    for k in range(3):
        out[:, 3 + k] = (wk[k] / n).reshape(-1).astype(np.float32)
    out[:, 6], out[:, 7] = np.float32(near), np.float32(far)
    return out


def random_rgba(h, w, seed=0):
    """Seeded (h, w, 4) uint8 noise whose alpha is 0, 255 or noise over a 3 x 3 arrangement of blocks, so that a resized image keeps
    transparent, opaque and partial pixels (both un-premultiply branches) and crosses every kind of edge."""
    g = np.random.default_rng([seed, h, w])
    img = g.integers(0, 256, (h, w, 4), dtype=np.uint8)
    kind = (np.arange(h)[:, None] * 3 // h + np.arange(w)[None, :] * 3 // w + seed) % 3
    img[..., 3] = np.where(kind == 0, 0, np.where(kind == 1, 255, img[..., 3]))
    return img


def focal(camera_angle_x, width):
    """read_meta's focal length (datasets/blender.py:105-108)."""
    return (400.0 / np.tan(camera_angle_x / 2)) * (width / 800)  # the 800-pixel focal length first, then the scale to ``width``


def blender_colors_stub(calls):
    """Stands in for ``ops.blender_colors`` on the host: the restatement on a CPU tensor; records (H, W, out_h, out_w, layout)."""
    import torch

    def stub(image_u8, out_h, out_w, out=None, layout=None, want_rgba=False):
        img = image_u8.numpy()
        hwc = img if layout == "hwc" else np.transpose(img, (1, 2, 0))
        calls.append(hwc.shape[:2] + (out_h, out_w, layout))
        small = resize_rgba(hwc, out_h, out_w)
        rgbs, mask = blend(small)
        if out is None:
            out = torch.empty(out_h * out_w, 3)
        out.copy_(torch.from_numpy(rgbs))
        res = (out, torch.from_numpy(mask.copy()))
        return res + (torch.from_numpy(small),) if want_rgba else res

    return stub


def pinhole_rays_stub(calls):
    """Stands in for ``ops.pinhole_rays`` on the host; records (h, w, fx, cx, cy)."""
    import torch

    def stub(h, w, fx, fy, cx, cy, c2w, near, far, out=None):
        calls.append((h, w, fx, cx, cy))
        rays = torch.from_numpy(pinhole_rays(h, w, fx, fy, cx, cy, c2w, near, far))
        if out is None:
            return rays
        out.copy_(rays)
        return out

    return stub


def write_scene(root, z, reader_images, n_val=None):
    """The fixture's scene (reference.npz ``z``) as ``transforms_{train,val}.json`` under ``root``; the frames' image paths are mapped to
    their (16, 16, 4) arrays in ``reader_images`` for a ``reader=`` that serves them.  ``n_val``: list the two validation frames
    cyclically up to that many."""
    import json
    import os

    n_train = z["all_rays"].shape[0] // 64
    n_all = z["images"].shape[0]
    val = list(range(n_train, n_all))
    if n_val is not None:
        val = [val[k % len(val)] for k in range(n_val)]
    for split, idx in (("train", range(n_train)), ("val", val)):
        frames = []
        for j, k in enumerate(idx):
            name = f"./{split}/r_{j}"
            reader_images[os.path.join(root, name + ".png")] = z["images"][k]
            frames.append({"file_path": name, "transform_matrix": z["transform_matrix"][k].tolist()})
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": float(z["camera_angle_x"]), "frames": frames}, f)
