"""Restatements for the Blender perturbations, written from the definition of ``sr_blender_perturb`` in
include/satrender.h and of ``add_perturbation`` in the reference (datasets/blender.py:61-79):

* ``pattern_rgba``: the tests' input images, a closed integer formula of (row, column, band, frame) -- no random generator, so every
  numpy gives the same bytes.  Every band takes all 256 byte values; alpha has blocks of 0, of 255 and of everything between.
* ``params``: s, b, left, top and the ten colours of one seed, from ``np.random.RandomState``.
* ``color_lut`` / ``occluders``: the (4, 256) byte table and the ten inclusive rectangles with their RGBA fills.
* ``perturb``: the table, then the rectangles clipped to the image in order (the last match wins), on an (H, W, 4) array.
* ``blender_perturb_stub``: stands in for ``ops.blender_perturb`` on the host.
"""
import hashlib

import numpy as np

SIZES = [(416, 416), (333, 417), (800, 800), (100, 120), (230, 611)]  # (h, w) of the fixture's cases
SEEDS = [1, 2, 3, 17, 99]
VARIANTS = [("color",), ("occ",), ("color", "occ")]
CROP = 6  # side of a stored crop: rows y - 3 .. y + 2, columns x - 3 .. x + 2 around a point (y, x)
SCENE_SRC, SCENE_WH, SCENE_TRAIN, SCENE_VAL = 416, 24, 4, 2


def pattern_rgba(h, w, frame=0):
    """(h, w, 4) uint8.  Colour band k: (7 r + 13 c + 85 k + 29 frame + (r c >> 4)) mod 256.  Alpha by 32 x 32 blocks, kind =
    (r // 32 + c // 32 + frame) mod 3: 0 -> 0, 1 -> 255, 2 -> (5 r + 3 c + 11 frame) mod 256."""
    r, c = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    img = np.empty((h, w, 4), np.uint8)
    for k in range(3):
        img[..., k] = (7 * r + 13 * c + 85 * k + 29 * frame + ((r * c) >> 4)) & 255
    kind = (r // 32 + c // 32 + frame) % 3
    img[..., 3] = np.where(kind == 0, 0, np.where(kind == 1, 255, (5 * r + 3 * c + 11 * frame) & 255))
    return img


def sha256(a):
    """The digest of an array's bytes in C order, as (32,) uint8."""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def params(seed):
    """{"s" (3,), "b" (3,), "left", "top", "colours" (10, 3) uint8}: what both perturbations draw for ``seed``; each reseeds."""
    g = np.random.RandomState(seed)
    s, b = g.uniform(0.8, 1.2, size=3), g.uniform(-0.2, 0.2, size=3)
    g = np.random.RandomState(seed)
    left, top = g.randint(200, 400), g.randint(200, 400)
    colours = np.array([np.random.RandomState(10 * seed + i).choice(range(256), 3) for i in range(10)]).astype(np.uint8)
    return {"s": s, "b": b, "left": int(left), "top": int(top), "colours": colours}


def color_lut(s, b):
    """(4, 256) uint8: band k's byte v -> uint8(255 * clip(s_k * (v / 255.0) + b_k, 0, 1)) in fp64; alpha -> uint8(255 * (v / 255.0))."""
    lut = np.empty((4, 256), np.uint8)
    for v in range(256):
        x = v / 255.0
        for k in range(3):
            lut[k, v] = int(255 * min(max(float(s[k]) * x + float(b[k]), 0.0), 1.0))
        lut[3, v] = int(255 * x)
    return lut


def occluders(left, top, colours):
    """(rects (10, 4) int32 [x0, y0, x1, y1] with both corners inside, fills (10, 4) uint8 with alpha 255)."""
    rects = np.array([[left + 20 * i, top, left + 20 * (i + 1), top + 200] for i in range(10)], np.int32)
    fills = np.concatenate([np.asarray(colours, np.uint8), np.full((10, 1), 255, np.uint8)], 1)
    return rects, fills


def perturb(img, lut=None, rects=None, fills=None):
    """A new (H, W, 4) uint8 array: ``lut`` on every band, then each rectangle in order, clipped to the image."""
    out = np.array(img, copy=True)
    h, w = out.shape[:2]
    if lut is not None:
        for k in range(4):
            out[..., k] = np.asarray(lut)[k][out[..., k]]
    if rects is not None:
        for (x0, y0, x1, y1), fill in zip(np.asarray(rects).tolist(), np.asarray(fills)):
            x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)
            if x0 <= x1 and y0 <= y1:
                out[y0:y1 + 1, x0:x1 + 1] = fill
    return out


def host_parameters(seed, variant):
    """(lut, rects, fills) of one seed and variant, the parts the variant does not name None."""
    p = params(seed)
    lut = color_lut(p["s"], p["b"]) if "color" in variant else None
    rects, fills = occluders(p["left"], p["top"], p["colours"]) if "occ" in variant else (None, None)
    return lut, rects, fills


def perturbed(img, seed, variant):
    """The restatement of ``add_perturbation(img, variant, seed)``."""
    return perturb(img, *host_parameters(seed, variant))


def crop_points(left, top):
    """(y, x) of the stored crops: the strip's four corners (rectangle 0's left edge, rectangle 9's right edge) and the column that
    rectangles 0 and 1 share, at the top."""
    return [(top, left), (top, left + 200), (top + 200, left), (top + 200, left + 200), (top, left + 20)]


def crops(img, left, top):
    """(5, CROP, CROP, 4) uint8: the windows of ``crop_points`` cut from ``img``, zero where a window leaves the image."""
    h, w = img.shape[:2]
    out = np.zeros((5, CROP, CROP, 4), np.uint8)
    for k, (y, x) in enumerate(crop_points(left, top)):
        y0, x0 = y - CROP // 2, x - CROP // 2
        ya, yb, xa, xb = max(y0, 0), min(y0 + CROP, h), max(x0, 0), min(x0 + CROP, w)
        if ya < yb and xa < xb:
            out[k, ya - y0:yb - y0, xa - x0:xb - x0] = img[ya:yb, xa:xb]
    return out


def blender_perturb_stub(calls):
    """Stands in for ``ops.blender_perturb`` on the host: the restatement on a CPU tensor; records (layout, has lut, number of
    rectangles, in place)."""
    import torch

    def stub(image_u8, lut=None, rects=None, fills=None, layout=None, out=None):
        img = image_u8.numpy()
        hwc = img if layout == "hwc" else np.transpose(img, (1, 2, 0))
        calls.append((layout, lut is not None, 0 if rects is None else len(rects), out is image_u8))
        res = perturb(hwc, lut, rects, fills)
        res = torch.from_numpy(np.ascontiguousarray(res if layout == "hwc" else np.transpose(res, (2, 0, 1))))
        if out is None:
            return res
        out.copy_(res)
        return out

    return stub


def scene_images():
    """The fixture scene's frames, (SCENE_TRAIN + SCENE_VAL, 416, 416, 4): training frames first."""
    return np.stack([pattern_rgba(SCENE_SRC, SCENE_SRC, frame=40 + k) for k in range(SCENE_TRAIN + SCENE_VAL)])


def write_scene(root, z, reader_images):
    """The fixture's scene (reference.npz ``z``: camera angle and matrices; the images come from ``scene_images``) as
    ``transforms_{train,val}.json`` under ``root``; image paths are mapped to their arrays in ``reader_images``."""
    import json
    import os

    images = scene_images()
    for split, idx in (("train", range(SCENE_TRAIN)), ("val", range(SCENE_TRAIN, SCENE_TRAIN + SCENE_VAL))):
        frames = []
        for j, k in enumerate(idx):
            name = f"./{split}/r_{j}"
            reader_images[os.path.join(root, name + ".png")] = images[k]
            frames.append({"file_path": name, "transform_matrix": z["transform_matrix"][k].tolist()})
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": float(z["camera_angle_x"]), "frames": frames}, f)
