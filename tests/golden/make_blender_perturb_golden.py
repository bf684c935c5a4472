#!/usr/bin/env python3
"""Generate tests/golden/blender_perturb/reference.npz by RUNNING THE REFERENCE's ``add_perturbation`` and
``BlenderDataset(..., perturbation=...)`` (datasets/blender.py:61-209) under Pillow.

Runs only in the build container, like make_blender_golden.py, whose reference location and npz writer it shares; the reference module
is loaded from its file with the same two stand-ins for its absent imports (``kornia.create_meshgrid``, ``torchvision``'s ``ToTensor``).

No input image is stored: every one is ``tests.blender_perturb_reference.pattern_rgba``, a closed integer formula.  Stored:

* per case, indexed [size, seed, variant] in the order of ``SIZES``, ``SEEDS`` and ``VARIANTS`` of ``tests.blender_perturb_reference``
  (the input is frame ``seed`` of the formula): ``hash_in`` [size, seed] and ``hash_out``, the SHA-256 of the input bytes and of the
  reference's perturbed bytes; ``crops`` (..., 5, 6, 6, 4), windows of the perturbed image at the strip's four corners and at the
  column rectangles 0 and 1 share (zero where a window leaves the image); ``touched``, the number of pixels the reference changed;
* per seed ``s``, ``b``, ``left``, ``top``, ``colours``: what the reference draws, from numpy's global generator in its order of calls;
* the scene: four 416 x 416 training and two validation frames (frames 40..45 of the formula), ``camera_angle_x`` and
  ``transform_matrix``; per variant the reference's ``all_rgbs`` and ``all_rays[:, 8]`` at img_wh = (24, 24), sample 2 of its
  ``test_train`` split (``rgbs`` and ``valid_mask`` per variant; ``rays``, ``ts``, ``c2w``, ``original_rgbs`` and
  ``original_valid_mask``, which every variant gives alike, once), and the key list of ``test_train`` sample 0 with and without a
  perturbation.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_blender_perturb_golden.py            # rewrite the fixture
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_blender_perturb_golden.py --check    # regenerate and compare bit for bit
"""
import argparse
import contextlib
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "blender_perturb", "reference.npz")
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
import make_blender_golden as G  # noqa: E402
from tests import blender_perturb_reference as P  # noqa: E402


@contextlib.contextmanager
def reference_module():
    """datasets/blender.py of the reference, loaded from its file with the two stand-ins in place."""
    import torch

    def create_meshgrid(height, width, normalized_coordinates=True):
        assert normalized_coordinates is False
        xs, ys = torch.linspace(0, width - 1, width), torch.linspace(0, height - 1, height)
        return torch.stack(torch.meshgrid(xs, ys, indexing="xy"), -1)[None]  # (1, H, W, 2), x then y

    class ToTensor:
        def __call__(self, pic):
            a = np.asarray(pic)
            assert a.dtype == np.uint8 and a.ndim == 3
            return torch.from_numpy(a.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    kornia = types.ModuleType("kornia")
    kornia.create_meshgrid = create_meshgrid
    tv, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tvt.ToTensor, tv.transforms = ToTensor, tvt
    stubs = {"kornia": kornia, "torchvision": tv, "torchvision.transforms": tvt}
    saved = {m: sys.modules.get(m) for m in stubs}
    sys.modules.update(stubs)
    try:
        spec = importlib.util.spec_from_file_location("reference_blender", os.path.join(G.REF, "datasets", "blender.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        torch.set_num_threads(1)
        yield mod
    finally:
        for m, v in saved.items():
            if v is None:
                sys.modules.pop(m, None)
            else:
                sys.modules[m] = v


def drawn(seed):
    """What add_perturbation draws for ``seed``, from numpy's global generator in the reference's order of calls."""
    np.random.seed(seed)
    s = np.random.uniform(0.8, 1.2, size=3)
    b = np.random.uniform(-0.2, 0.2, size=3)
    np.random.seed(seed)
    left = np.random.randint(200, 400)
    top = np.random.randint(200, 400)
    colours = []
    for i in range(10):
        np.random.seed(10 * seed + i)
        colours.append(tuple(np.random.choice(range(256), 3)))
    return {"s": s, "b": b, "left": np.int64(left), "top": np.int64(top), "colours": np.array(colours, np.uint8)}


def cases(mod):
    from PIL import Image

    per_seed = [drawn(seed) for seed in P.SEEDS]
    out = {k: np.stack([d[k] for d in per_seed]) for k in per_seed[0]}
    n = (len(P.SIZES), len(P.SEEDS), len(P.VARIANTS))
    out.update(hash_in=np.zeros(n[:2] + (32,), np.uint8), hash_out=np.zeros(n + (32,), np.uint8),
               crops=np.zeros(n + (5, P.CROP, P.CROP, 4), np.uint8), touched=np.zeros(n, np.int64))
    for i, (h, w) in enumerate(P.SIZES):
        for j, seed in enumerate(P.SEEDS):
            src = P.pattern_rgba(h, w, frame=seed)
            for band in range(4):
                assert len(np.unique(src[..., band])) == 256, (h, w, seed, band)  # every byte value in every band
            blocks = src[:h // 32 * 32, :w // 32 * 32, 3].reshape(h // 32, 32, w // 32, 32)
            assert (blocks == 0).all((1, 3)).any() and (blocks == 255).all((1, 3)).any()  # runs of 0 and of 255
            out["hash_in"][i, j] = P.sha256(src)
            for k, variant in enumerate(P.VARIANTS):
                got = np.asarray(mod.add_perturbation(Image.fromarray(src, "RGBA"), list(variant), seed))
                assert got.shape == src.shape and got.dtype == np.uint8
                out["hash_out"][i, j, k] = P.sha256(got)
                out["crops"][i, j, k] = P.crops(got, int(out["left"][j]), int(out["top"][j]))
                out["touched"][i, j, k] = (got != src).any(-1).sum()
    return out


def make_scene():
    g_angle = 0.6911112070083618
    mats = np.zeros((P.SCENE_TRAIN + P.SCENE_VAL, 4, 4))
    for k, m in enumerate(mats):  # rotations about two axes by fixed angles, and an origin on a ring of radius 4
        a, e = 0.7 * k + 0.3, 0.25 * k - 0.4
        ra = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        re = np.array([[1, 0, 0], [0, np.cos(e), -np.sin(e)], [0, np.sin(e), np.cos(e)]])
        m[:3, :3], m[:3, 3], m[3, 3] = ra @ re, (4 * np.cos(a), 4 * np.sin(a), 1.0 + 0.5 * k), 1.0
    return {"camera_angle_x": np.float64(g_angle), "transform_matrix": mats}


def scene(mod):
    from PIL import Image

    out = make_scene()
    images = P.scene_images()
    wh = (P.SCENE_WH, P.SCENE_WH)
    with tempfile.TemporaryDirectory() as root:
        for split, lo, hi in (("train", 0, P.SCENE_TRAIN), ("val", P.SCENE_TRAIN, P.SCENE_TRAIN + P.SCENE_VAL)):
            frames = []
            os.makedirs(os.path.join(root, split))
            for k in range(lo, hi):
                name = f"./{split}/r_{k - lo}"
                Image.fromarray(images[k], "RGBA").save(os.path.join(root, name + ".png"))
                frames.append({"file_path": name, "transform_matrix": out["transform_matrix"][k].tolist()})
            with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
                json.dump({"camera_angle_x": float(out["camera_angle_x"]), "frames": frames}, f)
        with contextlib.redirect_stdout(open(os.devnull, "w")):
            clean = mod.BlenderDataset(root, "test_train", img_wh=wh)
            out["test_train0_keys_clean"] = np.array(sorted(clean[0]))
            for variant in P.VARIANTS:
                v = "+".join(variant)
                train = mod.BlenderDataset(root, "train", img_wh=wh, perturbation=list(variant))
                assert train.all_rays.shape == (P.SCENE_TRAIN * P.SCENE_WH ** 2, 9)
                out[f"{v}_all_rgbs"], out[f"{v}_all_ts"] = train.all_rgbs.numpy(), train.all_rays[:, 8].contiguous().numpy()
                tt = mod.BlenderDataset(root, "test_train", img_wh=wh, perturbation=list(variant))
                out["test_train0_keys_perturbed"] = np.array(sorted(tt[0]))
                for k, t in tt[2].items():  # what does not depend on the variant is stored once
                    shared = k in ("rays", "c2w", "ts", "original_rgbs", "original_valid_mask")
                    key = f"tt2_{k}" if shared else f"{v}_tt2_{k}"
                    assert key not in out or (shared and out[key].tobytes() == t.numpy().tobytes()), key
                    out[key] = t.numpy()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--check", action="store_true", help="write nothing: regenerate and compare bit for bit")
    a = ap.parse_args()
    import PIL

    with reference_module() as mod:
        arrays = {"pillow_version": np.array(PIL.__version__), **cases(mod), **scene(mod)}
    if a.check:
        z = np.load(OUT, allow_pickle=False)
        bad = sorted(set(z.files) ^ set(arrays))
        for k in sorted(set(z.files) & set(arrays)):
            x, y = np.asarray(arrays[k]), z[k]
            if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
                bad.append(k)
        print(f"blender_perturb  {'OK: ' + str(len(arrays)) + ' arrays bit-equal' if not bad else 'MISMATCH: ' + ', '.join(bad)}")
        return 1 if bad else 0
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    blob = G.npz_bytes(arrays)
    with open(OUT, "wb") as f:
        f.write(blob)
    print(f"blender_perturb  reference.npz ({len(blob) / 1024:.0f} KiB), {len(arrays)} arrays, Pillow {arrays['pillow_version']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
