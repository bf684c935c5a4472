#!/usr/bin/env python3
"""Generate tests/golden/blender/reference.npz by RUNNING THE REFERENCE's BlenderDataset (datasets/blender.py) and Pillow.

Runs only in the build container (needs /root/reference, read-only, and Pillow).  A tiny synthetic scene -- 3 training and 2
validation frames, 16 x 16 RGBA PNGs whose alpha mixes 0, 255 and partial values, a non-trivial ``camera_angle_x`` and rotations -- is
written to a temporary directory as ``transforms_{train,val}.json`` + PNG files, and ``BlenderDataset(root, split, img_wh=(8, 8))`` runs on
it unmodified.  The module is loaded from its file (the package's ``__init__`` pulls in the satellite loaders' dependencies); its two
absent imports are supplied by a few lines of our own: ``kornia.create_meshgrid`` (pixel coordinates, x then y, unnormalised) and
``torchvision.transforms.ToTensor`` (u8 HWC -> fp32 CHW / 255).

Stored: the inputs (images, angle, matrices), the reference's ``all_rays[:, :8]``, ``all_rays[:, 8]`` and ``all_rgbs``, validation sample
1 (``rays``, ``ts``, ``rgbs``, ``valid_mask``), the Pillow version, and for every shape of ``tests.blender_reference.FIXTURE_SHAPES`` a
seeded RGBA image with Pillow's ``resize(..., Image.LANCZOS)`` of it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_blender_golden.py            # rewrite the fixture
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_blender_golden.py --check    # regenerate and compare bit for bit
"""
import argparse
import importlib.util
import io
import json
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "blender", "reference.npz")
REF = "/root/reference"
N_TRAIN, N_VAL, SRC, WH = 3, 2, 16, 8


def make_scene():
    """The inputs: images (5, 16, 16, 4) uint8, camera_angle_x, transform matrices (5, 4, 4) fp64 (train frames first)."""
    sys.path.insert(0, REPO)
    from tests import blender_reference as B

    g = np.random.default_rng(20241018)
    images = np.stack([B.random_rgba(SRC, SRC, seed=40 + k) for k in range(N_TRAIN + N_VAL)])
    mats = np.zeros((N_TRAIN + N_VAL, 4, 4))
    for m in mats:
        q, _ = np.linalg.qr(g.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        m[:3, :3], m[:3, 3], m[3, 3] = q, g.normal(size=3) * 2.5, 1.0
    return {"images": images, "camera_angle_x": np.float64(0.6911112070083618 + g.uniform(-0.1, 0.1)), "transform_matrix": mats}


def write_scene(root, scene):
    from PIL import Image

    for split, lo, hi in (("train", 0, N_TRAIN), ("val", N_TRAIN, N_TRAIN + N_VAL)):
        frames = []
        for k in range(lo, hi):
            name = f"./{split}/r_{k - lo}"
            os.makedirs(os.path.join(root, split), exist_ok=True)
            Image.fromarray(scene["images"][k], "RGBA").save(os.path.join(root, name + ".png"))
            frames.append({"file_path": name, "transform_matrix": scene["transform_matrix"][k].tolist()})
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": float(scene["camera_angle_x"]), "frames": frames}, f)


def run_reference(root):
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
        spec = importlib.util.spec_from_file_location("reference_blender", os.path.join(REF, "datasets", "blender.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        torch.set_num_threads(1)
        train = mod.BlenderDataset(root, "train", img_wh=(WH, WH))
        val = mod.BlenderDataset(root, "val", img_wh=(WH, WH))
        sample = val[1]
    finally:
        for m, v in saved.items():
            if v is None:
                sys.modules.pop(m, None)
            else:
                sys.modules[m] = v
    assert train.all_rays.shape == (N_TRAIN * WH * WH, 9) and train.all_rgbs.dtype == torch.float32
    return {"all_rays": train.all_rays[:, :8].contiguous().numpy(), "all_ts": train.all_rays[:, 8].contiguous().numpy(),
            "all_rgbs": train.all_rgbs.numpy(), "focal": np.float64(train.focal), "val1_rays": sample["rays"].numpy(),
            "val1_ts": sample["ts"].numpy(), "val1_rgbs": sample["rgbs"].numpy(), "val1_valid_mask": sample["valid_mask"].numpy(),
            "val1_c2w": sample["c2w"].numpy()}


def pillow_cases():
    import PIL
    from PIL import Image

    sys.path.insert(0, REPO)
    from tests import blender_reference as B

    out = {"pillow_version": np.array(PIL.__version__)}
    for k, (h, w, oh, ow) in enumerate(B.FIXTURE_SHAPES):
        src = B.random_rgba(h, w, seed=k)
        out[f"resize{k}_src"] = src
        out[f"resize{k}_out"] = np.asarray(Image.fromarray(src, "RGBA").resize((ow, oh), Image.LANCZOS))
        assert out[f"resize{k}_out"].shape == (oh, ow, 4)
    return out


def npz_bytes(arrays):
    """np.savez_compressed with fixed member timestamps: equal arrays -> equal file bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, b.getvalue())
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--check", action="store_true", help="write nothing: regenerate and compare bit for bit")
    a = ap.parse_args()
    sys.dont_write_bytecode = True
    scene = make_scene()
    with tempfile.TemporaryDirectory() as tmp:
        write_scene(tmp, scene)
        arrays = {**scene, **run_reference(tmp), **pillow_cases()}
    if a.check:
        z = np.load(OUT, allow_pickle=False)
        bad = sorted(set(z.files) ^ set(arrays))
        for k in sorted(set(z.files) & set(arrays)):
            x, y = np.asarray(arrays[k]), z[k]
            if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
                bad.append(k)
        print(f"blender  {'OK: ' + str(len(arrays)) + ' arrays bit-equal' if not bad else 'MISMATCH: ' + ', '.join(bad)}")
        return 1 if bad else 0
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    blob = npz_bytes(arrays)
    with open(OUT, "wb") as f:
        f.write(blob)
    print(f"blender  reference.npz ({len(blob) / 1024:.0f} KiB), {len(arrays)} arrays, Pillow {arrays['pillow_version']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
