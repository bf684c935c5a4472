"""Writes tests/golden/image_products/reference.npz.  Two parts:

``build_fill()`` needs scipy only: the fill fixtures of tests/image_products_reference.py and scipy's griddata(method="nearest")
output for each, with the scipy and numpy versions that recorded them.  tests/test_image_products_host.py reruns it where scipy is
installed.

``record_reference(reference_dir)`` RUNS THE REFERENCE: it imports study_solar_interpolation.py and train_utils.py from a checkout of
the reference and calls hstack_dsm_tifs_v1, hstack_sun_tifs, hstack_rgb_tifs and visualize_depth on seeded images, recording the bytes
they return.  The modules they import for other purposes (rasterio, cv2, rpcm, torchvision, the reference's dataset and evaluation
modules) are replaced by stand-ins: ``rasterio.open`` hands out the seeded arrays, and the OpenCV colour map is the identity
(index -> (index, index, index)), so what is recorded is the byte index the reference computes under this numpy, for the four
combinations of given / measured bounds, after its own crop and its own scipy fill.  The images' holes are a whole column of the crop
window, so each filled pixel has a single nearest neighbour and scipy's choice among equidistant pixels cannot show.

Usage: python tests/golden/make_image_products_golden.py /path/to/reference   (without the path: the fill part alone is refreshed and
the recorded reference arrays already in the file are kept)"""
import contextlib
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import image_products_reference as IP  # noqa: E402

OUT = os.path.join(HERE, "image_products", "reference.npz")


def griddata_nearest(img):
    """scipy's nearest-neighbour interpolation of the NaN pixels from the others, points as (x, y) = (column, row)."""
    from scipy.interpolate import griddata

    valid = ~np.isnan(img)
    out = img.copy()
    out[~valid] = griddata(np.argwhere(valid)[:, ::-1], img[valid], np.argwhere(~valid)[:, ::-1], method="nearest")
    return out


def build_fill():
    import scipy

    data = {"scipy_version": np.array(scipy.__version__), "numpy_version": np.array(np.__version__)}
    for name, (fraction, seed) in IP.FIXTURES.items():
        img = IP.fixture_image(fraction, seed)
        data[name + "_image"] = img
        data[name + "_scipy"] = griddata_nearest(img).astype(np.float32)
    return data


def color_images():
    """name -> (h, w) fp32 images for the colouring: three scales around 100 (wider than the given bounds), a constant image and one
    whose range is of the order of the 1e-8 added to it (given bounds 1e-9 and 1.2e-8 there).  Column w // 4 -- the first of the crop window -- is NaN in the first two."""
    rng = np.random.default_rng(5)
    images = {}
    for name, shape, scale in (("wide", (37, 53), 30.0), ("narrow", (20, 28), 1e-3), ("large", (16, 16), 1e4)):
        images[name] = (rng.standard_normal(shape) * scale + 100).astype(np.float32)
    images["wide"][:, 53 // 4] = np.nan
    images["narrow"][:, 28 // 4] = np.nan
    images["constant"] = np.full((8, 12), 12.5, np.float32)
    # here fp32(fp32(ma - mi) + 1e-8f) and the fp64 sum rounded once differ, and the second value's byte with them (133 / 132)
    images["tiny"] = np.tile(np.array([0.0, 1.298884377831655e-08, 1.1990259451977181e-08, 2.9e-9], np.float32), (4, 2))
    return images


def depth_images():
    rng = np.random.default_rng(6)
    plain = (rng.random((9, 11)) * 40).astype(np.float32)
    plain[2, 3] = plain[8, 10] = np.nan
    with_inf = plain.copy()
    with_inf[4, 4] = np.inf
    return {"nan": plain, "inf": with_inf}


def _module(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _load_reference(reference_dir, images):
    """Import the two reference modules with stand-ins for what they import but these functions do not need; ``images``: path -> (C, H,
    W) array that the stand-in rasterio.open(path).read() returns."""

    class _File:
        def __init__(self, path):
            self.path = path

        def read(self):
            return images[self.path].copy()

    @contextlib.contextmanager
    def open_(path):
        yield _File(path)

    identity = _module("cv2", COLORMAP_JET=2, COLORMAP_VIRIDIS=16, COLOR_BGR2RGB=4, applyColorMap=lambda x, cmap: np.dstack([x, x, x]),
                       cvtColor=lambda x, code: x)
    transforms = _module("torchvision.transforms", ToTensor=lambda: (lambda img: np.asarray(img)))
    nothing = lambda *a, **k: None  # noqa: E731
    stand_ins = {"rasterio": _module("rasterio", open=open_), "cv2": identity, "rpcm": _module("rpcm"),
                 "torchvision": _module("torchvision", transforms=transforms), "torchvision.transforms": transforms,
                 "datasets": _module("datasets", SatelliteDataset=None), "sat_utils": _module("sat_utils"),
                 "eval_satnerf": _module("eval_satnerf", load_nerf=nothing, batched_inference=nothing, save_nerf_output_to_images=nothing,
                                         predefined_val_ts=nothing)}
    saved = {k: sys.modules.get(k) for k in stand_ins}
    sys.modules.update(stand_ins)
    try:
        loaded = []
        for name in ("study_solar_interpolation", "train_utils"):
            spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(reference_dir, name + ".py"))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            loaded.append(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return loaded


def record_reference(reference_dir):
    import torch

    images = {"color/" + k: v[None] for k, v in color_images().items()}
    units = IP.unit_images()
    images.update({f"unit/{k}": np.ascontiguousarray(np.transpose(v, (2, 0, 1))) for k, v in enumerate(units)})
    study, train_utils = _load_reference(reference_dir, images)
    data = {}
    for name, img in color_images().items():
        data["color_" + name] = img
        for tag in IP.BOUNDS:
            vmin, vmax = IP.recorded_bounds(name, tag)
            with np.errstate(all="ignore"):
                strip = study.hstack_dsm_tifs_v1(["color/" + name], crop=True, vmin=vmin, vmax=vmax)
            assert strip.dtype == np.uint8 and (strip[:, :, 0] == strip[:, :, 2]).all()
            data[f"color_{name}_{tag}"] = strip[:, :, 0]
    for name, img in depth_images().items():
        data["depth_" + name] = img
        hwc = train_utils.visualize_depth(torch.from_numpy(img))
        assert hwc.dtype == np.uint8 and hwc.shape == img.shape + (3,)
        data[f"depth_{name}_index"] = hwc[:, :, 0]
    paths = [f"unit/{k}" for k in range(len(units))]
    data["unit_sun_strip"] = study.hstack_sun_tifs(paths, crop=True)
    data["unit_rgb_strip"] = study.hstack_rgb_tifs(paths, crop=True)
    data["unit_rgb_strip_uncropped"] = study.hstack_rgb_tifs(paths[:1], crop=False)
    return data


if __name__ == "__main__":
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    data = build_fill()
    if len(sys.argv) > 1:
        data.update(record_reference(sys.argv[1]))
    elif os.path.exists(OUT):
        data.update({k: v for k, v in np.load(OUT).items() if k not in data})
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, "with", len(data), "arrays")
