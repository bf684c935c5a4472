"""Orthorectification onto a DSM raster, host side (no GPU): the numpy reference of tests/orthorectify_reference.py on hand-built cases,
the conditions that keep the GPU comparisons from being empty (share floor) or from hiding a failure (at most 1 % of the cells
unstable), the prototypes and the argument checks of the two C entries, the errors of the Python layer, and the view order and RPC
rescaling of ``dsm.orthorectify_dataset`` on a temporary dataset."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import rpc_oracle as RO
from tests import heightfield_reference as H
from tests import orthorectify_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module", autouse=True)
def _library():
    from satnerf_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()


# ---- the samplers -----------------------------------------------------------------------------------------------------------------------
def test_samplers_on_hand_values():
    img = np.array([[0, 51], [102, 255]], np.uint8)  # 0, 0.2, 0.4, 1.0
    at = lambda col, row, mode: float(T.sample_np(img, np.array([col]), np.array([row]), mode)[0, 0])  # noqa: E731
    for mode in T.MODES:  # at a pixel centre every sampler gives the pixel
        assert at(1.0, 0.0, mode) == 51 / 255.0 and at(0.0, 1.0, mode) == 102 / 255.0
    assert at(0.5, 0.0, "nearest") == 51 / 255.0 and at(0.49, 0.51, "nearest") == 102 / 255.0  # floor(x + 0.5): a half rounds up
    assert at(0.5, 0.5, "bilinear") == pytest.approx((0 + 51 + 102 + 255) / 4 / 255.0, abs=1e-16)
    assert at(0.25, 0.0, "bilinear") == pytest.approx(0.25 * 51 / 255.0, abs=1e-16)
    s = np.linspace(0, 1, 11)
    assert np.allclose(T.keys(1 + s) + T.keys(s) + T.keys(1 - s) + T.keys(2 - s), 1.0, atol=1e-15)  # the taps' weights sum to one
    assert T.keys(np.array([0.0, 1.0, 2.0, 0.5])).tolist() == [1.0, 0.0, 0.0, 0.5625]
    ramp = np.tile(np.arange(8, dtype=np.float32) * 0.125, (8, 1))  # a linear image is reproduced inside, where no index is clamped
    assert float(T.sample_np(ramp, np.array([3.3]), np.array([4.7]), "bicubic")[0, 0]) == pytest.approx(3.3 * 0.125, abs=1e-15)
    assert float(T.sample_np(ramp, np.array([0.3]), np.array([0.0]), "bicubic")[0, 0]) != pytest.approx(0.3 * 0.125, abs=1e-6)  # edge replicate
    nan_img = np.array([[0.5, NAN], [0.5, 0.5]], np.float32)
    assert np.isnan(T.sample_np(nan_img, np.array([0.0]), np.array([0.0]), "bilinear")[0, 0])  # also under a zero weight
    assert T.sample_np(nan_img, np.array([0.0]), np.array([0.0]), "nearest")[0, 0] == 0.5
    assert T.pixel_values(np.zeros((2, 3), np.float32)).shape == (2, 3, 1)


# ---- the conditions on the GPU tests' inputs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(T.CASES))
def test_shares_and_unstable_cells(name):
    t = T.truth(name)
    st = t["status"]
    share = {k: float((st == v).mean()) for k, v in (("visible", T.VISIBLE), ("occluded", T.OCCLUDED), ("outside", T.OUTSIDE), ("empty", T.EMPTY))}
    unstable, unstable_nearest = T.unstable(name), T.unstable(name, nearest=True)
    print(f"{name}: {st.size} cells, shares {share}, unstable {unstable.sum()} ({unstable_nearest.sum()} for nearest), eps_px {t['eps']:.3e}")
    assert unstable_nearest.mean() <= 0.01 and unstable.mean() <= 0.01
    assert (st == T.VISIBLE).any()  # every case samples something
    if name in T.SHARE_FLOOR:
        assert min(share["visible"], share["occluded"], share["outside"]) >= 0.10
    assert ((st == T.EMPTY) == ~np.isfinite(T.case(name)["hgt"])).all()
    assert t["eps"] < 1e-3  # far below what would move a sample


def test_mosaic_views_are_stable_and_overlap():
    c = T.case("jax_0.3")
    seen = np.zeros(c["hgt"].shape, int)
    for image, rpc in T.mosaic_views():
        status, col, row, stable = T.status_np(c["hgt"], c["grid"], c["zone"], rpc)
        eps = T.eps_px(c["hgt"], c["grid"], c["zone"], rpc)
        assert T.unstable_np(col, row, stable, image.shape[1], image.shape[0], eps).mean() <= 0.01
        seen += status == T.VISIBLE
    print("cells seen by 0..3 views:", np.bincount(seen.ravel(), minlength=4).tolist())
    assert all((seen == k).any() for k in range(4))  # min_views has something to mask at every level


# ---- hand-built cases on the reference -----------------------------------------------------------------------------------------------------
def test_a_flat_raster_has_no_occluded_cell():
    for name in ("jax_0.3", "hole_0.8"):
        c = T.case(name)
        flat = np.where(np.isfinite(c["hgt"]), np.float32(11.0), np.float32(NAN))
        status = T.status_np(flat, c["grid"], c["zone"], c["rpc"])[0]
        assert not (status == T.OCCLUDED).any() and (status == T.VISIBLE).any() and (status == T.OUTSIDE).any()
    # ... and with a bias that lifts every start above the maximum nothing is cast at all
    c = T.case("jax_0.3")
    assert not (T.status_np(c["hgt"], c["grid"], c["zone"], c["rpc"], bias=40.0, delta=None)[0] == T.OCCLUDED).any()


def test_a_tower_hides_the_cells_behind_it():
    hgt, grid, zone, rpc = T.tower_case()
    status, col, row, stable = T.status_np(hgt, grid, zone, rpc)
    assert stable.all()
    T.check_tower(status)


def test_the_global_maximum_is_visible():
    checked = 0
    for name in sorted(T.CASES):  # wherever a case's highest cells fall inside its image (the tower's does, too)
        c, t = T.case(name), T.truth(name)
        at = (c["hgt"] == np.nanmax(c["hgt"])) & (t["status"] != T.OUTSIDE)
        assert (t["status"][at] == T.VISIBLE).all()
        checked += bool(at.any())
    assert checked >= 2


def test_a_camera_on_the_cell_centres_reproduces_its_image():
    hgt, grid, zone, rpc, image = T.grid_camera_case()
    status, col, row, stable = T.status_np(hgt, grid, zone, rpc)
    ysize, xsize = hgt.shape
    jj, cc = np.meshgrid(np.arange(ysize), np.arange(xsize), indexing="ij")
    assert (status == T.VISIBLE).all() and np.abs(col - cc - 2).max() < 1e-3 and np.abs(row - jj - 2).max() < 1e-3
    got = T.colors_np(image, status, col, row, "nearest")
    assert (got == image[2:2 + ysize, 2:2 + xsize].astype(np.float64) / 255.0).all()


def test_one_cell_and_all_nan_rasters():
    t = T.truth("one_cell")
    assert t["status"].tolist() == [[T.VISIBLE]]  # alone, it is the maximum: nothing is cast
    c = T.case("jax_0.3")
    empty = np.full((5, 7), NAN, np.float32)
    status, col, row, stable = T.status_np(empty, c["grid"], c["zone"], c["rpc"])
    assert (status == T.EMPTY).all() and np.isnan(col).all() and np.isnan(row).all()


def test_mosaic_reference_counts_and_means():
    c32 = [np.array([[[0.25], [0.5]]], np.float32), np.array([[[0.75], [NAN]]], np.float32)]
    st = [np.array([[1, 2]], np.uint8), np.array([[1, 3]], np.uint8)]
    total, count, mean = T.mosaic_np(c32, st)
    assert total.ravel().tolist() == [1.0, 0.0] and count.ravel().tolist() == [2, 0]
    assert mean[0, 0, 0] == 0.5 and np.isnan(mean[0, 1, 0])


# ---- the C entries ------------------------------------------------------------------------------------------------------------------------
def test_the_two_entries_are_declared_and_bound():
    from satnerf_amd import _lib

    with open(os.path.join(ROOT, "include", "satrender.h")) as f:
        text = f.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, arity in (("sr_orthorectify_scratch", 3), ("sr_orthorectify", 29)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, f"{name} is not declared in include/satrender.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        res, argtypes = _lib.SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == n_args == arity, (name, n_args, len(argtypes))
    assert _lib.SIGNATURES["sr_orthorectify"][1][-1] is C.c_void_p
    assert "section 7.16" in text and os.path.exists(os.path.join(ROOT, "satnerf_amd", "csrc", "orthorectify.hip"))


def test_scratch_size():
    from satnerf_amd import _lib, ops

    assert ops.orthorectify_scratch(37, 53) >= 37 * 53 * 17 and ops.orthorectify_scratch(1, 1) >= 17
    assert ops.orthorectify_scratch(2048, 2048) <= 2048 * 2048 * 17 + 1024
    for xsize, ysize in ((0, 5), (5, 0), (1 << 16, 1 << 15)):
        with pytest.raises(_lib.SatRenderError, match="sr_orthorectify_scratch"):
            ops.orthorectify_scratch(xsize, ysize)
    with pytest.raises(_lib.SatRenderError, match="null"):
        _lib.call("sr_orthorectify_scratch", 4, 4, None)


_ptr = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731  (fake: never dereferenced, every check comes before the launch)


def _call(**over):
    from satnerf_amd import _lib, ops

    a = dict(hgt=4096, xsize=37, ysize=53, res=0.5, xoff=1000.25, yoff=2000.0, zone=17, blockmax=4096, gmax=4096, accelerate=1, rpc="ok",
             image=4096, fmt=0, width=37, height=29, channels=3, row_stride=111, pix_stride=3, mode=1, bias=0.0, stages=0, scratch=4096,
             scratch_bytes=1 << 20, color=4096, status=4096, colrow=4096, sum=None, count=None)
    a.update(over)
    buf = None
    if a["rpc"] is not None:
        rpc = dict(RO.synthetic_rpc(1, 29, 37))
        if a["rpc"] != "ok":
            rpc[a["rpc"]] = 0.0
        buf = ops.rpc_buffer(rpc)
    _lib.call("sr_orthorectify", _ptr(a["hgt"]), a["xsize"], a["ysize"], a["res"], a["xoff"], a["yoff"], a["zone"], _ptr(a["blockmax"]),
              _ptr(a["gmax"]), a["accelerate"], None if buf is None else C.addressof(buf), _ptr(a["image"]), a["fmt"], a["width"], a["height"],
              a["channels"], a["row_stride"], a["pix_stride"], a["mode"], a["bias"], a["stages"], _ptr(a["scratch"]), a["scratch_bytes"],
              _ptr(a["color"]), _ptr(a["status"]), _ptr(a["colrow"]), _ptr(a["sum"]), _ptr(a["count"]), None)


@pytest.mark.parametrize("over", [
    dict(hgt=None), dict(gmax=None), dict(gmax=None, accelerate=0), dict(blockmax=None), dict(image=None), dict(scratch=None), dict(color=None),
    dict(status=None), dict(colrow=None), dict(rpc=None),
    dict(xsize=0), dict(ysize=0), dict(ysize=-2), dict(xsize=1 << 16, ysize=1 << 15),
    dict(res=0.0), dict(res=-0.5), dict(res=NAN), dict(res=INF), dict(xoff=NAN), dict(xoff=INF), dict(yoff=-INF), dict(yoff=NAN),
    dict(zone=0), dict(zone=61), dict(accelerate=2), dict(accelerate=-1),
    dict(width=0), dict(height=0), dict(height=-1), dict(channels=0), dict(channels=5), dict(fmt=2), dict(fmt=-1),
    dict(pix_stride=2), dict(row_stride=110), dict(row_stride=0), dict(pix_stride=-3),
    dict(mode=3), dict(mode=-1), dict(bias=-0.1), dict(bias=NAN), dict(bias=INF), dict(stages=3), dict(stages=-1),
    dict(sum=4096), dict(count=4096),
    dict(rpc="row_scale"), dict(rpc="col_scale"), dict(rpc="lat_scale"), dict(rpc="lon_scale"), dict(rpc="alt_scale"),
    dict(scratch_bytes=37 * 53 * 17 - 1), dict(scratch_bytes=0), dict(scratch=4100)])
def test_argument_errors(over):
    from satnerf_amd import _lib

    with pytest.raises(_lib.SatRenderError, match="sr_orthorectify"):
        _call(**over)


# ---- the Python layer without a GPU --------------------------------------------------------------------------------------------------------
def test_python_layer_errors():
    from satnerf_amd import dsm, evaluate, ops

    hgt = torch.zeros(5, 7)
    d = dsm.DSM(hgt, torch.ones(5, 7), 1000.25, 2000.0, 0.5, "17R")
    rpc = RO.synthetic_rpc(1, 29, 37)
    image = torch.zeros(29, 37, 3, dtype=torch.uint8)
    for fn in (lambda: ops.orthorectify(hgt, 0.5, 1000.25, 2000.0, 17, rpc, image), lambda: dsm.orthorectify(d, image, rpc),
               lambda: dsm.ortho_mosaic(d, [(image, rpc)]), lambda: evaluate.ortho_psnr(torch.zeros(5, 7, 3), {"color": torch.zeros(5, 7, 3),
                                                                                                                "count": torch.ones(5, 7)})):
        with pytest.raises(ValueError, match="GPU"):  # CPU tensors
            fn()
    with pytest.raises(ValueError, match="DSM"):
        dsm.orthorectify(hgt, image, rpc)
    with pytest.raises(ValueError, match="DSM"):
        dsm.ortho_mosaic(hgt, [(image, rpc)])
    for fn in (dsm.orthorectify, lambda d_, im, r, **kw: dsm.ortho_mosaic(d_, [(im, r)], **kw)):
        with pytest.raises(ValueError, match="mode"):
            fn(d, image, rpc, mode="lanczos")
        for bias in (-1.0, NAN, INF):
            with pytest.raises(ValueError, match="bias"):
                fn(d, image, rpc, bias=bias)
        with pytest.raises(ValueError, match="C in 1..4"):
            fn(d, torch.zeros(29, 37, 5, dtype=torch.uint8), rpc)
        with pytest.raises(ValueError, match="uint8 or float32"):
            fn(d, torch.zeros(29, 37, 3, dtype=torch.float64), rpc)
        with pytest.raises(ValueError, match="zone"):
            fn(dsm.DSM(hgt, torch.ones(5, 7), 1000.25, 2000.0, 0.5, ""), image, rpc)
        with pytest.raises(ValueError, match="zone"):
            fn(d, image, rpc, zone=61)
    with pytest.raises(ValueError, match="views is empty"):
        dsm.ortho_mosaic(d, [])
    with pytest.raises(ValueError, match="views is empty"):
        dsm.ortho_mosaic(d, iter(()))
    with pytest.raises(ValueError, match="min_views"):
        dsm.ortho_mosaic(d, [(image, rpc)], min_views=0)
    with pytest.raises(ValueError, match="mode"):
        ops.orthorectify(hgt, 0.5, 1000.25, 2000.0, 17, rpc, image, mode="cubic")


# ---- a dataset's split as views ---------------------------------------------------------------------------------------------------------------
def write_dataset(root, sizes=((12, 16), (10, 14), (8, 8)), n_test=1):
    """A tiny dataset under ``root``: JSONs from ``synthetic_rpc`` with PNGs written through Pillow; the last ``n_test`` are test images.
    Returns the images (uint8 (H, W, 3)) by file stem."""
    from PIL import Image

    os.makedirs(os.path.join(root, "imgs"), exist_ok=True)
    names, images = [], {}
    for k, (h, w) in enumerate(sizes):
        rpc = {key: (v.tolist() if hasattr(v, "tolist") else v) for key, v in RO.synthetic_rpc(40 + k, h, w).items()}
        stem = f"view_{k:02d}"
        img = T.image_u8(h, w, 3, 300 + k)
        Image.fromarray(img).save(os.path.join(root, "imgs", stem + ".png"))
        with open(os.path.join(root, stem + ".json"), "w") as f:
            json.dump({"rpc": rpc, "height": h, "width": w, "img": stem + ".png", "sun_elevation": 60.0, "sun_azimuth": 140.0}, f)
        names.append(stem + ".json")
        images[stem] = img
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("\n".join(names[:len(names) - n_test]) + "\n")
    with open(os.path.join(root, "test.txt"), "w") as f:
        f.write("\n".join(names[len(names) - n_test:]) + "\n")
    return images


@pytest.mark.parametrize("split,downscale", [("train", 1.0), ("train", 2.0), ("val", 1.0)])
def test_dataset_views_follow_the_split_and_rescale_the_cameras(tmp_path, monkeypatch, split, downscale):
    """Without a GPU: the colours come from a stand-in for ``data.load_colors`` (which needs the device) and the mosaic is intercepted, so
    what is checked is the pairing, the order, the shapes and the cameras that ``orthorectify_dataset`` hands on."""
    from satnerf_amd import data, dsm

    root = str(tmp_path)
    write_dataset(root)
    metas, _ = data._split_images(root, split, downscale)
    blocks = [torch.full((h * w, 3), float(k)) for k, (_, h, w) in enumerate(metas)]

    def fake_colors(root_dir, img_dir, split="train", img_downscale=1.0, device="cuda", reader=None):
        assert (root_dir, img_dir, img_downscale, reader) == (root, os.path.join(root, "imgs"), downscale, "the reader")
        return torch.cat(blocks) if split == "train" else blocks

    seen = {}
    monkeypatch.setattr(data, "load_colors", fake_colors)
    monkeypatch.setattr(dsm, "ortho_mosaic", lambda d, views, **kw: seen.update(dsm=d, views=views, kw=kw) or "mosaic")
    d = dsm.DSM(torch.zeros(5, 7), torch.ones(5, 7), 1000.25, 2000.0, 0.5, "17R")
    out = dsm.orthorectify_dataset(d, root, os.path.join(root, "imgs"), split=split, img_downscale=downscale, reader="the reader",
                                   mode="bicubic", min_views=2)
    assert out == "mosaic" and seen["dsm"] is d and seen["kw"] == dict(mode="bicubic", min_views=2)
    assert len(seen["views"]) == len(metas) == 2  # two training images; the first of them and the test image
    for k, ((image, rpc), (meta, h, w)) in enumerate(zip(seen["views"], metas)):
        assert tuple(image.shape) == (h, w, 3) and bool((image == float(k)).all())
        assert rpc == data.rescale_rpc(meta["rpc"], 1.0 / downscale)
        assert rpc["col_scale"] == meta["rpc"]["col_scale"] / downscale and rpc["lat_scale"] == meta["rpc"]["lat_scale"]
