"""A dataset's colours, host side: the fp64 oracle (tests/image_colors_reference.py) against torch's bicubic
interpolation on the CPU -- what the reference's torchvision Resize runs --, the u8 / 255 table, load_colors / load_dataset's ordering
and checks with the kernel replaced by the oracle, and the declarations."""
import json
import os

import numpy as np
import pytest
import torch

from tests import image_colors_reference as IC
from tests.scene_loc_reference import scene_copy as _scene_copy
from tests.test_scene_loc_host import FP32_LOC, _rays_stub

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SIZES = {"img_00": (37, 29), "img_01": (64, 96), "img_02": (1, 1), "img_03": (50, 70)}  # the fixture's height x width


def _torch_reference(img_u8, oh, ow):
    """The reference's own steps (datasets/satellite.py:69-79) on the CPU, with the resize taken whatever the factor."""
    img = np.transpose(img_u8, (2, 0, 1)) / 255.
    res = torch.nn.functional.interpolate(torch.Tensor(img)[None], size=(oh, ow), mode="bicubic", align_corners=False)
    return res[0].reshape(3, -1).permute(1, 0).numpy().astype(np.float64)


@pytest.mark.parametrize("h,w,down", IC.SHAPES)
def test_oracle_matches_torch_bicubic_on_the_cpu(h, w, down):
    img, oh, ow, want = IC.case(h, w, down)
    ref = _torch_reference(img, oh, ow)
    assert want.shape == ref.shape == (oh * ow, 3) and oh * ow >= 1
    err = np.abs(want - ref).max()
    print(f"{h} x {w} at {down}: oracle - torch = {err:.3e}")
    assert err <= 2e-6
    if (h, w) == (3, 3):
        assert (oh, ow) == (1, 1)  # a single output pixel
    if (h, w) == (4, 2048):
        # the coordinate is fp32 arithmetic by definition: with fp64 coordinates the same restatement is further from torch
        err64 = np.abs(IC.colors(img, oh, ow, fp64_coords=True) - ref).max()
        print(f"fp64 coordinates: {err64:.3e}")
        assert err64 > err and err64 > 2e-6


def test_conversion_table_is_one_fp32_division():
    x = np.arange(256)
    ref = (x / 255.).astype(np.float32)  # float32(float64(u8) / 255.), the reference's
    one = x.astype(np.float32) / np.float32(255)
    assert one.dtype == np.float32 and np.array_equal(ref.view(np.int32), one.view(np.int32))
    assert np.array_equal(IC.convert(x.astype(np.uint8)).view(np.int32), ref.view(np.int32))


def _write_images(root, img_dir):
    """One seeded random image per JSON of the dataset, in ``img_dir`` under the JSON's "img" name; returns {img_id: uint8 (H, W, 3)}."""
    from PIL import Image

    os.makedirs(img_dir, exist_ok=True)
    made = {}
    for name, (h, w) in SIZES.items():
        with open(os.path.join(root, name + ".json")) as f:
            d = json.load(f)
        assert (d["height"], d["width"]) == (h, w) and d["img"] == name + ".tif"
        made[name] = IC.random_image(h, w, seed=int(name[-2:]) + 7)
        Image.fromarray(made[name]).save(os.path.join(img_dir, d["img"]))
    return made


def _dataset(tmp_path):
    root = _scene_copy(tmp_path)
    img_dir = str(tmp_path / "images")  # not the JSONs' directory
    with open(os.path.join(root, "scene.loc"), "w") as f:
        json.dump(FP32_LOC, f, indent=2)
    return root, img_dir, _write_images(root, img_dir)


def _want(img, down):
    oh, ow = IC.out_size(img.shape[0], img.shape[1], down)
    return torch.from_numpy(IC.colors(img, oh, ow).astype(np.float32))


@pytest.mark.parametrize("down", [1.0, 2.0])
def test_load_colors_follows_load_rays_order_and_offsets(tmp_path, monkeypatch, down):
    from satnerf_amd import data, ops

    root, img_dir, made = _dataset(tmp_path)
    calls = []
    monkeypatch.setattr(ops, "image_colors", IC.image_colors_stub(calls))
    monkeypatch.setattr(ops, "rpc_rays", _rays_stub([]))
    _, _, index = data.load_rays(root, "train", img_downscale=down, device="cpu")
    rgbs = data.load_colors(root, img_dir, "train", img_downscale=down, device="cpu")
    assert rgbs.dtype == torch.float32 and rgbs.shape == (sum(h * w for _, h, w, _ in index), 3)
    for name, h, w, off in index:
        assert (h, w) == IC.out_size(*SIZES[name], down)
        assert torch.equal(rgbs[off:off + h * w], _want(made[name], down)), name
    if down == 1.0:
        assert [i[1:] for i in index] == [(37, 29, 0), (64, 96, 1073), (1, 1, 7217)]
        assert calls == [(37, 29, 37, 29, "hwc"), (64, 96, 64, 96, "hwc"), (1, 1, 1, 1, "hwc")]
        assert torch.equal(rgbs[7217], torch.from_numpy(IC.convert(made["img_02"][0, 0])))  # the 1 x 1 image: one row
    else:
        assert [i[1:] for i in index] == [(18, 14, 0), (32, 48, 252), (0, 0, 1788)] and rgbs.shape == (1788, 3)
        assert calls == [(37, 29, 18, 14, "hwc"), (64, 96, 32, 48, "hwc")]  # the 1 x 1 image: no row and no kernel call
    # validation: the first training image, then test.txt
    calls.clear()
    val = data.load_colors(root, img_dir, "val", img_downscale=down, device="cpu")
    assert len(val) == 2 and [c[:2] for c in calls] == [(37, 29), (50, 70)]
    assert torch.equal(val[0], _want(made["img_00"], down)) and torch.equal(val[1], _want(made["img_03"], down))
    # a reader that returns CHW (rasterio's f.read()) gives the same colours
    calls.clear()

    def chw_reader(path):
        return np.transpose(data._read_image_pillow(path), (2, 0, 1))

    again = data.load_colors(root, img_dir, "train", img_downscale=down, device="cpu", reader=chw_reader)
    assert torch.equal(again, rgbs) and calls and all(c[4] == "chw" for c in calls)
    with pytest.raises(ValueError, match="split"):
        data.load_colors(root, img_dir, "test", device="cpu")


@pytest.mark.parametrize("down", [1.0, 2.0])
def test_load_dataset_returns_the_bank_inputs_and_val_dicts(tmp_path, monkeypatch, down):
    from satnerf_amd import data, ops

    root, img_dir, made = _dataset(tmp_path)
    monkeypatch.setattr(ops, "image_colors", IC.image_colors_stub([]))
    monkeypatch.setattr(ops, "rpc_rays", _rays_stub([]))
    rays, ids, index = data.load_rays(root, "train", img_downscale=down, device="cpu")
    all_rays, all_rgbs, all_ids, index2 = data.load_dataset(root, img_dir, "train", img_downscale=down, device="cpu")
    assert index2 == index and torch.equal(all_rays, rays) and torch.equal(all_ids, ids)
    assert torch.equal(all_rgbs, data.load_colors(root, img_dir, "train", img_downscale=down, device="cpu"))
    assert all_rgbs.shape == (all_rays.shape[0], 3)
    val = data.load_dataset(root, img_dir, "val", img_downscale=down, device="cpu")
    assert [(v["src_id"], v["ts"]) for v in val] == [("img_00", 0), ("img_03", 3)]
    for v in val:
        assert sorted(v) == ["h", "rays", "rgbs", "src_id", "ts", "w"] and v["rgbs"].shape == (v["h"] * v["w"], 3)
        assert torch.equal(v["rgbs"], _want(made[v["src_id"]], down))


@pytest.mark.parametrize("down", [1.0, 2.0])
def test_load_colors_names_the_file_it_cannot_use(tmp_path, monkeypatch, down):
    from PIL import Image

    from satnerf_amd import data, ops

    root, img_dir, made = _dataset(tmp_path)
    monkeypatch.setattr(ops, "image_colors", IC.image_colors_stub([]))
    path = os.path.join(img_dir, "img_01.tif")
    Image.fromarray(IC.random_image(64, 95)).save(path)  # one column short of the JSON's 64 x 96
    with pytest.raises(ValueError, match=r"img_01\.tif is 64 x 95 .* 64 x 96"):
        data.load_colors(root, img_dir, "train", img_downscale=down, device="cpu")
    rgba = np.concatenate([made["img_01"], np.full((64, 96, 1), 255, np.uint8)], 2)
    Image.fromarray(rgba).save(path)
    with pytest.raises(ValueError, match=r"img_01\.tif does not have exactly three bands"):
        data.load_colors(root, img_dir, "train", img_downscale=down, device="cpu")
    Image.fromarray(made["img_01"][:, :, 0]).save(path)  # one band
    with pytest.raises(ValueError, match=r"img_01\.tif does not have exactly three bands"):
        data.load_colors(root, img_dir, "train", img_downscale=down, device="cpu")
    Image.fromarray(made["img_01"][:, :, 0].astype(np.uint16) * 257).save(path)  # 16-bit samples
    with pytest.raises(ValueError, match=r"img_01\.tif is not an 8-bit image"):
        data.load_colors(root, img_dir, "train", img_downscale=down, device="cpu")
    # a reader's 16-bit RGB array of the right shape is refused the same way
    with pytest.raises(ValueError, match=r"img_00\.tif is not an 8-bit image"):
        data.load_colors(root, img_dir, "train", img_downscale=down, device="cpu",
                         reader=lambda p: np.zeros((37, 29, 3), np.uint16))


def test_colors_from_image_takes_host_arrays_and_tensors(monkeypatch):
    from satnerf_amd import data, ops

    calls = []
    monkeypatch.setattr(ops, "image_colors", IC.image_colors_stub(calls))
    img = IC.random_image(5, 7)
    img.setflags(write=False)  # as Pillow hands its pixels out
    want = torch.from_numpy(IC.colors(img, 2, 3).astype(np.float32))
    assert torch.equal(data.colors_from_image(img, 2, 3, device="cpu", layout="hwc"), want)
    assert torch.equal(data.colors_from_image(torch.from_numpy(img.copy()).permute(2, 0, 1), 2, 3, device="cpu", layout="chw"), want)
    out = torch.zeros(6, 3)
    assert data.colors_from_image(img, 2, 3, device="cpu", out=out, layout="hwc") is out and torch.equal(out, want)
    with pytest.raises(ValueError, match="uint8"):
        data.colors_from_image(img.astype(np.float32), 2, 3, device="cpu")


def test_bad_arguments_are_refused_before_any_launch():
    """Host-side checks of sr_image_colors: they return before anything touches a device, so this runs without one."""
    from satnerf_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    f = _lib.lib().sr_image_colors
    err = lambda: _lib.lib().sr_last_error().decode()
    src, out = 0x1000, 0x2000  # never dereferenced: every call below stops at a check
    assert f(src, 0, 7, 21, 3, 1, 2, 3, out, None) != 0 and "at least 1 x 1" in err()
    assert f(src, 5, -7, 21, 3, 1, 2, 3, out, None) != 0 and "at least 1 x 1" in err()
    assert f(src, 5, 7, 21, 3, 1, -2, 3, out, None) != 0 and "output size" in err()
    assert f(src, 5, 7, 21, 3, 1, 2, -3, out, None) != 0 and "output size" in err()
    assert f(src, 5, 7, 21, 0, 1, 2, 3, out, None) != 0 and "strides" in err()
    assert f(None, 5, 7, 21, 3, 1, 2, 3, out, None) != 0 and "null pointer" in err()
    assert f(src, 5, 7, 21, 3, 1, 2, 3, None, None) != 0 and "null pointer" in err()
    assert f(None, 5, 7, 21, 3, 1, 0, 3, None, None) == 0  # an empty output: nothing to do, pointers or not
    assert f(None, 5, 7, 21, 3, 1, 2, 0, None, None) == 0


def test_abi_declared_in_header_and_binding():
    import inspect

    from satnerf_amd import _lib, data, ops

    with open(os.path.join(REPO, "include", "satrender.h")) as f:
        header = " ".join(f.read().split())
    assert ("int sr_image_colors(const uint8_t* src, int src_h, int src_w, int64_t row_stride, int64_t pix_stride, int64_t chan_stride, "
            "int out_h, int out_w, float* out, void* stream);") in header
    assert "satellite.py:67-80" in header
    res, args = _lib.SIGNATURES["sr_image_colors"]
    assert res is _lib._i and args == [_lib._vp, _lib._i, _lib._i, _lib._i64, _lib._i64, _lib._i64, _lib._i, _lib._i, _lib._vp, _lib._vp]
    assert list(inspect.signature(ops.image_colors).parameters) == ["image_u8", "out_h", "out_w", "out", "layout"]
    assert list(inspect.signature(data.colors_from_image).parameters)[:5] == ["image", "h", "w", "device", "out"]
    assert list(inspect.signature(data.load_colors).parameters) == ["root_dir", "img_dir", "split", "img_downscale", "device", "reader"]
    assert list(inspect.signature(data.load_dataset).parameters) == ["root_dir", "img_dir", "split", "img_downscale", "device", "cache_dir",
                                                                     "create_scene_loc", "reader"]
    assert list(inspect.signature(data.load_rays).parameters) == ["root_dir", "split", "img_downscale", "device", "cache_dir",
                                                                  "create_scene_loc"]
