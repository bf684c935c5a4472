"""A dataset's colours on the GPU (csrc/image_colors.hip through ops.image_colors and satnerf_amd.data): the
conversion bit for bit, the bicubic resize against the fp64 oracle of tests/image_colors_reference.py in both layouts, sources smaller
than the stencil, partial blocks, writing into a slice of a larger tensor, an output past 2^31 bytes, the empty output, and a dataset
directory end to end into RayBank and evaluate_image.

The resize bound, 4e-6 absolute, is derived: 16 products and 15 adds in fp32 on values <= 1 with sum |w| <= 1.27^2 ~ 1.6 give about
1.7e-6, and the rounding of the eight polynomial weights about 8e-7 more."""
import json
import os

import numpy as np
import pytest
import torch

from tests import image_colors_reference as IC
from tests.scene_loc_reference import scene_copy as _scene_copy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 4e-6


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


def _dev(img_hwc, layout):
    t = torch.from_numpy(np.array(img_hwc if layout == "hwc" else np.transpose(img_hwc, (2, 0, 1)), order="C"))  # a writable copy
    return t.to(DEV)


def _both(img, oh, ow):
    """ops.image_colors of one (H, W, 3) uint8 image from its HWC and its CHW tensor; the two must agree bit for bit."""
    from satnerf_amd import ops

    a = ops.image_colors(_dev(img, "hwc"), oh, ow, layout="hwc")
    b = ops.image_colors(_dev(img, "chw"), oh, ow, layout="chw")
    assert a.shape == (oh * ow, 3) and a.dtype == torch.float32 and a.is_cuda and a.is_contiguous()
    assert _same_bits(a, b)
    return a


@pytest.mark.parametrize("h,w", [(256, 1), (37, 29)])
def test_identity_is_u8_over_255_bit_for_bit(h, w):
    if (h, w) == (256, 1):
        img = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, 2)  # every byte value in each channel
        img[:, :, 1] = img[::-1, :, 0]
        img[:, :, 2] = np.roll(img[:, :, 0], 101, 0)
    else:
        img = IC.random_image(h, w)  # 3219 bytes: the last thread of the dense path converts three of its four
    want = torch.from_numpy(IC.convert(img).reshape(-1, 3))
    assert _same_bits(_both(img, h, w), want)


@pytest.mark.parametrize("h,w,down", IC.SHAPES)
def test_resize_against_the_fp64_oracle_in_both_layouts(h, w, down):
    img, oh, ow, want = IC.case(h, w, down)
    got = _both(img, oh, ow).cpu().numpy().astype(np.float64)
    err = np.abs(got - want).max()
    print(f"{h} x {w} at {down} -> {oh} x {ow}: |gpu - oracle| = {err:.3e}")
    assert err <= BOUND


@pytest.mark.parametrize("h,w,oh,ow", [(1, 1, 1, 1), (2, 3, 1, 1), (3, 7, 1, 3), (40, 40, 16, 16), (37, 53, 24, 35), (9, 130, 4, 65)])
def test_small_sources_and_partial_blocks(h, w, oh, ow):
    """Sources smaller than the 4 x 4 stencil (every tap clamps), 256 output pixels exactly (one full block), 840 = three blocks and 72
    threads, 260 = one block and four threads."""
    img = IC.random_image(h, w, seed=h * w)
    got = _both(img, oh, ow).cpu().numpy().astype(np.float64)
    err = np.abs(got - IC.colors(img, oh, ow)).max()
    print(f"{h} x {w} -> {oh} x {ow}: |gpu - oracle| = {err:.3e}")
    assert err <= BOUND


@pytest.mark.parametrize("oh,ow", [(37, 53), (24, 35)])
def test_writing_into_a_slice_leaves_the_neighbours_alone(oh, ow):
    """``out`` = rows 5 .. 5 + n of a larger tensor (60 bytes in: 4-byte aligned only, so the conversion takes its scalar form)."""
    from satnerf_amd import ops

    img = IC.random_image(37, 53)
    n = oh * ow
    for layout in ("hwc", "chw"):
        src = _dev(img, layout)
        alone = ops.image_colors(src, oh, ow, layout=layout)
        big = torch.full((n + 11, 3), -7.25, device=DEV)
        ret = ops.image_colors(src, oh, ow, out=big[5:5 + n], layout=layout)
        assert ret.data_ptr() == big[5:5 + n].data_ptr()
        assert (big[:5] == -7.25).all() and (big[5 + n:] == -7.25).all() and _same_bits(big[5:5 + n], alone)


def test_output_past_two_gib():
    """13400 x 13400: the converted image is 2.15 GB and so is the 13398 x 13398 resize -- byte offsets beyond 2^31 in the output.  The
    conversion against a lookup of the 256 reference values on the device, the resize's first and last rows against the oracle."""
    from satnerf_amd import ops

    side = 13400
    img = torch.randint(0, 256, (side, side, 3), dtype=torch.uint8, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    got = ops.image_colors(img, side, side)
    assert got.shape == (side * side, 3) and got.numel() * 4 > 2 ** 31
    table = torch.from_numpy(IC.convert(np.arange(256, dtype=np.uint8))).to(DEV)
    assert torch.equal(got.view(-1), torch.index_select(table, 0, img.view(-1).int()))
    del got
    oh, ow = IC.out_size(side, side, 1.0001)
    assert (oh, ow) == (13398, 13398) and oh * ow * 12 > 2 ** 31
    got = ops.image_colors(img, oh, ow)
    iy, wy = IC.axis_taps(side, oh)
    rows = np.array([0, 1, oh - 2, oh - 1])
    taps = IC.convert(img[torch.from_numpy(iy[rows].reshape(-1)).to(DEV)].cpu().numpy()).reshape(len(rows), 4, side, 3)
    want = IC.resize_rows(taps, wy[rows], ow)
    have = got.view(oh, ow, 3)[torch.from_numpy(rows).to(DEV)].cpu().numpy().astype(np.float64)
    err = np.abs(have - want).max()
    print(f"{side} x {side} -> {oh} x {ow}, rows {rows.tolist()}: |gpu - oracle| = {err:.3e}")
    assert err <= BOUND


def test_empty_output_launches_nothing():
    from satnerf_amd import _lib, ops

    img = _dev(IC.random_image(5, 7), "hwc")
    for oh, ow in ((0, 3), (2, 0), (0, 0)):
        got = ops.image_colors(img, oh, ow)
        assert got.shape == (0, 3) and got.dtype == torch.float32
    big = torch.full((4, 3), 2.5, device=DEV)
    ops.image_colors(img, 0, 9, out=big[2:2])
    torch.cuda.synchronize()
    assert (big == 2.5).all()
    assert _lib.lib().sr_image_colors(None, 5, 7, 21, 3, 1, 0, 4, None, None) == 0  # no pointer to launch with, and no error


def test_wrapper_names_the_argument_it_refuses():
    from satnerf_amd import ops

    img = _dev(IC.random_image(5, 7), "hwc")
    with pytest.raises(ValueError, match="image_u8 must live on the GPU"):
        ops.image_colors(img.cpu(), 2, 3)
    with pytest.raises(ValueError, match="image_u8 must be torch.uint8"):
        ops.image_colors(img.float(), 2, 3)
    with pytest.raises(ValueError, match="image_u8 must be contiguous"):
        ops.image_colors(img.permute(2, 0, 1), 2, 3)
    with pytest.raises(ValueError, match="three bands"):
        ops.image_colors(torch.zeros(5, 7, 4, dtype=torch.uint8, device=DEV), 2, 3)
    with pytest.raises(ValueError, match=r"out must be \(6, 3\)"):
        ops.image_colors(img, 2, 3, out=torch.zeros(7, 3, device=DEV))
    with pytest.raises(ValueError, match="out must be contiguous"):
        ops.image_colors(img, 2, 3, out=torch.zeros(6, 4, device=DEV)[:, :3])
    with pytest.raises(ValueError, match="out_h and out_w"):
        ops.image_colors(img, -1, 3)
    # 3 x W x 3 reads both ways: the layout has to be said, and it decides the answer
    amb = IC.random_image(3, 5)
    with pytest.raises(ValueError, match="layout"):
        ops.image_colors(_dev(amb, "hwc"), 3, 5)
    as_hwc = ops.image_colors(_dev(amb, "hwc"), 3, 5, layout="hwc")
    assert _same_bits(as_hwc, torch.from_numpy(IC.convert(amb).reshape(-1, 3)))
    as_chw = ops.image_colors(_dev(amb, "hwc"), 5, 3, layout="chw")  # the same bytes read as three 5 x 3 planes
    assert _same_bits(as_chw, torch.from_numpy(IC.convert(amb).reshape(3, 15).T.copy()))


def _dataset(tmp_path):
    from PIL import Image

    root = _scene_copy(tmp_path)
    img_dir = str(tmp_path / "images")
    os.makedirs(img_dir)
    made = {}
    for name in ("img_00", "img_01", "img_02", "img_03"):
        with open(os.path.join(root, name + ".json")) as f:
            d = json.load(f)
        made[name] = IC.random_image(d["height"], d["width"], seed=int(name[-2:]) + 7)
        Image.fromarray(made[name]).save(os.path.join(img_dir, d["img"]))
    return root, img_dir, made


def test_dataset_directory_to_ray_bank_and_evaluate_image(tmp_path):
    from satnerf_amd import data
    from satnerf_amd.evaluate import evaluate_image
    from tests.test_hip_metrics import _model_and_rays

    root, img_dir, made = _dataset(tmp_path)
    all_rays, all_rgbs, all_ids, index = data.load_dataset(root, img_dir, "train", img_downscale=2.0, device=DEV, create_scene_loc=True)
    rays, ids, index2 = data.load_rays(root, "train", img_downscale=2.0, device=DEV)
    assert index == index2 == [("img_00", 18, 14, 0), ("img_01", 32, 48, 252), ("img_02", 0, 0, 1788)]
    assert _same_bits(all_rays, rays) and torch.equal(all_ids, ids) and all_rgbs.shape == (1788, 3) and all_rgbs.is_cuda
    for name, h, w, off in index:
        if h * w:
            block = data.colors_from_image(made[name], h, w, device=DEV)
            assert _same_bits(all_rgbs[off:off + h * w], block), name
            err = np.abs(block.cpu().numpy().astype(np.float64) - IC.colors(made[name], h, w)).max()
            assert err <= BOUND, (name, err)
    # the bank: a batch's colours are the rows of all_rgbs at the indices drawn
    drawn = data.RayBank(all_rays, all_rgbs, all_ids, 64).next_indices()
    b_rays, b_ts, b_rgbs = data.RayBank(all_rays, all_rgbs, all_ids, 64).next_batch()  # the same seed: the same draw
    assert drawn.shape == (64,) and _same_bits(b_rgbs, all_rgbs[drawn]) and _same_bits(b_rays, all_rays[drawn])
    assert torch.equal(b_ts, all_ids[drawn])
    # validation: each entry carries its colours, and evaluate_image takes them
    val = data.load_dataset(root, img_dir, "val", img_downscale=2.0, device=DEV)
    assert [(v["src_id"], v["ts"], v["h"], v["w"]) for v in val] == [("img_00", 0, 18, 14), ("img_03", 3, 25, 35)]
    assert _same_bits(val[0]["rgbs"], all_rgbs[:252])
    assert _same_bits(val[1]["rgbs"], data.colors_from_image(np.transpose(made["img_03"], (2, 0, 1)), 25, 35, device=DEV))
    v = val[0]
    models, args, _, _, _ = _model_and_rays(1)
    res = evaluate_image(models, v["rays"], torch.full((v["h"] * v["w"],), v["ts"], dtype=torch.int64, device=DEV), v["rgbs"], v["h"], v["w"],
                         args)
    assert np.isfinite(res["psnr"]) and np.isfinite(res["ssim"]) and res["outputs"]["rgb"].shape == (252, 3)
