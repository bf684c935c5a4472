"""The Blender loader on the GPU (csrc/blender.hip through ops.blender_colors, ops.pinhole_rays and satnerf_amd.data; DESIGN.md section
7.8): the resized bytes against Pillow's stored ones and, at the workload's 800 x 800 -> 400 x 400, against the integer restatement of
tests/blender_reference.py; the fp32 blend bit for bit; the rays against the fp64 restatement and the reference's own output;
load_blender against the reference's BlenderDataset on the fixture scene; and a batch of it through render_rays with the classic NeRF.

Ray bounds.  Against the restatement: 1 fp32 ulp of a direction component (at most 2^-24 for |d| <= 1) -- bit equality is expected, the
ulp allows a device fp64 sqrt or division that is not correctly rounded and nothing else.  Against the reference: 2^-21 absolute, its
fp32 chain's at most eight roundings on quantities no larger than the unit result.  Origins, near and far are exact in both."""
import os

import numpy as np
import pytest
import torch

from oracle import satnerf_oracle as O
from tests import blender_reference as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
REF_BOUND = 2.0 ** -21


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "blender", "reference.npz"), allow_pickle=False))


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _both(img, oh, ow):
    """ops.blender_colors of one (H, W, 4) uint8 image from its HWC and its CHW tensor, which must agree bit for bit; returns the host
    arrays (rgbs, valid_mask, rgba)."""
    from satnerf_amd import ops

    hwc = torch.from_numpy(np.array(img, order="C")).to(DEV)
    chw = torch.from_numpy(np.array(np.transpose(img, (2, 0, 1)), order="C")).to(DEV)
    a = ops.blender_colors(hwc, oh, ow, layout="hwc", want_rgba=True)
    b = ops.blender_colors(chw, oh, ow, layout="chw", want_rgba=True)
    assert a[0].shape == (oh * ow, 3) and a[0].dtype == torch.float32 and a[0].is_cuda and a[0].is_contiguous()
    assert a[1].shape == (oh * ow,) and a[1].dtype == torch.bool and a[2].shape == (oh, ow, 4) and a[2].dtype == torch.uint8
    got = [t.cpu().numpy() for t in a]
    for x, y in zip(got, b):
        assert _same_bits(x, y.cpu().numpy())
    return got


def _check_blend(rgbs, mask, rgba):
    want, want_mask = B.blend(rgba)
    assert _same_bits(rgbs, want) and _same_bits(mask, want_mask)


@pytest.mark.parametrize("k", range(len(B.FIXTURE_SHAPES)))
def test_resized_bytes_are_pillows(golden, k):
    """16x16 -> 8x8; 37x53 -> 11x17 (odd sizes, taps truncated at both borders); 9x13 -> 18x26 (upscale, ksize 7); 64x64 -> 64x32
    (horizontal pass only); 33x47 -> 5x47 (vertical pass only).  Random 0..255 noise overshoots, so the negative lobes clip; the alpha
    blocks keep transparent, opaque and partial pixels."""
    h, w, oh, ow = B.FIXTURE_SHAPES[k]
    rgbs, mask, rgba = _both(golden[f"resize{k}_src"], oh, ow)
    want = golden[f"resize{k}_out"]
    print(f"{h} x {w} -> {oh} x {ow}: {(rgba != want).sum()} bytes differ from Pillow {golden['pillow_version']}")
    assert _same_bits(rgba, want)
    _check_blend(rgbs, mask, rgba)


def test_same_size_is_the_identity():
    img = B.random_rgba(20, 20, seed=3)
    rgbs, mask, rgba = _both(img, 20, 20)
    assert _same_bits(rgba, img)  # no premultiply round trip: colour bytes under alpha 0 and partial alpha survive
    assert (img[..., :3][img[..., 3] == 0] != 0).any()
    _check_blend(rgbs, mask, rgba)


def test_workload_shape_equals_the_restatement():
    img = B.random_rgba(800, 800, seed=5)
    rgbs, mask, rgba = _both(img, 400, 400)
    want = B.resize_rgba(img, 400, 400)
    print(f"800 x 800 -> 400 x 400: {(rgba != want).sum()} bytes differ")
    assert _same_bits(rgba, want)
    _check_blend(rgbs, mask, rgba)
    assert mask.any() and not mask.all()


def test_writing_into_a_slice_and_the_empty_output():
    from satnerf_amd import ops

    img = B.random_rgba(37, 53, seed=1)
    src = torch.from_numpy(img).to(DEV)
    alone, mask = ops.blender_colors(src, 11, 17)
    n = 11 * 17
    big = torch.full((n + 11, 3), -7.25, device=DEV)
    ret, mask2 = ops.blender_colors(src, 11, 17, out=big[5:5 + n])
    assert ret.data_ptr() == big[5:5 + n].data_ptr() and torch.equal(mask, mask2)
    assert (big[:5] == -7.25).all() and (big[5 + n:] == -7.25).all() and _same_bits(big[5:5 + n].cpu().numpy(), alone.cpu().numpy())
    rgbs, mask, rgba = ops.blender_colors(src, 0, 9, want_rgba=True)
    assert rgbs.shape == (0, 3) and mask.shape == (0,) and rgba.shape == (0, 9, 4)
    with pytest.raises(ValueError, match="four bands"):
        ops.blender_colors(src[:, :, :3].contiguous(), 11, 17)
    with pytest.raises(ValueError, match="GPU"):
        ops.blender_colors(torch.from_numpy(img), 11, 17)


def _check_rays(got, want, bound):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert _same_bits(got[:, [0, 1, 2, 6, 7]], want[:, [0, 1, 2, 6, 7]])
    err = np.abs(got[:, 3:6].astype(np.float64) - want[:, 3:6])
    print(f"direction error {err.max():.3e}, {(got[:, 3:6] != want[:, 3:6]).sum()} components differ in bits")
    assert (err <= bound).all()


@pytest.mark.parametrize("h,w", [(8, 8), (1, 1), (3, 517)])
def test_pinhole_rays_against_the_restatement(golden, h, w):
    """8 x 8 (the fixture), one pixel, and a non-square grid whose row is longer than a workgroup (1551 rays: seven blocks, the last
    partial)."""
    from satnerf_amd import ops

    f = B.focal(float(golden["camera_angle_x"]), w) * 1.25
    c2w = golden["transform_matrix"][1][:3, :4]
    with torch.cuda.device(DEV):
        got = ops.pinhole_rays(h, w, f, 0.9 * f, w / 2 + 0.25, h / 2, c2w, 2.0, 6.0)
    assert got.shape == (h * w, 8) and got.is_cuda
    want = B.pinhole_rays(h, w, f, 0.9 * f, w / 2 + 0.25, h / 2, c2w, 2.0, 6.0)
    ulp = np.spacing(np.abs(want[:, 3:6])).astype(np.float64)
    _check_rays(got.cpu().numpy(), want, ulp)
    with torch.cuda.device(DEV):
        assert ops.pinhole_rays(0, 5, f, f, 2.5, 0.0, c2w, 2.0, 6.0).shape == (0, 8)


def test_pinhole_rays_against_the_reference(golden):
    from satnerf_amd import data

    f = float(golden["focal"])
    for t in range(3):
        got = data.blender_rays(8, 8, f, golden["transform_matrix"][t][:3, :4], device=DEV)
        _check_rays(got.cpu().numpy(), golden["all_rays"][t * 64:(t + 1) * 64], REF_BOUND)


def _scene(tmp_path, golden, n_val=None):
    images = {}
    B.write_scene(str(tmp_path), golden, images, n_val=n_val)
    return str(tmp_path), images.__getitem__


def test_load_blender_equals_the_reference_dataset(tmp_path, golden):
    from satnerf_amd import data

    root, reader = _scene(tmp_path, golden, n_val=11)
    rays, rgbs, ts = data.load_blender(root, "train", img_wh=(8, 8), device=DEV, reader=reader)
    assert rays.is_cuda and rgbs.is_cuda and ts.is_cuda and ts.dtype == torch.int64
    assert _same_bits(rgbs.cpu().numpy(), golden["all_rgbs"])
    _check_rays(rays.cpu().numpy(), golden["all_rays"], REF_BOUND)
    assert _same_bits(ts.cpu().numpy(), golden["all_ts"].astype(np.int64))
    val = data.load_blender(root, "val", img_wh=(8, 8), device=DEV, reader=reader)
    assert len(val) == 8  # the JSON lists 11 frames
    for v in val:
        assert sorted(v) == ["c2w", "rays", "rgbs", "ts", "valid_mask"]
        assert v["rays"].shape == (64, 8) and v["rgbs"].shape == (64, 3) and v["c2w"].shape == (3, 4) and v["ts"].shape == (64,)
        assert v["ts"].dtype == torch.int64 and not v["ts"].any() and v["valid_mask"].dtype == torch.bool and v["valid_mask"].shape == (64,)
    v = val[1]
    assert _same_bits(v["rgbs"].cpu().numpy(), golden["val1_rgbs"]) and _same_bits(v["valid_mask"].cpu().numpy(), golden["val1_valid_mask"])
    _check_rays(v["rays"].cpu().numpy(), golden["val1_rays"], REF_BOUND)


def test_a_batch_of_the_loaded_scene_renders_with_the_classic_nerf(tmp_path, golden):
    from satnerf_amd import data, rendering
    from satnerf_amd.models import load_model

    root, reader = _scene(tmp_path, golden)
    rays, rgbs, ts = data.load_blender(root, "train", img_wh=(8, 8), device=DEV, reader=reader)
    idx = torch.arange(0, rays.shape[0], 2, device=DEV)  # a batch by plain indexing: rows of all three frames
    args = O.default_args(model="nerf", n_samples=16, n_importance=8)
    models = {}
    for typ, seed in (("coarse", 1), ("fine", 2)):
        m = load_model(args)
        m.load_state_dict(O.procedural_nerf_params(args.fc_units, seed=seed))
        models[typ] = m.to(DEV).eval()
    with torch.no_grad():
        res = rendering.render_rays(models, args, rays[idx], ts[idx])
    n = idx.numel()
    assert n == 96 and res["rgb_coarse"].shape == res["rgb_fine"].shape == rgbs[idx].shape == (n, 3)
    assert res["depth_coarse"].shape == res["depth_fine"].shape == (n,)
    assert res["weights_coarse"].shape == (n, 16) and res["weights_fine"].shape == (n, 24)
    for k, v in res.items():
        assert torch.isfinite(v).all(), k
    assert torch.isfinite(((res["rgb_fine"] - rgbs[idx]) ** 2).mean())  # the colours pair with the rays row for row
