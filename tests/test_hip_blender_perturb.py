"""NeRF-W's perturbations of a Blender scene on the GPU (csrc/blender.hip's perturb_kernel through ops.blender_perturb and
satnerf_amd.data).  Every comparison is byte equality of whole images against the numpy restatement
(tests/blender_perturb_reference.py), and every fixture case also against the SHA-256 of what the reference's own ``add_perturbation``
wrote (tests/golden/blender_perturb/reference.npz).  ``load_blender_perturbed`` is held to the reference's
``BlenderDataset(..., perturbation=...)``: colours bit for bit in fp32 -- the resize and the blend behind the perturbation are the
byte-exact kernels of tests/test_hip_blender.py, so there is nothing to tolerate -- and ray directions to the sibling file's 2^-21
against the reference's fp32 chain."""
import os

import numpy as np
import pytest
import torch

from oracle import satnerf_oracle as O
from tests import blender_perturb_reference as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
REF_BOUND = 2.0 ** -21
WH = P.SCENE_WH
N = WH * WH


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "blender_perturb", "reference.npz"), allow_pickle=False))


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _all_ways(img, lut, rects, fills):
    """ops.blender_perturb of one (H, W, 4) uint8 image four ways -- HWC and CHW, each into a new tensor and in place -- which must agree
    byte for byte and leave the source alone when it is not the destination; returns the host (H, W, 4) result."""
    from satnerf_amd import ops

    got = []
    for layout, host in (("hwc", np.array(img, order="C")), ("chw", np.array(np.transpose(img, (2, 0, 1)), order="C"))):
        src = torch.from_numpy(host).to(DEV)
        out = ops.blender_perturb(src, lut, rects, fills, layout=layout)
        assert out.shape == src.shape and out.dtype == torch.uint8 and out.is_cuda and out.data_ptr() != src.data_ptr()
        assert _same_bits(src.cpu().numpy(), host)
        same = ops.blender_perturb(src, lut, rects, fills, layout=layout, out=src)
        assert same is src and torch.equal(src, out)
        res = out.cpu().numpy()
        got.append(res if layout == "hwc" else np.ascontiguousarray(np.transpose(res, (1, 2, 0))))
    assert _same_bits(got[0], got[1])
    return got[0]


@pytest.mark.parametrize("h,w", [(416, 416), (333, 417), (100, 120), (230, 611)])
def test_fixture_cases_equal_the_restatement_and_the_reference(golden, h, w):
    """416 x 416: every seed's strip is clipped at the right and / or bottom edge.  333 x 417: odd sides, a width that is no multiple of
    4 (nor of the 64 columns of a wave), rows that are no multiple of a workgroup's 16; seeds 2 and 99 draw, the others lie below the
    image.  100 x 120: every rectangle is outside.  230 x 611: strips cut off at the bottom."""
    i = P.SIZES.index((h, w))
    for j, seed in enumerate(P.SEEDS):
        src = P.pattern_rgba(h, w, frame=seed)
        results = {}
        for k, variant in enumerate(P.VARIANTS):
            got = _all_ways(src, *P.host_parameters(seed, variant))
            want = P.perturbed(src, seed, variant)
            touched = int((got != src).any(-1).sum())
            print(f"{h} x {w} seed {seed} {'+'.join(variant)}: {(got != want).sum()} bytes differ, {touched} pixels touched")
            assert _same_bits(got, want)
            assert _same_bits(P.sha256(got), golden["hash_out"][i, j, k]) and touched == golden["touched"][i, j, k]
            results[variant] = got
        if not golden["touched"][i, j, P.VARIANTS.index(("occ",))]:  # nothing drawn: the input, and the colour-only result
            assert _same_bits(results[("occ",)], src) and _same_bits(results[("color", "occ")], results[("color",)])


def test_the_workload_frame(golden):
    """800 x 800, seed 3: the whole strip lies inside, 201 x 201 pixels."""
    i, j = P.SIZES.index((800, 800)), P.SEEDS.index(3)
    src = P.pattern_rgba(800, 800, frame=3)
    for k, variant in enumerate(P.VARIANTS):
        got = _all_ways(src, *P.host_parameters(3, variant))
        assert _same_bits(P.sha256(got), golden["hash_out"][i, j, k])
        assert _same_bits(got, P.perturbed(src, 3, variant))
        if "color" not in variant:
            assert (got != src).any(-1).sum() == 40401


HAND_MADE = {
    "negative corners": ([[-20, -7, 5, 3]], [[9, 8, 7, 6]]),
    "one pixel": ([[63, 63, 63, 63], [0, 0, 0, 0], [17, 31, 17, 31]], [[1, 2, 3, 4], [5, 6, 7, 8], [250, 251, 252, 253]]),
    "later wins": ([[10, 10, 40, 40], [30, 5, 50, 20]], [[200, 100, 50, 255], [1, 1, 1, 0]]),
    "x1 < x0 and y1 < y0": ([[30, 10, 29, 50], [5, 40, 60, 39], [70, 70, 90, 90], [-9, -9, -1, -1]], [[255, 255, 255, 255]] * 4),
    "sixteen": ([[4 * i, 3 * i, 4 * i + 9, 3 * i + 20] for i in range(16)], [[16 * i, 255 - 16 * i, 7 * i, 255 - i] for i in range(16)]),
    "the whole image and beyond": ([[-(2 ** 31), -(2 ** 31), 2 ** 31 - 1, 2 ** 31 - 1]], [[0, 0, 0, 0]]),
    "none": ([], []),
}


@pytest.mark.parametrize("name", list(HAND_MADE))
def test_hand_made_rectangles(name):
    rects, fills = HAND_MADE[name]
    rects, fills = np.array(rects, np.int64).reshape(-1, 4), np.array(fills, np.uint8).reshape(-1, 4)
    src = P.pattern_rgba(64, 64, frame=7)
    lut = P.color_lut([1.1, 0.9, 1.2], [-0.1, 0.15, 0.0])
    for table in (None, lut):
        got = _all_ways(src, table, rects, fills)
        assert _same_bits(got, P.perturb(src, table, rects, fills))
    if name == "x1 < x0 and y1 < y0":
        assert _same_bits(_all_ways(src, None, rects, fills), src)
    if name == "later wins":
        assert _same_bits(_all_ways(src, None, rects, fills)[10, 35], np.array([1, 1, 1, 0], np.uint8))


def test_a_table_alone_and_an_unaligned_image():
    """No rectangles at all; an arbitrary table on every band, alpha included; and a dense HWC image at an odd address, which moves as
    bytes and must give what the aligned one gives."""
    from satnerf_amd import ops

    src = P.pattern_rgba(37, 53, frame=1)
    lut = ((np.arange(256)[None, :] * np.array([3, 5, 7, 11])[:, None] + np.array([1, 2, 3, 4])[:, None]) % 256).astype(np.uint8)
    want = P.perturb(src, lut)
    assert _same_bits(_all_ways(src, lut, None, None), want)
    assert _same_bits(_all_ways(src, None, None, None), src)  # nothing to do: a copy
    rects, fills = np.array([[3, 3, 40, 20]], np.int32), np.array([[4, 3, 2, 1]], np.uint8)
    buf = torch.zeros(src.size + 8, dtype=torch.uint8, device=DEV)
    odd = buf[1:1 + src.size].view(37, 53, 4)
    odd.copy_(torch.from_numpy(src))
    assert odd.data_ptr() % 4 == 1
    got = ops.blender_perturb(odd, lut, rects, fills, layout="hwc", out=odd)
    assert _same_bits(got.cpu().numpy(), P.perturb(src, lut, rects, fills))
    assert not buf[0].item() and not buf[1 + src.size:].any().item()  # nothing written around it


def test_arguments_ops_refuses():
    from satnerf_amd import ops

    img = torch.from_numpy(P.pattern_rgba(16, 16)).to(DEV)
    rects, fills = np.zeros((1, 4), np.int32), np.zeros((1, 4), np.uint8)
    with pytest.raises(ValueError, match="GPU"):
        ops.blender_perturb(img.cpu())
    with pytest.raises(ValueError, match="four bands"):
        ops.blender_perturb(img[:, :, :3].contiguous())
    with pytest.raises(ValueError, match="lut must be"):
        ops.blender_perturb(img, lut=np.zeros((3, 256), np.uint8))
    with pytest.raises(ValueError, match="come together"):
        ops.blender_perturb(img, rects=rects)
    with pytest.raises(ValueError, match="n <= 16"):
        ops.blender_perturb(img, rects=np.zeros((17, 4), np.int32), fills=np.zeros((17, 4), np.uint8))
    with pytest.raises(ValueError, match="fills must be"):
        ops.blender_perturb(img, rects=rects, fills=np.zeros((1, 3), np.uint8))
    with pytest.raises(ValueError, match="out must be"):
        ops.blender_perturb(img, out=torch.empty(16, 17, 4, dtype=torch.uint8, device=DEV))


def _scene(tmp_path, golden):
    images = {}
    P.write_scene(str(tmp_path), golden, images)
    return str(tmp_path), images.__getitem__


def _check_rays(got, want, bound):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert _same_bits(got[:, [0, 1, 2, 6, 7]], want[:, [0, 1, 2, 6, 7]])
    assert (np.abs(got[:, 3:6].astype(np.float64) - want[:, 3:6]) <= bound).all()


@pytest.mark.parametrize("variant", P.VARIANTS, ids="+".join)
def test_load_blender_perturbed_equals_the_reference_dataset(tmp_path, golden, variant):
    from satnerf_amd import data

    root, reader = _scene(tmp_path, golden)
    v = "+".join(variant)
    clean = data.load_blender(root, "train", img_wh=(WH, WH), device=DEV, reader=reader)
    rays, rgbs, ts = data.load_blender_perturbed(root, list(variant), "train", img_wh=(WH, WH), device=DEV, reader=reader)
    assert rays.is_cuda and rgbs.is_cuda and ts.is_cuda and ts.dtype == torch.int64
    print(f"{v}: {(rgbs.cpu().numpy() != golden[f'{v}_all_rgbs']).sum()} colour values differ from the reference")
    assert _same_bits(rgbs.cpu().numpy(), golden[f"{v}_all_rgbs"])
    assert _same_bits(ts.cpu().numpy(), golden[f"{v}_all_ts"].astype(np.int64))
    assert torch.equal(rays, clean[0]) and torch.equal(rgbs[:N], clean[1][:N]) and not torch.equal(rgbs[N:], clean[1][N:])
    tt = data.load_blender_perturbed(root, list(variant), "test_train", img_wh=(WH, WH), device=DEV, reader=reader)
    assert len(tt) == P.SCENE_TRAIN and [int(d["ts"][0]) for d in tt] == list(range(P.SCENE_TRAIN))
    for d in tt:
        assert sorted(d) == list(golden["test_train0_keys_perturbed"]) and all(t.is_cuda for t in d.values())
    d = {k: t.cpu().numpy() for k, t in tt[2].items()}
    assert _same_bits(d["rgbs"], golden[f"{v}_tt2_rgbs"]) and _same_bits(d["valid_mask"], golden[f"{v}_tt2_valid_mask"])
    assert _same_bits(d["original_rgbs"], golden["tt2_original_rgbs"]) and _same_bits(d["original_valid_mask"], golden["tt2_original_valid_mask"])
    assert _same_bits(d["ts"], golden["tt2_ts"]) and _same_bits(d["c2w"], golden["tt2_c2w"])
    _check_rays(d["rays"], golden["tt2_rays"], REF_BOUND)
    assert torch.equal(tt[0]["original_rgbs"], tt[0]["rgbs"])
    # an image that is already on the device is perturbed into a copy
    frame = torch.from_numpy(P.scene_images()[1]).to(DEV)
    keep = frame.clone()
    one, _ = data.blender_colors_from_image(frame, WH, WH, device=DEV, perturb=data.blender_perturbation(1, variant))
    assert torch.equal(frame, keep) and torch.equal(one, rgbs[N:2 * N])


def test_val_is_load_blender(tmp_path, golden):
    from satnerf_amd import data

    root, reader = _scene(tmp_path, golden)
    want = data.load_blender(root, "val", img_wh=(WH, WH), device=DEV, reader=reader)
    got = data.load_blender_perturbed(root, ["color", "occ"], "val", img_wh=(WH, WH), device=DEV, reader=reader)
    assert len(got) == len(want) == P.SCENE_VAL
    for a, b in zip(got, want):
        assert sorted(a) == sorted(b) == ["c2w", "rays", "rgbs", "ts", "valid_mask"] and all(torch.equal(a[k], b[k]) for k in a)


def test_a_batch_of_the_perturbed_scene_renders_with_the_classic_nerf(tmp_path, golden):
    from satnerf_amd import data, rendering
    from satnerf_amd.models import load_model

    root, reader = _scene(tmp_path, golden)
    rays, rgbs, ts = data.load_blender_perturbed(root, ["color", "occ"], "train", img_wh=(WH, WH), device=DEV, reader=reader)
    idx = torch.arange(0, rays.shape[0], 24, device=DEV)  # a batch by plain indexing: rows of all four frames
    args = O.default_args(model="nerf", n_samples=16, n_importance=8)
    models = {}
    for typ, seed in (("coarse", 1), ("fine", 2)):
        m = load_model(args)
        m.load_state_dict(O.procedural_nerf_params(args.fc_units, seed=seed))
        models[typ] = m.to(DEV).eval()
    with torch.no_grad():
        res = rendering.render_rays(models, args, rays[idx], ts[idx])
    n = idx.numel()
    assert n == 96 and set(ts[idx].tolist()) == {0, 1, 2, 3}
    assert res["rgb_coarse"].shape == res["rgb_fine"].shape == rgbs[idx].shape == (n, 3)
    for k, t in res.items():
        assert torch.isfinite(t).all(), k
    assert torch.isfinite(((res["rgb_fine"] - rgbs[idx]) ** 2).mean())  # the colours pair with the rays row for row
