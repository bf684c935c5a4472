"""scene.loc and the dataset's rays from its RPCs on the GPU (datasets/satellite.py:117-216): sr_rpc_scene_bounds
bit for bit against the min / max of the project's own rays, data.scene_bounds against the values the reference's
init_scaling_params produced on the committed dataset (tests/golden/scene_loc/), init_scaling_params and load_rays on a copy of it,
the non-finite camera, and graph capture."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import rpc_oracle as R
from tests import scene_loc_reference as S
from tests.scene_loc_reference import SCENE, check_against_fixture, expected as _expected, scene_copy as _scene_copy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bounds_from_rays(rpc, w, h, lo, hi):
    """[xmin, xmax, ymin, ymax, zmin, zmax] of cat([o, o + far * d]) in torch fp32 (a multiply, then an add) on sr_rpc_rays' (HW, 8)."""
    from satnerf_amd import ops

    _, r8 = ops.rpc_rays(rpc, w, h, lo, hi, [0.0, 0.0, 0.0], 1.0, 50.0, 150.0, DEV, want_cache=True)
    pts = torch.cat([r8[:, :3], r8[:, :3] + r8[:, 7:8] * r8[:, 3:6]], 0)
    assert torch.isfinite(pts).all()
    return torch.stack([pts.min(0).values, pts.max(0).values], 1).reshape(6)


def _same_bits(a, b):
    return torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


@pytest.mark.parametrize("down", [1.0, 2.0])
def test_bounds_are_the_extremes_of_the_projects_own_rays_bit_for_bit(down):
    from satnerf_amd import data, ops

    images, _ = S.load_images(SCENE)
    for d in images:
        h, w = int(d["height"] // down), int(d["width"] // down)
        if h * w == 0:
            continue
        rpc = data.rescale_rpc(d["rpc"], 1.0 / down)
        got, n_bad = ops.rpc_scene_bounds(rpc, w, h, d["min_alt"], d["max_alt"], DEV)
        assert got.shape == (6,) and got.dtype == torch.float32 and n_bad.dtype == torch.int64 and n_bad.item() == 0
        assert _same_bits(got, _bounds_from_rays(rpc, w, h, d["min_alt"], d["max_alt"])), (d["img"], down)
        again, _ = ops.rpc_scene_bounds(rpc, w, h, d["min_alt"], d["max_alt"], DEV)
        assert _same_bits(got, again)


def test_bounds_of_many_blocks_with_a_partial_last_wave_bit_for_bit():
    """301 x 299 = 89,999 pixels: 352 blocks (the launch has one thread per pixel and no grid cap, so there is no stride loop to
    cover), the last one with two full waves, one of 15 live lanes and one of none."""
    from satnerf_amd import ops

    h, w = 301, 299
    rpc = R.synthetic_rpc(5, height=h, width=w)
    got, n_bad = ops.rpc_scene_bounds(rpc, w, h, -25.0, 60.0, DEV)
    assert n_bad.item() == 0 and _same_bits(got, _bounds_from_rays(rpc, w, h, -25.0, 60.0))
    again, _ = ops.rpc_scene_bounds(rpc, w, h, -25.0, 60.0, DEV)
    assert _same_bits(got, again)


@pytest.mark.parametrize("down,tag", [(1.0, "s1"), (2.0, "s2")])
def test_scene_bounds_match_the_reference_fixture(down, tag):
    from satnerf_amd import data

    exp = _expected()
    images, paths = S.load_images(SCENE)
    loc, per_image = data.scene_bounds(images, img_downscale=down, device=DEV, names=paths, return_per_image=True)
    assert per_image.shape == (4, 6) and all(type(v) is float and np.float32(v) == v for v in loc.values())
    lo, hi = per_image[:, 0::2].min(0), per_image[:, 1::2].max(0)
    print(tag, "min", lo - exp["min_" + tag], "max", hi - exp["max_" + tag],
          "offset", [loc[a + "_offset"] - float(exp["offset_" + tag][k]) for k, a in enumerate("XYZ")],
          "scale", [loc[a + "_scale"] - float(exp["scale_" + tag][k]) for k, a in enumerate("XYZ")])
    check_against_fixture(loc, exp, tag, lo, hi)
    if down == 2.0:  # the 1 x 1 image has no pixel: no launch, no bound
        assert np.array_equal(per_image[2], np.array([np.inf, -np.inf] * 3, np.float32))


def test_init_scaling_params_writes_what_read_scene_loc_reads(tmp_path):
    from satnerf_amd import data

    root = _scene_copy(tmp_path)
    images, paths = S.load_images(root)
    center, rng = data.init_scaling_params(root, device=DEV)
    loc = data.scene_bounds(images, device=DEV, names=paths)
    with open(os.path.join(root, "scene.loc")) as f:
        assert json.load(f) == loc
    c2, r2 = data.read_scene_loc(root)
    assert torch.equal(center, c2) and rng == r2
    assert center.tolist() == [loc["X_offset"], loc["Y_offset"], loc["Z_offset"]] and rng == max(loc["X_scale"], loc["Y_scale"], loc["Z_scale"])
    check_against_fixture(loc, _expected(), "s1")
    with pytest.raises(FileExistsError):
        data.init_scaling_params(root, device=DEV)


def test_load_rays_builds_the_splits_and_uses_its_cache(tmp_path):
    from satnerf_amd import data

    root = _scene_copy(tmp_path)
    all_rays, all_ids, index = data.load_rays(root, "train", device=DEV, create_scene_loc=True)
    center, rng = data.read_scene_loc(root)
    images, _ = S.load_images(root)

    def block(d):
        return data.rays_from_rpc(d["rpc"], d["height"], d["width"], d["min_alt"], d["max_alt"], center, rng, d["sun_elevation"],
                                  d["sun_azimuth"], device=DEV)

    assert all_rays.is_cuda and _same_bits(all_rays, torch.cat([block(d) for d in images[:3]], 0))
    assert index == [("img_00", 37, 29, 0), ("img_01", 64, 96, 1073), ("img_02", 1, 1, 7217)]
    assert all_ids.dtype == torch.int64 and torch.equal(all_ids.cpu(), torch.repeat_interleave(torch.arange(3), torch.tensor([1073, 6144, 1])))
    val = data.load_rays(root, "val", device=DEV)
    assert [(v["src_id"], v["ts"], v["h"], v["w"]) for v in val] == [("img_00", 0, 37, 29), ("img_03", 3, 50, 70)]
    assert _same_bits(val[0]["rays"], block(images[0])) and _same_bits(val[1]["rays"], block(images[3]))
    # the cache: written by the first call, read by the second, same bytes out
    cache_dir = str(tmp_path / "cache")
    first, _, _ = data.load_rays(root, "train", device=DEV, cache_dir=cache_dir)
    files = sorted(os.listdir(cache_dir))
    assert files == ["img_00.data", "img_01.data", "img_02.data"] and _same_bits(first, all_rays)
    stamps = [os.path.getmtime(os.path.join(cache_dir, f)) for f in files]
    second, ids2, index2 = data.load_rays(root, "train", device=DEV, cache_dir=cache_dir)
    assert index2 == index and torch.equal(ids2, all_ids) and _same_bits(second, first)
    assert stamps == [os.path.getmtime(os.path.join(cache_dir, f)) for f in files]
    marked = torch.load(os.path.join(cache_dir, "img_01.data"))
    marked[5, 7] += 64.0  # a mark only the file carries: the next call must show it
    torch.save(marked, os.path.join(cache_dir, "img_01.data"))
    third, _, _ = data.load_rays(root, "train", device=DEV, cache_dir=cache_dir)
    want = first.clone()
    want[1073 + 5, 7] = (marked[5:6, 7] / rng).item()
    assert not _same_bits(third, first) and _same_bits(third, want)


def test_non_finite_camera_is_counted_and_named(tmp_path):
    from satnerf_amd import data, ops

    root = _scene_copy(tmp_path)
    images, paths = S.load_images(root)
    good = torch.stack([ops.rpc_scene_bounds(d["rpc"], d["width"], d["height"], d["min_alt"], d["max_alt"], DEV)[0] for d in images]).cpu()
    images[1]["rpc"]["row_num"][0] = float("nan")  # every localisation of this camera is NaN: arithmetic, no fault
    bounds = torch.zeros(4, 6, device=DEV)
    n_bad = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    for k, d in enumerate(images):
        ops.rpc_scene_bounds(d["rpc"], d["width"], d["height"], d["min_alt"], d["max_alt"], DEV, out=bounds[k], n_bad=n_bad[k:k + 1])
    assert n_bad.tolist() == [0, 64 * 96, 0, 0]
    assert bounds[1].tolist() == [np.inf, -np.inf] * 3  # no finite pixel: the neutral elements
    for k in (0, 2, 3):
        assert _same_bits(bounds[k], good[k])
    with pytest.raises(ValueError, match=r"img_01\.json.*n_bad = 6144 of its 6144"):
        data.scene_bounds(images, device=DEV, names=paths)
    with open(paths[1], "w") as f:
        json.dump(images[1], f)
    with pytest.raises(ValueError, match=r"img_01\.json.*n_bad = 6144"):
        data.init_scaling_params(root, device=DEV)
    assert not os.path.exists(os.path.join(root, "scene.loc"))


def test_bounds_replay_from_a_captured_graph():
    from satnerf_amd import ops

    h, w = 64, 96
    rpc = R.synthetic_rpc(107, height=h, width=w)
    eager, eager_bad = ops.rpc_scene_bounds(rpc, w, h, -32.0, 73.0, DEV)
    out = torch.zeros(6, device=DEV)
    n_bad = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.rpc_scene_bounds(rpc, w, h, -32.0, 73.0, DEV, out=out, n_bad=n_bad)  # loads the kernels before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.rpc_scene_bounds(rpc, w, h, -32.0, 73.0, DEV, out=out, n_bad=n_bad)
    out.fill_(3.0)
    n_bad.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(out, eager) and n_bad.item() == eager_bad.item() == 0
