"""scene.loc and the dataset's rays from its RPCs, host side: the fixture the reference's
SatelliteDataset.init_scaling_params produced (tests/golden/scene_loc/, made by tests/golden/make_scene_loc_golden.py) against the numpy
restatement (tests/scene_loc_reference.py), the file round trip, and load_rays' ordering rules with the kernels replaced by CPU stubs."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import scene_loc_reference as S
from tests.scene_loc_reference import SCENE, check_against_fixture, expected as _expected, scene_copy as _scene_copy

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GEN = os.path.join(HERE, "golden", "make_scene_loc_golden.py")
TRAIN, TEST = ["img_00", "img_01", "img_02"], ["img_03"]


def _generator_ref():
    spec = importlib.util.spec_from_file_location("make_scene_loc_golden", GEN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.REF


@pytest.mark.skipif(not os.path.isdir(os.path.join(_generator_ref(), "datasets")), reason="the reference tree is absent")
def test_fixture_regenerates_bit_equal():
    r = subprocess.run([sys.executable, GEN, "--check"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert r.returncode == 0 and "bit-equal" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_fixture_shape_and_contents():
    exp = _expected()
    assert not os.path.exists(os.path.join(SCENE, "scene.loc"))
    assert sorted(f for f in os.listdir(SCENE) if f.endswith(".json")) == [n + ".json" for n in TRAIN + TEST]  # expected.* is no image
    assert (exp["n_points_s1"] == 2 * 10718).all() and (exp["n_points_s2"] == 2 * 2663).all()
    for tag in ("s1", "s2"):
        for k in ("scale_", "offset_", "min_", "max_"):
            assert exp[k + tag].dtype == np.float32 and exp[k + tag].shape == (3,)
        # rpc_scaling_params in float32 is what the file must hold, bit for bit
        for a in range(3):
            sc, off = S.scaling_params(exp["min_" + tag][a], exp["max_" + tag][a])
            assert sc == exp["scale_" + tag][a] and off == exp["offset_" + tag][a]


def test_restatement_matches_the_reference_and_the_extremes_need_every_part():
    exp = _expected()
    images, _ = S.load_images(SCENE)
    for s, tag in ((1.0, "s1"), (2.0, "s2")):
        loc, per_image, pixels = S.scene_bounds(images, s)
        assert 2 * pixels == exp["n_points_" + tag][0]
        check_against_fixture(loc, exp, tag, per_image[:, 0::2].min(0), per_image[:, 1::2].max(0))
    assert np.isinf(S.scene_bounds(images, 2.0)[1][2]).all()  # the 1 x 1 image has no pixel at downscale 2
    # what the fixture pins at downscale 1: extremes from near AND far points, from the first and the last pixel of an image
    d = images[1]
    pts = S.image_points(d)
    n = pts.shape[0] // 2
    near, far = pts[:n], pts[n:]
    lo, hi = exp["min_s1"], exp["max_s1"]
    from_near = [near[:, a].min() == lo[a] for a in range(3)] + [near[:, a].max() == hi[a] for a in range(3)]
    from_far = [far[:, a].min() == lo[a] for a in range(3)] + [far[:, a].max() == hi[a] for a in range(3)]
    assert any(from_near) and any(from_far) and all(x or y for x, y in zip(from_near, from_far))
    ends = {int(np.argmin(pts[:, a])) % n for a in range(3)} | {int(np.argmax(pts[:, a])) % n for a in range(3)}
    assert n - 1 in ends, "the last pixel of the 64 x 96 image carries an extreme: a dropped tail changes the answer"


def _oracle_bounds_stub(calls):
    def stub(rpc, width, height, min_alt, max_alt, device, out=None, n_bad=None):
        assert width >= 1 and height >= 1, "an empty grid must not reach the ABI"
        calls.append((width, height))
        d = {"rpc": rpc, "height": height, "width": width, "min_alt": min_alt, "max_alt": max_alt}
        out.copy_(torch.from_numpy(S.footprint(S.image_points(d))))
        n_bad.zero_()
        return out, n_bad

    return stub


def test_scene_bounds_host_side_against_the_fixture(monkeypatch):
    """data.scene_bounds with the kernel replaced by the oracle: grid sizes, rescaled cameras, the skipped empty grid, the float32
    scaling parameters and the Python floats it returns."""
    from satnerf_amd import data, ops

    exp = _expected()
    images, paths = S.load_images(SCENE)
    for s, tag, sizes in ((1.0, "s1", [(29, 37), (96, 64), (1, 1), (70, 50)]), (2.0, "s2", [(14, 18), (48, 32), (35, 25)])):
        calls = []
        monkeypatch.setattr(ops, "rpc_scene_bounds", _oracle_bounds_stub(calls))
        loc, per_image = data.scene_bounds(images, img_downscale=s, device="cpu", names=paths, return_per_image=True)
        assert calls == sizes and per_image.shape == (4, 6) and per_image.dtype == np.float32
        assert sorted(loc) == sorted(S.KEYS) and all(type(v) is float and np.float32(v) == v for v in loc.values())
        check_against_fixture(loc, exp, tag, per_image[:, 0::2].min(0), per_image[:, 1::2].max(0))
        for a, axis in enumerate("XYZ"):  # same restatement underneath: exactly the reference's values
            assert loc[axis + "_scale"] == exp["scale_" + tag][a] and loc[axis + "_offset"] == exp["offset_" + tag][a]


def test_scene_bounds_names_the_bad_image(monkeypatch):
    from satnerf_amd import data, ops

    images, paths = S.load_images(SCENE)

    def stub(rpc, width, height, min_alt, max_alt, device, out=None, n_bad=None):
        n_bad.fill_(width * height if (width, height) == (96, 64) else 0)
        return out, n_bad

    monkeypatch.setattr(ops, "rpc_scene_bounds", stub)
    with pytest.raises(ValueError, match=r"img_01\.json.*n_bad = 6144"):
        data.scene_bounds(images, device="cpu", names=paths)


FP32_LOC = {"X_scale": 356.34375, "X_offset": float(np.float32(799437.6)), "Y_scale": 225.75, "Y_offset": float(np.float32(-5453281.3)),
            "Z_scale": float(np.float32(282.6251)), "Z_offset": float(np.float32(3199147.1))}


def test_scene_loc_round_trips_and_is_not_overwritten(tmp_path, monkeypatch):
    from satnerf_amd import data

    root = _scene_copy(tmp_path)
    seen = {}

    def fake_bounds(images, img_downscale=1.0, device="cuda", names=None, return_per_image=False):
        seen.update(n=len(images), s=img_downscale, names=names)
        return dict(FP32_LOC)

    monkeypatch.setattr(data, "scene_bounds", fake_bounds)
    with pytest.raises(FileNotFoundError, match="scene.loc.*required"):
        data.read_scene_loc(root)
    center, rng = data.init_scaling_params(root, img_downscale=2.0, device="cpu")
    assert seen["n"] == 4 and seen["s"] == 2.0 and [os.path.basename(p) for p in seen["names"]] == [n + ".json" for n in TRAIN + TEST]
    with open(os.path.join(root, "scene.loc")) as f:
        text = f.read()
    assert list(json.loads(text)) == list(S.KEYS) and text == json.dumps({k: FP32_LOC[k] for k in S.KEYS}, indent=2)
    assert center.dtype == torch.float32 and [np.float32(v) for v in center.tolist()] == [np.float32(FP32_LOC[a + "_offset"]) for a in "XYZ"]
    assert rng == FP32_LOC["X_scale"]
    c2, r2 = data.read_scene_loc(root)
    assert torch.equal(c2, center) and r2 == rng
    with pytest.raises(FileExistsError):
        data.init_scaling_params(root, device="cpu")
    FP32_LOC2 = dict(FP32_LOC, Y_scale=400.5)
    monkeypatch.setattr(data, "scene_bounds", lambda *a, **k: dict(FP32_LOC2))
    assert data.init_scaling_params(root, device="cpu", overwrite=True)[1] == 400.5


def test_json_without_rpc_is_named(tmp_path):
    from satnerf_amd import data

    root = _scene_copy(tmp_path)
    with open(os.path.join(root, "notes.json"), "w") as f:
        json.dump({"height": 3, "width": 3}, f)
    with pytest.raises(ValueError, match=r"rpc.*notes\.json"):
        data.init_scaling_params(root, device="cpu")
    assert not os.path.exists(os.path.join(root, "scene.loc"))


def _rays_stub(calls):
    """ops.rpc_rays on the CPU: rows that name their image (min_alt) and pixel, the cache rows likewise."""
    def stub(rpc, width, height, min_alt, max_alt, center, scene_range, sun_elevation_deg, sun_azimuth_deg, device, want_cache=False,
             out=None):
        n = width * height
        calls.append((width, height, float(rpc["row_scale"])))
        rays = torch.empty(n, 11) if out is None else out
        rays[:, 0] = min_alt
        rays[:, 1] = torch.arange(n, dtype=torch.float32)
        rays[:, 2:] = sun_azimuth_deg
        cache = torch.full((n, 8), float(max_alt)) if want_cache else None
        return rays, cache

    return stub


def test_load_rays_ordering_ids_and_cache(tmp_path, monkeypatch):
    from satnerf_amd import data, ops

    root = _scene_copy(tmp_path)
    with pytest.raises(FileNotFoundError, match="scene.loc.*required"):
        data.load_rays(root, device="cpu")
    with open(os.path.join(root, "scene.loc"), "w") as f:
        json.dump(FP32_LOC, f, indent=2)
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("img_00.json\n\nimg_01.json\nimg_02.json\n")  # blank lines are no images
    images, _ = S.load_images(root)
    calls = []
    monkeypatch.setattr(ops, "rpc_rays", _rays_stub(calls))
    all_rays, all_ids, index = data.load_rays(root, "train", device="cpu")
    assert index == [("img_00", 37, 29, 0), ("img_01", 64, 96, 1073), ("img_02", 1, 1, 7217)]
    assert all_rays.shape == (7218, 11) and all_rays.dtype == torch.float32 and all_ids.dtype == torch.int64 and all_ids.shape == (7218,)
    assert calls == [(29, 37, 37 / 2 + 10), (96, 64, 64 / 2 + 10), (1, 1, 1 / 2 + 10)]
    for t, (name, h, w, off) in enumerate(index):
        sl = slice(off, off + h * w)
        assert (all_ids[sl] == t).all() and (all_rays[sl, 0] == images[t]["min_alt"]).all()
        assert torch.equal(all_rays[sl, 1], torch.arange(h * w, dtype=torch.float32))
    # down-scaled: floor sizes, rescaled cameras, the empty image keeps its id but has no rows
    calls.clear()
    all_rays, all_ids, index = data.load_rays(root, "train", img_downscale=2.0, device="cpu")
    assert index == [("img_00", 18, 14, 0), ("img_01", 32, 48, 252), ("img_02", 0, 0, 1788)] and all_rays.shape == (1788, 11)
    assert calls == [(14, 18, (37 / 2 + 10) / 2), (48, 32, (64 / 2 + 10) / 2)] and sorted(set(all_ids.tolist())) == [0, 1]
    # validation: the first training image with id 0, then test.txt with ids n_train + k
    val = data.load_rays(root, "val", device="cpu")
    assert [(v["src_id"], v["ts"], v["h"], v["w"]) for v in val] == [("img_00", 0, 37, 29), ("img_03", 3, 50, 70)]
    assert all(v["rays"].shape == (v["h"] * v["w"], 11) for v in val) and (val[1]["rays"][:, 0] == images[3]["min_alt"]).all()
    with pytest.raises(ValueError, match="split"):
        data.load_rays(root, "test", device="cpu")
    # cache_dir: missing files are written, existing ones are read through rays_from_cache and the kernel is not called
    cache_dir = str(tmp_path / "cache")
    calls.clear()
    data.load_rays(root, "train", device="cpu", cache_dir=cache_dir)
    assert len(calls) == 3 and sorted(os.listdir(cache_dir)) == ["img_00.data", "img_01.data", "img_02.data"]
    c = torch.load(os.path.join(cache_dir, "img_01.data"))
    assert c.shape == (6144, 8) and c.dtype == torch.float32 and (c == images[1]["max_alt"]).all()
    calls.clear()
    center, rng = data.read_scene_loc(root)
    again, _, index2 = data.load_rays(root, "train", device="cpu", cache_dir=cache_dir)
    assert calls == [] and [i[3] for i in index2] == [0, 1073, 7217]
    want = data.rays_from_cache(os.path.join(cache_dir, "img_01.data"), center, rng, images[1]["sun_elevation"], images[1]["sun_azimuth"])
    assert torch.equal(again[1073:7217], want)
    with pytest.raises(ValueError, match="img_00.data holds 1073 rays"):
        data.load_rays(root, "train", img_downscale=2.0, device="cpu", cache_dir=cache_dir)


def test_create_scene_loc_runs_init_scaling_params_first(tmp_path, monkeypatch):
    from satnerf_amd import data, ops

    root = _scene_copy(tmp_path)
    seen = []
    monkeypatch.setattr(data, "scene_bounds", lambda images, img_downscale=1.0, **k: seen.append(img_downscale) or dict(FP32_LOC))
    monkeypatch.setattr(ops, "rpc_rays", _rays_stub([]))
    data.load_rays(root, "val", img_downscale=2.0, device="cpu", create_scene_loc=True)
    assert seen == [2.0] and os.path.exists(os.path.join(root, "scene.loc"))
    data.load_rays(root, "val", img_downscale=2.0, device="cpu", create_scene_loc=True)  # the file is there: not computed again
    assert seen == [2.0]


def test_abi_declared_in_header_and_binding():
    import inspect

    from satnerf_amd import _lib, data, ops

    with open(os.path.join(REPO, "include", "satrender.h")) as f:
        header = " ".join(f.read().split())
    assert ("int sr_rpc_scene_bounds(const double* rpc, int width, int height, double min_alt, double max_alt, float* bounds6, "
            "int64_t* n_bad, void* stream);") in header
    assert "satellite.py:139-151" in header
    res, args = _lib.SIGNATURES["sr_rpc_scene_bounds"]
    assert res is _lib._i and args == [_lib._vp, _lib._i, _lib._i, _lib._d, _lib._d, _lib._vp, _lib._vp, _lib._vp]
    assert list(inspect.signature(ops.rpc_scene_bounds).parameters) == ["rpc", "width", "height", "min_alt", "max_alt", "device", "out", "n_bad"]
    assert inspect.signature(ops.rpc_rays).parameters["out"].default is None
    for fn in ("scene_bounds", "init_scaling_params", "load_rays"):
        assert callable(getattr(data, fn))
