"""Depth supervision from tie points, host side: the numpy restatement (tests/depth_supervision_reference.py)
against the arrays the reference's SatelliteDataset_depth built on the committed scene (tests/golden/depth_supervision/, made by
tests/golden/make_depth_golden.py), and the fixture's own regeneration when the reference tree is present."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import depth_supervision_reference as D

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE = os.path.join(HERE, "golden", "depth_supervision")
GEN = os.path.join(HERE, "golden", "make_depth_golden.py")


def _fixture():
    z = np.load(os.path.join(SCENE, "reference.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def test_fixture_shape_and_contents():
    g = _fixture()
    images, pts3d, center, scene_range = D.load_scene(SCENE)
    n = sum(len(d["keypoints"]["pts3d_indices"]) for d in images)
    assert len(images) >= 9 and pts3d.dtype == np.float64 and pts3d.shape[1] == 3
    assert g["all_rays"].shape == (n, 11) and g["all_depths"].shape == (n, 2) and g["all_ids"].shape == (n, 1)
    assert g["errmat"].shape == (pts3d.shape[0], len(images)) and g["errmat"].dtype == np.float32
    assert np.array_equal(g["center"], center) and g["range"] == scene_range
    unseen = (g["errmat"] == 0).all(1)
    assert 0 < unseen.sum() < 0.1 * pts3d.shape[0] and (g["e"][unseen] == 0).all()  # unobserved points count with e = 0 in the mean
    assert (g["errmat"] > 5).any()  # the outliers


def test_restatement_matches_the_reference():
    g = _fixture()
    images, pts3d, center, scene_range = D.load_scene(SCENE)
    rays, depths, ts, e, e_mean, w, errmat = D.depth_supervision(images, pts3d, center, scene_range)
    assert np.array_equal(ts, g["all_ids"][:, 0].astype(np.int64))
    # same fp64 arithmetic, same fp32 cast: the origin may differ by one ulp of fp32 ECEF (libm), everything else to fp32 rounding
    assert np.abs(rays[:, :3] - g["all_rays"][:, :3]).max() <= 0.5 / scene_range + 1e-6
    assert np.abs(rays[:, 3:] - g["all_rays"][:, 3:]).max() < 2e-6
    assert np.abs(depths[:, 0] - g["all_depths"][:, 0]).max() <= np.sqrt(3) * 0.5 / scene_range + 1e-6
    # the error matrix: fp64 errors rounded to fp32, within one fp32 ulp of the reference's; the last duplicate wins in both
    ulp = np.spacing(np.maximum(np.abs(errmat), np.abs(g["errmat"])))
    assert (np.abs(errmat - g["errmat"]) <= ulp).all() and np.array_equal(errmat == 0, g["errmat"] == 0)
    # fp64 sums rounded once vs the reference's fp32 sums
    assert np.abs(e - g["e"]).max() <= 2e-6 * np.abs(g["e"]).max()
    assert abs(e_mean - g["e_mean"]) <= 2e-6 * g["e_mean"]
    assert np.abs(w - g["kp_weights"]).max() <= 5e-6
    assert np.abs(depths[:, 1] - g["all_depths"][:, 1]).max() <= 5e-6


def test_duplicate_observation_keeps_the_last():
    g = _fixture()
    images, pts3d, _, _ = D.load_scene(SCENE)
    for t, d in enumerate(images):
        ix = d["keypoints"]["pts3d_indices"]
        dup = [p for p in set(ix) if ix.count(p) > 1]
        for p in dup:
            last = len(ix) - 1 - ix[::-1].index(p)
            first = ix.index(p)
            cr = np.asarray(d["keypoints"]["2d_coordinates"], np.float64)
            errs = D.reprojection_errors(d["rpc"], cr[[first, last]], pts3d[[p, p]]).astype(np.float32)
            assert errs[0] != errs[1]
            assert abs(g["errmat"][p, t] - errs[1]) <= np.spacing(errs[1]) and abs(g["errmat"][p, t] - errs[0]) > np.spacing(errs[0])
            return
    pytest.fail("the fixture has no duplicated observation")


def _generator_ref():
    spec = importlib.util.spec_from_file_location("make_depth_golden", GEN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.REF


@pytest.mark.skipif(not os.path.isdir(os.path.join(_generator_ref(), "datasets")), reason="the reference tree is absent")
def test_fixture_regenerates_bit_equal():
    r = subprocess.run([sys.executable, GEN, "--check"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert r.returncode == 0 and "bit-equal" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
