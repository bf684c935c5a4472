"""Cloud fusion on the host: the numpy restatement of tests/cloud_grid_reference.py pinned to the fixtures the
reference's eval_s2p.project_cloud_into_utm_grid wrote (rule "nearest") and to rasterize_np (rule "floor"), the fixture recipe's
--check, the argument checks of the Python interface, and the C ABI's declaration.  CPU only."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cloud_grid_reference as R
from tests.test_dsm_host import rasterize_np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference"


@pytest.mark.parametrize("name", R.FIXTURES)
def test_nearest_rule_matches_the_reference_fixtures(name):
    g = R.load(name)
    xyz, bb, d = g["xyz"], g["bb"], float(g["definition"])
    assert np.isfinite(xyz).all() and 500 <= len(xyz) <= 5000
    map_w, map_h = R.map_size(bb, d)
    args = (xyz[:, 0], xyz[:, 1], xyz[:, 2], bb[0], bb[2], d, map_w, map_h, "nearest")
    for mode in ("min", "max", "med"):
        out, _ = R.cloud_grid_np(*args, mode)
        assert out.shape == g[mode].shape == (map_h, map_w)
        assert R.same_bits(out, g[mode]), mode
    avg, count = R.cloud_grid_np(*args, "avg")
    assert (np.isnan(avg) == np.isnan(g["avg"])).all() and ((count == 0) == np.isnan(avg)).all()
    ok = ~np.isnan(avg)
    err = np.abs(avg[ok] - g["avg"][ok])
    assert (err <= R.avg_bound_np(*args)[ok]).all(), err.max()


def test_fixtures_hold_the_cases_they_were_built_for():
    # ties: x0 - 0.25 is kept in column 0, the last centre + 0.25 by half-even, one step beyond is dropped
    g = R.load("ties")
    bb, d = g["bb"], float(g["definition"])
    assert R.map_size(bb, d) == (5, 4)
    x, y, z = g["xyz"].T
    one = lambda px, py: R.cloud_grid_np(np.array([px]), np.array([py]), np.array([1.0]), bb[0], bb[2], d, 5, 4, "nearest", "min")[1]
    assert any((x == 101.0) & (y == 51.75)) and one(101.0, 51.75).sum() == 0  # row 3.5 -> 4: dropped
    assert any((x == 101.0) & (y == 49.75)) and one(101.0, 49.75)[3, 2] == 1  # row -0.5 -> -0: the reference's row 0, flipped to the last
    assert any(x == bb[0] - 0.25) and one(bb[0] - 0.25, 50.0)[3, 0] == 1
    assert any(x == bb[0] + 4 * d + 0.25) and one(bb[0] + 4 * d + 0.25, 50.0)[3, 4] == 1  # 4.5 -> 4: kept
    assert any(x == bb[0] - 0.5) and one(bb[0] - 0.5, 50.0).sum() == 0 and one(bb[0] + 4 * d + 0.5, 50.0).sum() == 0
    assert np.isfinite(g["min"]).all()  # every cell of the 4 x 5 map is hit
    # counts: the cell populations the sort's paths switch on
    g = R.load("counts")
    w, h = R.map_size(g["bb"], float(g["definition"]))
    _, count = R.cloud_grid_np(*g["xyz"].T, g["bb"][0], g["bb"][2], float(g["definition"]), w, h, "nearest", "min")
    assert sorted(count.ravel().tolist()) == [0, 0, 1, 2, 3, 4, 63, 64, 65, 1500]
    # city: empty cells, negative altitudes, duplicate altitudes inside a cell; metric: a definition that is no power of two
    g = R.load("city")
    w, h = R.map_size(g["bb"], float(g["definition"]))
    assert (w, h) == (40, 30) and np.isnan(g["med"]).any() and (g["min"][~np.isnan(g["min"])] < 0).any()
    zs, start, count = R.segments_np(*g["xyz"].T, g["bb"][0], g["bb"][2], float(g["definition"]), w, h, "nearest")
    cell_of = np.repeat(np.arange(w * h), count)
    assert ((np.diff(zs) == 0) & (np.diff(cell_of) == 0)).any()
    g = R.load("metric")
    assert float(g["definition"]) == 0.3 and g["xyz"][:, 0].min() > 4e5 and g["xyz"][:, 1].min() > 3.3e6
    for name in R.FIXTURES:  # no -0.0 anywhere, so no cell can hold both zeros
        assert not (np.signbit(R.load(name)["xyz"][:, 2]) & (R.load(name)["xyz"][:, 2] == 0)).any()
        assert os.path.getsize(os.path.join(R.GOLDEN, name + ".npz")) < 1 << 20


def test_floor_rule_matches_the_rasteriser_restatement():
    rng = np.random.default_rng(21)
    xoff, yoff, res, xsize, ysize = 435000.0, 3354000.0, 0.5, 23, 17
    # at most one point per cell, some cells empty, some points on cell edges, outside the grid and non-finite
    pick = rng.permutation(xsize * ysize)[:250]
    j, c = pick // xsize, pick % xsize
    fx, fy = rng.uniform(0, 1, len(pick)), rng.uniform(0, 1, len(pick))
    fx[:40], fy[20:60] = 0.0, 0.0  # exactly on the west / north edge of the cell
    east, north = xoff + (c + fx) * res, yoff - (j + fy) * res
    alt = rng.uniform(-5, 50, len(pick))
    east = np.concatenate([east, [xoff + xsize * res, xoff - 1e-9, xoff + 1.0, np.nan, xoff + 1.0, np.inf]])
    north = np.concatenate([north, [yoff - 1.0, yoff - 1.0, yoff - ysize * res, yoff - 1.0, -np.inf, yoff - 1.0]])
    alt = np.concatenate([alt, [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]])
    alt[5] = np.nan
    want, weight = rasterize_np(east, north, alt, xoff, yoff, res, xsize, ysize, 0, float("inf"))
    assert weight.max() == 1
    for mode in R.MODES:
        got, count = R.cloud_grid_np(east, north, alt, xoff, yoff, res, xsize, ysize, "floor", mode)
        assert R.same_bits(got, want), mode
        assert (count == weight).all()


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_fixture_recipe_check_passes():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "golden", "make_cloud_grid_golden.py"), "--check"],
                       capture_output=True, text=True, env={**os.environ, "PYTHONDONTWRITEBYTECODE": "1"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("bit-equal") == len(R.FIXTURES)


def test_python_interface_rejects_cpu_tensors_and_bad_modes():
    from satnerf_amd import dsm

    xyz = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="no CPU path"):
        dsm.project_cloud_into_utm_grid(xyz, [0, 1, 0, 1], 0.5, "med")
    with pytest.raises(ValueError, match="mode"):
        dsm.project_cloud_into_utm_grid(xyz, [0, 1, 0, 1], 0.5, "mean")
    e = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(ValueError, match="no CPU path"):
        dsm.dsm_from_clouds(e, e, e, roi=[0.0, 0.0, 4, 0.5])
    with pytest.raises(ValueError, match="no CPU path"):
        dsm.dsm_from_clouds([e, e], [e, e], [e, e], roi=[0.0, 0.0, 4, 0.5])
    with pytest.raises(ValueError, match="mode"):
        dsm.dsm_from_clouds(e, e, e, roi=[0.0, 0.0, 4, 0.5], mode="median")
    with pytest.raises(ValueError, match="mode"):
        dsm.render_fused_dsm({}, [], None, None, 1.0, mode="mean")


def test_header_declares_and_library_exports_sr_cloud_grid():
    from satnerf_amd import _lib

    header = open(os.path.join(REPO, "include", "satrender.h")).read()
    assert "int sr_cloud_grid(" in header and "int sr_cloud_grid_scratch(" in header and "eval_s2p.py:175-226" in header
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert raw.sr_cloud_grid is not None and raw.sr_cloud_grid_scratch is not None
    # host-only checks of the C entry: the scratch size, and the int32 limits
    lib = _lib.lib()
    nbytes = ctypes.c_int64(0)
    assert lib.sr_cloud_grid_scratch(1000, 40, 30, ctypes.byref(nbytes)) == 0
    assert nbytes.value >= 12 * 1000 + 8 * 1200 and nbytes.value % 8 == 0
    assert lib.sr_cloud_grid_scratch(1 << 31, 40, 30, ctypes.byref(nbytes)) != 0
    assert lib.sr_cloud_grid_scratch(1000, 1 << 16, 1 << 15, ctypes.byref(nbytes)) != 0
    assert lib.sr_cloud_grid_scratch(1000, 0, 30, ctypes.byref(nbytes)) != 0
