"""Ray casting against a DSM raster, host side (no GPU): the brute-force reference of tests/heightfield_reference.py on hand-built cases,
the condition its stability filter puts on the GPU tests' inputs (at most 1 % of the rays left out), the chord approximation of the
scene-frame rays on the shared scenes, the prototypes and the argument checks of the three C entries, and the errors of the Python
layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import satnerf_oracle as O
from tests import heightfield_reference as H
from tests import sun_rays_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module", autouse=True)
def _library():
    from satnerf_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()


def _cast(hgt, A, B, r=1.0, skip=None):
    s, cell = H.cast_np(np.asarray(hgt, np.float32), r, np.array([A], np.float64), np.array([B], np.float64),
                        None if skip is None else np.array([skip]))
    return float(s[0]), int(cell[0])


# ---- the reference on hand-built cases ------------------------------------------------------------------------------------------------
TOWER = [[NAN, NAN, NAN], [NAN, 10.0, NAN], [NAN, NAN, NAN]]  # one column over x, y in [1, 2], r = 1


def test_single_column_top_wall_and_inside():
    # falling 1 m per metre along x at y = 1.5: z = 12.25 - 0.25 - x ... the top at z = 10
    s, cell = _cast(TOWER, (0.0, 1.5, 11.5), (3.0, 1.5, 8.5))
    assert cell == 4 and s == pytest.approx(0.5, abs=1e-15)  # z(s) = 11.5 - 3 s = 10 at s = 0.5, x = 1.5: on the roof
    s, cell = _cast(TOWER, (0.0, 1.5, 5.0), (3.0, 1.5, 5.0))
    assert cell == 4 and s == pytest.approx(1 / 3, abs=1e-15)  # level ray below the roof: the wall x = 1
    s, cell = _cast(TOWER, (1.25, 1.75, 3.0), (1.25, 1.75, 30.0))
    assert cell == 4 and s == 0.0  # a start inside the column
    assert _cast(TOWER, (0.0, 1.5, 10.5), (3.0, 1.5, 10.5)) == pytest.approx((NAN, -1), nan_ok=True)  # over the roof
    assert _cast(TOWER, (0.0, 1.5, 5.0), (0.9, 1.5, 5.0))[1] == -1  # ends before the wall


def test_nan_gap_between_two_columns():
    hgt = [[5.0, NAN, 8.0]]
    s, cell = _cast(hgt, (1.5, 0.5, 6.0), (3.5, 0.5, 6.0))  # starts over the gap, above the left column's roof
    assert cell == 2 and s == pytest.approx(0.25, abs=1e-15)
    s, cell = _cast(hgt, (0.5, 0.5, 6.0), (2.9, 0.5, 6.0))  # over the left roof, through the gap, into the right wall
    assert cell == 2 and s == pytest.approx(1.5 / 2.4, abs=1e-15)
    assert _cast(hgt, (1.1, 0.5, -50.0), (1.9, 0.5, -50.0))[1] == -1  # inside the gap, however low


def test_axis_parallel_rays():
    hgt = [[1.0, 1.0, 9.0], [1.0, 1.0, 1.0]]
    s, cell = _cast(hgt, (0.25, 0.5, 4.0), (3.25, 0.5, 4.0))  # dy = 0
    assert cell == 2 and s == pytest.approx(1.75 / 3.0, abs=1e-15)
    s, cell = _cast(hgt, (2.5, 1.75, 4.0), (2.5, -1.0, 4.0))  # dx = 0, towards smaller y
    assert cell == 2 and s == pytest.approx(0.75 / 2.75, abs=1e-15)
    s, cell = _cast(hgt, (1.5, 0.5, 20.0), (1.5, 0.5, 0.0))  # straight down
    assert cell == 1 and s == pytest.approx(0.95, abs=1e-15)
    # along the edge x = 2 the layout's half-open cells give the line to column 2
    assert _cast(hgt, (2.0, 0.25, 4.0), (2.0, 0.75, 4.0))[1] == 2 and _cast(hgt, (2.0, 0.25, 4.0), (2.0, 0.75, 4.0), skip=2)[1] == -1


def test_misses_and_entries_from_outside():
    hgt = np.full((4, 6), 3.0, np.float32)
    assert _cast(hgt, (-5.0, -1.0, 1.0), (10.0, -0.5, 1.0))[1] == -1  # passes beside the grid
    assert _cast(hgt, (-5.0, 1.0, 1.0), (-1.0, 1.0, 1.0))[1] == -1  # ends before it
    assert _cast(hgt, (NAN, 1.0, 1.0), (3.0, 1.0, 1.0))[1] == -1 and _cast(hgt, (0.0, 1.0, 1.0), (INF, 1.0, 1.0))[1] == -1
    s, cell = _cast(hgt, (-2.0, 1.5, 1.0), (2.0, 1.5, 1.0))  # enters through the wall x = 0 of cell (1, 0)
    assert cell == 6 and s == pytest.approx(0.5, abs=1e-15)
    s, cell = _cast(hgt, (-2.0, 1.5, 7.5), (6.0, 1.5, -0.5))  # enters above the surface, comes down on cell (1, 2) at x = 2.5
    assert cell == 6 + 2 and s == pytest.approx(0.5625, abs=1e-15)
    s, cell = _cast(hgt, (2.5, 9.0, 2.0), (2.5, -9.0, 2.0))  # from the south side: y runs against the rows
    assert cell == 3 * 6 + 2 and s == pytest.approx(5.0 / 18.0, abs=1e-15)


def test_tie_rule_on_an_exact_diagonal():
    """A segment through cell corners touches the two off-diagonal cells in one point each: they are not visited, however tall."""
    hgt = np.full((3, 3), 1.0, np.float32)
    hgt[0, 1] = hgt[1, 0] = hgt[1, 2] = hgt[2, 1] = 99.0
    assert _cast(hgt, (0.0, 0.0, 5.0), (3.0, 3.0, 5.0))[1] == -1 and _cast(hgt, (3.0, 3.0, 5.0), (0.0, 0.0, 5.0))[1] == -1
    assert _cast(hgt, (3.0, 0.0, 5.0), (0.0, 3.0, 5.0))[1] == -1
    hgt[1, 1] = 6.0
    s, cell = _cast(hgt, (0.0, 0.0, 5.0), (3.0, 3.0, 5.0))
    assert cell == 4 and s == pytest.approx(1 / 3, abs=1e-15)  # the diagonal cell itself, entered through its corner
    s, cell = _cast(hgt, (0.0, 0.25, 5.0), (2.75, 3.0, 5.0))  # a quarter cell off the diagonal: the neighbour is entered
    assert cell == 3 and s == pytest.approx(0.75 / 2.75, abs=1e-15)


def test_one_cell_raster():
    assert _cast([[2.0]], (0.5, 0.5, 5.0), (0.5, 0.5, 0.0)) == (pytest.approx(0.6, abs=1e-15), 0)
    assert _cast([[2.0]], (-1.0, 0.5, 1.0), (0.5, 0.5, 1.0)) == (pytest.approx(2 / 3, abs=1e-15), 0)
    assert _cast([[NAN]], (0.5, 0.5, 5.0), (0.5, 0.5, 0.0))[1] == -1 and _cast([[2.0]], (0.5, 0.5, 5.0), (0.5, 0.5, 2.5))[1] == -1
    mask, _ = H.shadow_mask_np([[2.0]], 0.5, S.sun_direction(8, 40))
    assert mask.tolist() == [[1.0]]
    bm, top = H.blockmax_np(np.array([[NAN]], np.float32))
    assert bm.tolist() == [[-INF]] and top == -INF


def test_mask_reference_on_a_step():
    """A wall of height 4 along x >= 3 r with the sun in the east at 45 degrees: the shadow reaches 4 m west of the wall."""
    hgt = np.zeros((1, 20), np.float32)
    hgt[0, 12:] = 4.0
    mask, _ = H.shadow_mask_np(hgt, 0.5, (1.0, 0.0, 1.0))
    # cell c (centre 0.5 c + 0.25) is shadowed when the wall at x = 6 is at most 4 m away: c >= 4
    assert mask[0].tolist() == [1.0] * 4 + [0.0] * 8 + [1.0] * 8
    assert H.shadow_mask_np(np.full((5, 7), 3.0, np.float32), 0.5, S.sun_direction(8, 40))[0].min() == 1.0  # a flat raster is lit


# ---- the condition on the GPU tests' inputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.SEGMENT_RASTERS)
def test_at_most_one_percent_of_the_segments_is_unstable(name):
    stable, s, cell = H.segment_truth(name)
    A, B = H.segments(name)
    d = B - A
    print(f"{name}: {len(stable)} segments, {(~stable).sum()} unstable, {(cell >= 0).sum()} hits, {(d[:, 2] > 0).sum()} rising, "
          f"{((d[:, 0] == 0) | (d[:, 1] == 0)).sum()} with a zero component")
    assert (~stable).mean() <= 0.01
    assert 0.2 <= (cell >= 0).mean() <= 0.9 or name == "1x1"  # both outcomes are exercised
    assert (d[:, 2] > 0).sum() == len(stable) // 2 and ((d[:, 0] == 0) | (d[:, 1] == 0)).sum() >= len(stable) // 10


@pytest.mark.parametrize("name,elevation,azimuth", H.SHADOW_CASES)
def test_at_most_one_percent_of_the_mask_is_unstable(name, elevation, azimuth):
    mask, stable = H.shadow_truth(name, elevation, azimuth)
    print(f"{name} at {elevation}/{azimuth}: {(~stable).sum()} unstable of {stable.size}, {(mask == 0).sum()} shadowed, {(mask == 1).sum()} lit")
    assert (~stable).mean() <= 0.01
    assert (np.isnan(mask) == np.isnan(H.raster(name))).all()


@pytest.mark.parametrize("name", ["jax", "cape_town"])
def test_at_most_one_percent_of_the_scene_rays_is_unstable(name):
    stable, s, cell = H.scene_truth(name)
    print(f"{name}: {len(stable)} rays, {(~stable).sum()} unstable at {H.DELTA_SCENE} m, {(cell >= 0).sum()} hits")
    assert (~stable).mean() <= 0.01 and (cell >= 0).mean() >= 0.5


# ---- the chord ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["jax", "cape_town"])
def test_chord_sag_on_the_sun_rays(name):
    """The walk takes the straight chord between the UTM images of a ray's ends.  The ray itself, straight in ECEF, rises above that
    chord in altitude by at most run^2 / (8 R) at its middle (R >= 6.3e6 m is below every radius of curvature of the ellipsoid)."""
    from tests.test_dsm_host import utm_forward_np

    sc = S.scene(name)
    s = sc["s"]
    rows, valid, _ = S.sun_rays_np(sc["rays"], sc["depth"], s["center"], s["scene_range"], s["max_alt"], sun_d=sc["sun"], bias_rel=1 / 64)
    rows = rows.astype(np.float32).astype(np.float64)[valid]
    UA, UB = H.utm_segments_np(rows, s["center"], s["scene_range"], s["zone"])
    lat, lon, alt = O.latlonalt_from_depth(rows, 0.5 * (rows[:, 6] + rows[:, 7]), np.asarray(s["center"], np.float64), s["scene_range"])
    e, n = utm_forward_np(lat, lon, s["zone"])
    run = np.hypot(UB[:, 0] - UA[:, 0], UB[:, 1] - UA[:, 1])
    # the altitudes of the three points in extended precision: fp64 leaves a noise of some 1e-9 m on each, more than the bound allows
    args = (s["center"], s["scene_range"])
    mid_alt = H.altitude_ld(rows, 0.5 * (rows[:, 6] + rows[:, 7]), *args)
    dz = np.abs(mid_alt - 0.5 * (H.altitude_ld(rows, rows[:, 6], *args) + H.altitude_ld(rows, rows[:, 7], *args))).astype(np.float64)
    assert np.finfo(np.longdouble).nmant > 52 and np.abs(mid_alt.astype(np.float64) - alt).max() <= 1e-8
    dh = np.hypot(e - 0.5 * (UA[:, 0] + UB[:, 0]), n - 0.5 * (UA[:, 1] + UB[:, 1]))
    bound = run ** 2 / (8 * 6.3e6) + 1e-9
    print(f"{name}: run <= {run.max():.1f} m, altitude offset <= {dz.max():.2e} m (bound {bound.max():.2e} m), horizontal offset <= {dh.max():.2e} m")
    assert (dz <= bound).all()
    assert dh.max() <= 1e-3  # recorded, and far below a cell


# ---- the C entries ------------------------------------------------------------------------------------------------------------------------
def test_the_three_entries_are_declared_and_bound():
    from satnerf_amd import _lib

    with open(os.path.join(ROOT, "include", "satrender.h")) as f:
        text = f.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, arity in (("sr_heightfield_blockmax", 6), ("sr_heightfield_cast", 22), ("sr_heightfield_shadow", 11)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, f"{name} is not declared in include/satrender.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        res, argtypes = _lib.SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == n_args == arity, (name, n_args, len(argtypes))
        assert argtypes[-1] is C.c_void_p
    assert "never accumulated" in text and "both" in text and "section 7.15" in text
    assert os.path.exists(os.path.join(ROOT, "satnerf_amd", "csrc", "heightfield.hip"))


_ptr = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731  (fake: never dereferenced, every check comes before the launch)


def _cast_call(**over):
    from satnerf_amd import _lib

    a = dict(hgt=4096, xsize=37, ysize=53, res=0.5, blockmax=4096, gmax=4096, accelerate=1, rays=4096, ray_stride=11, center=(1.0, 2.0, 3.0),
             range=210.0, zone=17, xoff=1000.25, yoff=2000.0, seg_a=None, seg_b=None, n=5, depth=4096, cell=4096, s=None, seg=4096)
    a.update(over)
    ctr = None if a["center"] is None else (C.c_double * 3)(*a["center"])
    _lib.call("sr_heightfield_cast", _ptr(a["hgt"]), a["xsize"], a["ysize"], a["res"], _ptr(a["blockmax"]), _ptr(a["gmax"]), a["accelerate"],
              _ptr(a["rays"]), a["ray_stride"], None if ctr is None else C.addressof(ctr), a["range"], a["zone"], a["xoff"], a["yoff"],
              _ptr(a["seg_a"]), _ptr(a["seg_b"]), a["n"], _ptr(a["depth"]), _ptr(a["cell"]), _ptr(a["s"]), _ptr(a["seg"]), None)


SEGS = dict(rays=None, seg=None, seg_a=4096, seg_b=4096)


@pytest.mark.parametrize("over", [
    dict(hgt=None), dict(xsize=0), dict(ysize=0), dict(xsize=1 << 16, ysize=1 << 15), dict(res=0.0), dict(res=-0.5), dict(res=NAN), dict(res=INF),
    dict(accelerate=2), dict(accelerate=-1), dict(blockmax=None), dict(gmax=None), dict(ray_stride=7), dict(zone=0), dict(zone=61),
    dict(range=0.0), dict(range=-1.0), dict(range=NAN), dict(range=INF), dict(xoff=NAN), dict(yoff=INF), dict(center=None),
    dict(center=(NAN, 0.0, 0.0)), dict(depth=None), dict(cell=None), dict(seg=None), dict(rays=None), dict(seg_a=4096), dict(seg_b=4096),
    dict(seg_a=4096, seg_b=4096), dict(SEGS, seg_a=None), dict(SEGS, seg_b=None), dict(SEGS, seg=4096), dict(SEGS, depth=None),
    dict(SEGS, cell=None), dict(SEGS, res=0.0), dict(SEGS, blockmax=None)])
def test_cast_argument_errors(over):
    from satnerf_amd import _lib

    with pytest.raises(_lib.SatRenderError, match="sr_heightfield_cast"):
        _cast_call(**over)


def test_empty_casts_launch_nothing_and_the_plain_walk_needs_no_maxima():
    _cast_call(n=0, depth=None, cell=None, seg=None)
    _cast_call(**dict(SEGS, n=0, depth=None, cell=None))
    _cast_call(n=0, accelerate=0, blockmax=None, gmax=None)


def _blockmax_call(**over):
    from satnerf_amd import _lib

    a = dict(hgt=4096, xsize=37, ysize=53, blockmax=4096, gmax=4096)
    a.update(over)
    _lib.call("sr_heightfield_blockmax", _ptr(a["hgt"]), a["xsize"], a["ysize"], _ptr(a["blockmax"]), _ptr(a["gmax"]), None)


@pytest.mark.parametrize("over", [dict(hgt=None), dict(blockmax=None), dict(gmax=None), dict(xsize=0), dict(ysize=-3), dict(xsize=1 << 16, ysize=1 << 15)])
def test_blockmax_argument_errors(over):
    from satnerf_amd import _lib

    with pytest.raises(_lib.SatRenderError, match="sr_heightfield_blockmax"):
        _blockmax_call(**over)


def _shadow_call(**over):
    from satnerf_amd import _lib

    a = dict(hgt=4096, xsize=37, ysize=53, res=0.5, blockmax=4096, gmax=4096, accelerate=1, sun=(0.3, 0.4, 0.8), bias=0.0, out=4096)
    a.update(over)
    sun = None if a["sun"] is None else (C.c_double * 3)(*a["sun"])
    _lib.call("sr_heightfield_shadow", _ptr(a["hgt"]), a["xsize"], a["ysize"], a["res"], _ptr(a["blockmax"]), _ptr(a["gmax"]), a["accelerate"],
              None if sun is None else C.addressof(sun), a["bias"], _ptr(a["out"]), None)


@pytest.mark.parametrize("over", [
    dict(hgt=None), dict(xsize=0), dict(ysize=0), dict(xsize=1 << 16, ysize=1 << 15), dict(res=0.0), dict(res=-1.0), dict(res=NAN), dict(res=INF),
    dict(accelerate=2), dict(blockmax=None), dict(gmax=None), dict(gmax=None, accelerate=0), dict(out=None), dict(sun=None),
    dict(sun=(0.0, 0.0, 0.0)), dict(sun=(0.3, 0.4, 0.0)), dict(sun=(0.3, 0.4, -0.5)), dict(sun=(NAN, 0.4, 0.5)), dict(sun=(0.3, INF, 0.5)),
    dict(bias=-0.1), dict(bias=NAN), dict(bias=INF)])
def test_shadow_argument_errors(over):
    from satnerf_amd import _lib

    with pytest.raises(_lib.SatRenderError, match="sr_heightfield_shadow"):
        _shadow_call(**over)


# ---- the Python layer without a GPU --------------------------------------------------------------------------------------------------------
def test_python_layer_errors():
    from satnerf_amd import dsm, ops

    hgt = torch.zeros(5, 7)
    d = dsm.DSM(hgt, torch.ones(5, 7), 1000.25, 2000.0, 0.5, "17R")
    rays = torch.zeros(4, 11)
    scene = (np.array([1.0, 2.0, 3.0]), 210.0)
    for fn in (lambda: ops.heightfield_blockmax(hgt), lambda: ops.heightfield_shadow(hgt, 0.5, (0.3, 0.4, 0.8)),
               lambda: ops.heightfield_cast(hgt, 0.5, seg_a=torch.zeros(4, 3, dtype=torch.float64), seg_b=torch.zeros(4, 3, dtype=torch.float64)),
               lambda: dsm.cast_rays(d, rays, *scene), lambda: dsm.shadow_mask(d, (0.3, 0.4, 0.8)),
               lambda: dsm.sun_visibility_from_dsm(d, rays, torch.zeros(4), *scene, 49.0, n_samples=64)):
        with pytest.raises(ValueError, match="GPU"):
            fn()
    with pytest.raises(ValueError, match="DSM"):
        dsm.cast_rays(hgt, rays, *scene)
    with pytest.raises(ValueError, match="DSM"):
        dsm.shadow_mask(hgt, (0.3, 0.4, 0.8))