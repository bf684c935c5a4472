"""Nadir DSM rays, host side (no GPU): the fp64 restatement of tests/ortho_reference.py against the forward projection and the
ECEF -> geodetic yardsticks, and the argument checks of the two entry points and their Python wrappers."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import satnerf_oracle as O
from oracle.rpc_oracle import latlon_to_ecef
from satnerf_amd import _lib, data, dsm
from tests import ortho_reference as R
from tests.test_dsm_host import central_meridian, utm_forward_np


@pytest.fixture(scope="module", autouse=True)
def _library():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()


# ---- the restated inverse against the forward ------------------------------------------------------------------------------------
@pytest.mark.parametrize("zone", [17, 31, 34])
def test_restated_inverse_against_the_forward(zone):
    lat, dlon = np.meshgrid(np.linspace(-60, 60, 121), np.linspace(-3.5, 3.5, 29))  # southern points included
    lat, lon = lat.ravel(), central_meridian(zone) + dlon.ravel()
    east, north = utm_forward_np(lat, lon, zone)
    lat2, lon2 = R.utm_inverse_np(east, north, zone)
    assert np.abs(lat2 - lat).max() <= 1e-11 and np.abs(lon2 - lon).max() <= 1e-11  # forward, then inverse
    e2, n2 = utm_forward_np(lat2, lon2, zone)
    assert np.abs(e2 - east).max() <= 1e-6 and np.abs(n2 - north).max() <= 1e-6  # inverse, then forward
    assert (north[lat < 0] < 0).all()  # false northing 0 in the south


# ---- the restated rays -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [R.jax, R.cape_town])
def test_restated_rays(make):
    s = make(37, 53)
    rays, latlon = R.ortho_rays_np(**s)
    lat, lon = latlon[:, 0], latlon[:, 1]
    column = s["max_alt"] - s["min_alt"]
    # the direction is the normalised difference of the ECEF points at min_alt and max_alt, up to that difference's cancellation
    hi, lo = np.stack(latlon_to_ecef(lat, lon, s["max_alt"]), 1), np.stack(latlon_to_ecef(lat, lon, s["min_alt"]), 1)
    diff = lo - hi
    length = np.linalg.norm(diff, axis=1)
    err = np.abs(rays[:, 3:6] - diff / length[:, None]).max()
    bound = 4 * np.spacing(6.4e6) / column
    print(f"analytic direction vs ECEF difference: {err:.2e} (bound {bound:.2e})")
    assert err <= bound
    assert np.abs(np.linalg.norm(rays[:, 3:6], axis=1) - 1).max() <= 4e-16
    assert np.abs(length - column).max() <= 1e-8  # the vertical is a straight line of that length
    assert np.abs(rays[:, 7] * s["scene_range"] - column).max() <= 1e-8 and (rays[:, 6] == 0).all()
    # the origin is the point at max_alt: de-normalised, it is ECEF(max_alt) to fp64 rounding of an ECEF coordinate
    assert np.abs(rays[:, 0:3] * s["scene_range"] + s["center"] - hi).max() <= 4 * np.spacing(6.4e6)


def test_cell_order_agrees_with_grid_from_roi():
    roi = np.array([435400.25, 3354000.0, 6.0, 0.5])  # {aoi}_DSM.txt: lower-left corner, size, resolution
    grid = dsm.grid_from_roi(roi)
    east, north = R.cell_centres(grid)
    assert east.shape == (6, 6)
    assert east[0, 0] == roi[0] + 0.25 and north[0, 0] == roi[1] + 6 * 0.5 - 0.25  # row 0 is the top (north) row
    assert east[5, 5] == roi[0] + 2.75 and north[5, 5] == roi[1] + 0.25
    # row-major: the flat index of cell (j, c) is j * xsize + c, the cell dsm.DSM documents
    j, c = 4, 1
    e, n = east.ravel()[j * 6 + c], north.ravel()[j * 6 + c]
    assert int(np.floor((e - grid[0]) / grid[4])) == c and int(np.floor((grid[1] - n) / grid[4])) == j


def _points_along(s, seed):
    """Points at random depths along the restated fp32 rays, through the fp64 ECEF -> geodetic -> UTM yardsticks."""
    rays64, _ = R.ortho_rays_np(**s)
    rays = rays64.astype(np.float32)
    depth = np.random.default_rng(seed).uniform(0, rays[:, 7]).astype(np.float32)
    lat, lon, alt = O.latlonalt_from_depth(rays, depth, s["center"], s["scene_range"])
    east, north = utm_forward_np(lat, lon, s["zone"])
    return depth, east, north, alt


@pytest.mark.parametrize("make", [R.jax, R.cape_town])
def test_points_land_in_their_own_cell_at_the_closed_form_altitude(make):
    s = make(37, 37)  # 0.5 m cells, x offset ending in .25, range 210 m
    xoff, yoff, xsize, ysize, r = s["grid"]
    assert (xoff * 4) % 4 == 1.0
    depth, east, north, alt = _points_along(s, 3)
    c, j = np.floor((east - xoff) / r).astype(int), np.floor((yoff - north) / r).astype(int)
    jj, cc = np.meshgrid(np.arange(ysize), np.arange(xsize), indexing="ij")
    assert (c == cc.ravel()).all() and (j == jj.ravel()).all()
    ce, cn = R.cell_centres(s["grid"])
    drift = max(np.abs(east - ce.ravel()).max(), np.abs(north - cn.ravel()).max())
    closed = s["max_alt"] - depth.astype(np.float64) * s["scene_range"]
    print(f"drift from the cell centre {drift:.2e} m (margin {r / 2} m), altitude {np.abs(alt - closed).max():.2e} m")
    assert np.abs(alt - closed).max() <= 1e-3


def test_fp64_normalisation_beats_the_reference_fp32_origin():
    """What the one rounding buys: the reference casts the ECEF origin to fp32 before subtracting the centre."""
    s = R.jax(37, 37)
    rays64, latlon = R.ortho_rays_np(**s)
    hi = np.stack(latlon_to_ecef(latlon[:, 0], latlon[:, 1], s["max_alt"]), 1)
    c32, r32 = s["center"].astype(np.float32), np.float32(s["scene_range"])
    ref = (hi.astype(np.float32) - c32) / r32  # normalize_rays in the tensor's own fp32
    back = lambda o: o.astype(np.float64) * s["scene_range"] + s["center"]  # noqa: E731
    err_ref = np.linalg.norm(back(ref) - hi, axis=1).max()
    err_new = np.linalg.norm(back(rays64[:, 0:3].astype(np.float32)) - hi, axis=1).max()
    print(f"origin error: fp32 before the subtraction {err_ref:.3f} m, fp64 then one rounding {err_new:.2e} m")
    assert err_new <= 3 * 2.0**-24 * np.abs(rays64[:, 0:3]).max() * s["scene_range"] * 1.01 and err_ref > 100 * err_new


# ---- argument errors: nothing reaches a device -------------------------------------------------------------------------------------
def _ortho_call(**over):
    a = dict(xoff=435000.25, yoff=3354000.0, res=0.5, xsize=4, ysize=3, zone=17, min_alt=-24.0, max_alt=49.0, range=210.0, stride=11)
    a.update(over)
    ctr, sun = (C.c_double * 3)(1.0, 2.0, 3.0), (C.c_float * 3)(0.0, 0.0, 1.0)
    fake = C.c_void_p(4096)  # never dereferenced: every check comes before the launch
    _lib.call("sr_ortho_rays", a["xoff"], a["yoff"], a["res"], a["xsize"], a["ysize"], a["zone"], a["min_alt"], a["max_alt"], C.addressof(ctr),
              a["range"], sun, fake, a["stride"], None, None)


@pytest.mark.parametrize("over", [dict(zone=0), dict(zone=61), dict(min_alt=49.0), dict(min_alt=50.0), dict(res=0.0), dict(res=-0.5),
                                  dict(res=float("nan")), dict(xsize=0), dict(ysize=0), dict(xsize=65536, ysize=32768), dict(stride=10),
                                  dict(range=0.0), dict(max_alt=float("inf"))])
def test_ortho_rays_argument_errors(over):
    with pytest.raises(_lib.SatRenderError, match="sr_ortho_rays"):
        _ortho_call(**over)


@pytest.mark.parametrize("zone", [0, 61, -3])
def test_utm_to_latlon_argument_errors(zone):
    fake = C.c_void_p(4096)
    with pytest.raises(_lib.SatRenderError, match="zone must be in 1..60"):
        _lib.call("sr_utm_to_latlon", fake, fake, 5, zone, fake, fake, None)
    _lib.call("sr_utm_to_latlon", None, None, 0, 17, None, None, None)  # n == 0 launches nothing


def test_python_wrappers_reject_cpu_tensors_and_ambiguous_grids():
    s = R.jax(4, 3)
    e = torch.zeros(3, dtype=torch.float64)
    with pytest.raises(ValueError):
        dsm.lonlat_from_utm(e, e, 17)
    with pytest.raises(ValueError):
        data.ortho_rays(device="cpu", **s)
    with pytest.raises(ValueError):
        data.ortho_rays(out=torch.zeros(12, 13), **s)
    with pytest.raises(ValueError):
        data.ortho_rays(**{**s, "min_alt": 60.0})
    with pytest.raises(ValueError):
        data.ortho_rays(**{**s, "grid": (0.0, 0.0, 0, 3, 0.5)})
    with pytest.raises(ValueError):
        data.ortho_rays(**{**s, "zone": 61})
    with pytest.raises(ValueError):
        dsm.ortho_dsm_from_depth(torch.zeros(12), s["grid"], 49.0, 210.0)
    roi = np.array([435400.0, 3354000.0, 8.0, 0.5])
    for kw in (dict(roi=roi, grid=s["grid"]), dict()):
        with pytest.raises(ValueError, match="exactly one of roi= and grid="):
            dsm.render_ortho_dsm({}, 0, None, s["center"], 210.0, -24.0, 49.0, s["sun_d"], **kw)
