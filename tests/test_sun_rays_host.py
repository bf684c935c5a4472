"""Sun rays, host side (no GPU): the fp64 restatement of tests/sun_rays_reference.py pinned from independent routes (unit length, the
altitude where a ray ends, its direction by finite differences in geodetic coordinates, the edge cases), the prototypes and the
argument checks of the two C entries, and the errors of the Python layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import satnerf_oracle as O
from tests import ortho_reference as R
from tests import sun_rays_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["jax", "cape_town"]


@pytest.fixture(scope="module", autouse=True)
def _library():
    from satnerf_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()


def _restated(name):
    sc = S.scene(name)
    s = sc["s"]
    rows, valid, lla = S.sun_rays_np(sc["rays"], sc["depth"], s["center"], s["scene_range"], s["max_alt"], sun_d=sc["sun"], bias_rel=1 / 64)
    return sc, s, rows, valid, lla


def _geodetic(E):
    zero = np.zeros((E.shape[0], 6))
    zero[:, 0:3] = E
    return O.latlonalt_from_depth(zero, np.zeros(E.shape[0]), np.zeros(3), 1.0)


# ---- the restatement from independent routes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_directions_have_unit_length(name):
    _, _, rows, valid, _ = _restated(name)
    assert valid.all()
    err = np.abs(np.linalg.norm(rows[:, 3:6], axis=1) - 1).max()
    print(f"{name}: | |dir| - 1 | <= {err:.1e}")
    assert err <= 1e-15


@pytest.mark.parametrize("name", NAMES)
def test_the_ray_ends_at_max_alt_up_to_the_curvature_drop(name):
    """far is where the ray reaches max_alt on the tangent plane of its start; the ellipsoid falls away from that plane by at most
    run^2 / (2 R) over a horizontal run, and 6.3e6 m is below every radius of curvature of the ellipsoid."""
    sc, s, rows, _, _ = _restated(name)
    assert (rows[:, 7] > rows[:, 6]).all()  # every point of these scenes lies below max_alt by more than the bias
    end = (rows[:, 0:3] + rows[:, 3:6] * rows[:, 7:8]) * s["scene_range"] + s["center"]
    alt_end = _geodetic(end)[2]
    run = rows[:, 7] * s["scene_range"] * np.cos(np.radians(sc["elevation"]))
    bound = run ** 2 / (2 * 6.3e6) + 1e-6
    err = alt_end - s["max_alt"]
    print(f"{name}: altitude at the end off max_alt by at most {np.abs(err).max():.2e} m (bound {bound.max():.2e} m)")
    assert (np.abs(err) <= bound).all()


@pytest.mark.parametrize("name", NAMES)
def test_direction_by_finite_differences(name):
    """One metre along dir moves latitude, longitude and altitude by the sun vector's north, east and up components."""
    sc, s, rows, _, (lat, lon, alt) = _restated(name)
    E = rows[:, 0:3] * s["scene_range"] + s["center"]
    lat1, lon1, alt1 = _geodetic(E + rows[:, 3:6] * 1.0)
    phi = np.radians(lat)
    w2 = 1 - S.E2_WGS84 * np.sin(phi) ** 2
    M, N = S.A_WGS84 * (1 - S.E2_WGS84) / w2 ** 1.5, S.A_WGS84 / np.sqrt(w2)  # meridional and prime-vertical radii
    moved = np.stack([np.radians(lon1 - lon) * (N + alt) * np.cos(phi), np.radians(lat1 - lat) * (M + alt), alt1 - alt], 1)
    hat = sc["sun"] / np.linalg.norm(sc["sun"])
    err = np.abs(moved - hat).max()
    print(f"{name}: finite differences against (e, n, u) {err:.1e}")
    assert err <= 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_zenith_sun_on_a_nadir_ray_points_back_along_it(name):
    sc = S.scene(name)
    s = sc["s"]
    rays64 = R.ortho_rays_np(**s)[0]  # not rounded: the direction is the inward ellipsoid normal to fp64
    rows, valid, _ = S.sun_rays_np(rays64, sc["depth"], s["center"], s["scene_range"], s["max_alt"], sun_d=(0.0, 0.0, 2.5))
    err = np.abs(rows[:, 3:6] + rays64[:, 3:6]).max()
    print(f"{name}: dir + d = {err:.1e}")
    assert valid.all() and err <= 1e-15
    assert (rows[:, 8:11] == [0.0, 0.0, 2.5]).all()  # the sun columns carry the vector as given, not normalised


def test_invalid_rays_and_points_above_max_alt():
    sc = S.scene("jax")
    s = sc["s"]
    rays, depth = sc["rays"][:12].copy(), sc["depth"][:12].copy()
    depth[1], depth[2], depth[3] = np.nan, np.inf, -np.inf
    rays[4, 8:11] = 0.0
    rays[5, 8:11] = (0.3, 0.4, -0.1)  # below the horizon
    rays[6, 8:11] = (0.3, 0.4, 0.0)  # on it
    rays[7, 8:11] = (np.nan, 0.4, 0.5)
    rays[8, 8:11] = (np.inf, 0.4, 0.5)
    depth[9], depth[10] = -0.01, 0.0  # above max_alt, and exactly at the ray's origin on it
    rows, valid, _ = S.sun_rays_np(rays, depth, s["center"], s["scene_range"], s["max_alt"], bias_rel=1 / 64)
    assert valid.tolist() == [True, False, False, False, False, False, False, False, False, True, True, True]
    bad = ~valid
    assert np.isfinite(rows[bad, 0:8]).all() and (rows[bad, 0:6] == rays[bad, 0:6]).all() and (rows[bad, 6:8] == 0).all()
    assert (rows[bad, 8:11].view(np.uint64) == rays[bad, 8:11].astype(np.float64).view(np.uint64)).all()  # sun columns unchanged, NaN included
    near = (1 / 64) * (rays[:, 7].astype(np.float64) - rays[:, 6])
    assert (rows[valid, 6] == near[valid]).all()
    assert rows[9, 7] == rows[9, 6] and rows[10, 7] == rows[10, 6]  # far == near at or above max_alt
    assert rows[0, 7] > rows[0, 6] and rows[11, 7] > rows[11, 6]
    # a call-level sun replaces the planted columns: those rays become valid, and the others do not change
    rows2, valid2, _ = S.sun_rays_np(rays, depth, s["center"], s["scene_range"], s["max_alt"], sun_d=sc["sun"], bias_abs=0.003)
    assert valid2.tolist() == [True, False, False, False] + [True] * 8 and (rows2[valid2, 6] == 0.003).all()


def test_shading_restatement():
    albedo = np.array([[0.5, 1.5, -0.2], [0.25, 0.5, 0.75], [0.3, 0.3, 0.3]], np.float32)
    sky = np.array([[0.2, 0.9, 0.5], [0.5, 0.5, 0.5], [0.1, 0.2, 0.3]], np.float32)
    got = S.shade_np(albedo, sky, np.array([1.0, 0.0, np.nan], np.float32))
    assert got.dtype == np.float32 and (got[0] == [0.5, 1.0, 0.0]).all() and (got[1] == [0.125, 0.25, 0.375]).all() and np.isnan(got[2]).all()


# ---- the C entries ---------------------------------------------------------------------------------------------------------------------
def test_the_two_entries_are_declared_and_bound():
    from satnerf_amd import _lib

    with open(os.path.join(ROOT, "include", "satrender.h")) as f:
        text = f.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, arity in (("sr_sun_rays", 15), ("sr_sun_shade", 9)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, f"{name} is not declared in include/satrender.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        res, argtypes = _lib.SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == n_args == arity, (name, n_args, len(argtypes))
        assert argtypes[-1] is C.c_void_p
    assert "metrics.py:27-33" in text and "rendering.py:102-108" in text  # what the entries replace and correct
    assert os.path.exists(os.path.join(ROOT, "satnerf_amd", "csrc", "sun_rays.hip"))


def _sun_rays_call(**over):
    from satnerf_amd import _lib

    a = dict(ray_stride=11, n=5, range=210.0, max_alt=49.0, sun=(0.3, 0.4, 0.8), bias_abs=0.0, bias_rel=1 / 64, out_stride=11,
             rays=4096, depth=4096, out=4096, valid=4096, center=(1.0, 2.0, 3.0))
    a.update(over)
    ctr = None if a["center"] is None else (C.c_double * 3)(*a["center"])
    sun = None if a["sun"] is None else (C.c_float * 3)(*a["sun"])
    ptr = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731  (fake: never dereferenced, every check comes before the launch)
    _lib.call("sr_sun_rays", ptr(a["rays"]), a["ray_stride"], ptr(a["depth"]), a["n"], None if ctr is None else C.addressof(ctr), a["range"],
              a["max_alt"], sun, a["bias_abs"], a["bias_rel"], ptr(a["out"]), a["out_stride"], ptr(a["valid"]), None, None)


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("over", [dict(ray_stride=10), dict(out_stride=10), dict(range=0.0), dict(range=-1.0), dict(range=NAN), dict(range=INF),
                                  dict(max_alt=NAN), dict(max_alt=INF), dict(bias_abs=-0.1), dict(bias_abs=NAN), dict(bias_rel=-0.1),
                                  dict(bias_rel=INF), dict(sun=(0.0, 0.0, 0.0)), dict(sun=(0.3, 0.4, 0.0)), dict(sun=(0.3, 0.4, -0.5)),
                                  dict(sun=(NAN, 0.4, 0.5)), dict(sun=(0.3, INF, 0.5)), dict(rays=None), dict(depth=None), dict(out=None),
                                  dict(valid=None), dict(center=None), dict(center=(NAN, 0.0, 0.0))])
def test_sun_rays_argument_errors(over):
    from satnerf_amd import _lib

    with pytest.raises(_lib.SatRenderError, match="sr_sun_rays"):
        _sun_rays_call(**over)


def test_empty_calls_launch_nothing():
    from satnerf_amd import _lib

    _sun_rays_call(n=0, rays=None, depth=None, out=None, valid=None)
    _sun_rays_call(n=0, rays=None, depth=None, out=None, valid=None, sun=None)
    _lib.call("sr_sun_shade", None, 3, None, 3, None, 0, None, 3, None)


@pytest.mark.parametrize("over", [dict(albedo_stride=2), dict(sky_stride=2), dict(rgb_stride=0), dict(albedo=None), dict(sky=None), dict(vis=None),
                                  dict(rgb=None)])
def test_sun_shade_argument_errors(over):
    from satnerf_amd import _lib

    a = dict(albedo=4096, albedo_stride=3, sky=4096, sky_stride=13, vis=4096, n=7, rgb=4096, rgb_stride=3)
    a.update(over)
    ptr = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731
    with pytest.raises(_lib.SatRenderError, match="sr_sun_shade"):
        _lib.call("sr_sun_shade", ptr(a["albedo"]), a["albedo_stride"], ptr(a["sky"]), a["sky_stride"], ptr(a["vis"]), a["n"], ptr(a["rgb"]),
                  a["rgb_stride"], None)


# ---- the Python layer without a GPU ----------------------------------------------------------------------------------------------------
def test_python_layer_errors():
    from satnerf_amd import data, dsm, evaluate, ops, rendering
    from satnerf_amd.models import load_model

    args = O.default_args(mlp_mode="bf16")
    models = {"coarse": load_model(args), "t": torch.nn.Embedding(args.t_embbeding_vocab, args.t_embbeding_tau)}
    rays, ts = O.synthetic_rays(16, seed=1)
    scene = (np.array([1.0, 2.0, 3.0]), 210.0, 49.0)
    with pytest.raises(ValueError, match="nerf"):
        rendering.render_sun_visibility(models, rays, ts, O.default_args(model="nerf"), *scene)
    with pytest.raises(ValueError):
        rendering.render_sun_visibility(models, rays, ts, O.default_args(model="bogus"), *scene)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rendering.render_sun_visibility(models, rays, ts, args, *scene)
    with pytest.raises(ValueError, match="GPU"):
        data.sun_rays(rays, torch.zeros(16), *scene, n_samples=64)
    with pytest.raises(ValueError, match="GPU"):
        ops.sun_rays(rays, torch.zeros(16), *scene)
    with pytest.raises(ValueError, match="GPU"):
        ops.sun_shade(torch.zeros(16, 3), torch.zeros(16, 3), torch.zeros(16))
    sweep = (models, rays, ts, args, 4, 4, np.array([0.0, 0.3, 0.9]), np.array([0.3, 0.4, 0.5]), scene[0], scene[1])
    with pytest.raises(ValueError, match="max_alt"):
        evaluate.sun_interp_shadows(*sweep, shadows="geometry")
    with pytest.raises(ValueError, match="shadows"):
        evaluate.sun_interp_shadows(*sweep, shadows="bogus")
    with pytest.raises(ValueError, match="shadows"):
        dsm.render_ortho_dsm(models, 0, args, scene[0], 210.0, -24.0, 49.0, (0.3, 0.4, 0.8), grid=(0.0, 0.0, 4, 4, 0.5), shadows="bogus")
