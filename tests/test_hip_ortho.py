"""Nadir DSM on the GPU (csrc/ortho.hip through satnerf_amd.dsm / data): the inverse UTM kernel and the vertical rays against the fp64
restatement of tests/ortho_reference.py, their consistency with the existing depth -> UTM kernel, the depth -> DSM step on a known
height field, and render_ortho_dsm end to end on a random-initialised field."""
import functools

import numpy as np
import pytest
import torch

from oracle import satnerf_oracle as O
from tests import ortho_reference as R
from tests.test_dsm_host import central_meridian, utm_forward_np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCENES = {"jax": R.jax, "cape_town": R.cape_town}


def _mods():
    from satnerf_amd import data, dsm, ops

    return data, dsm, ops


def _d(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64).to(DEV)


@functools.lru_cache(maxsize=None)
def _reference(name, xsize, ysize):
    """(scene, restated fp64 rays, restated latlon): computed once per grid and shared, never written to."""
    s = SCENES[name](xsize, ysize)
    rays, latlon = R.ortho_rays_np(**s)
    rays.setflags(write=False), latlon.setflags(write=False)
    return s, rays, latlon


# ---- sr_utm_to_latlon -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 257, 4096])  # 257: the one-lane tail of a second 256-thread block
@pytest.mark.parametrize("zone,south", [(17, False), (34, True)])
def test_utm_to_latlon_matches_restatement_and_round_trips(n, zone, south):
    _, dsm, ops = _mods()
    rng = np.random.default_rng(1000 + n + zone)
    lat = rng.uniform(-60, 0, n) if south else rng.uniform(0, 60, n)
    east, north = utm_forward_np(lat, central_meridian(zone) + rng.uniform(-3.5, 3.5, n), zone)
    lons, lats = dsm.lonlat_from_utm(_d(east), _d(north), zone)  # the reference's return order
    assert lons.dtype == lats.dtype == torch.float64 and lons.is_cuda and lons.shape == (n,)
    if n == 0:
        return
    want_lat, want_lon = R.utm_inverse_np(east, north, zone)
    err = max(np.abs(lats.cpu().numpy() - want_lat).max(), np.abs(lons.cpu().numpy() - want_lon).max())
    e2, n2 = ops.utm_from_latlon(lats, lons, zone)
    trip = max(np.abs(e2.cpu().numpy() - east).max(), np.abs(n2.cpu().numpy() - north).max())
    print(f"n {n} zone {zone}: {err:.2e} deg against the restatement, round trip {trip:.2e} m")
    assert err <= 1e-11 and trip <= 1e-6
    assert not south or (north < 0).all()


def test_utm_to_latlon_nan_in_nan_out():
    _, dsm, _ = _mods()
    east, north = utm_forward_np(np.linspace(29, 31, 300), np.linspace(-83, -80, 300), 17)
    bad_e, bad_n = east.copy(), north.copy()
    bad_e[5], bad_n[64], bad_e[299], bad_n[130] = np.nan, np.nan, np.inf, -np.inf
    lons, lats = (t.cpu().numpy() for t in dsm.lonlat_from_utm(_d(bad_e), _d(bad_n), "17R"))
    bad = np.zeros(300, bool)
    bad[[5, 64, 299, 130]] = True
    assert np.isnan(lons[bad]).all() and np.isnan(lats[bad]).all()
    want_lat, want_lon = R.utm_inverse_np(east, north, 17)
    assert np.abs(lats[~bad] - want_lat[~bad]).max() <= 1e-11 and np.abs(lons[~bad] - want_lon[~bad]).max() <= 1e-11


# ---- sr_ortho_rays ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xsize,ysize", [(1, 1), (37, 53), (300, 5)])
@pytest.mark.parametrize("name", ["jax", "cape_town"])
def test_ortho_rays_match_restatement(name, xsize, ysize):
    data, _, _ = _mods()
    s, want, want_ll = _reference(name, xsize, ysize)
    n = xsize * ysize
    rays, latlon = data.ortho_rays(device=DEV, return_latlon=True, **s)
    assert rays.shape == (n, 11) and rays.dtype == torch.float32 and latlon.shape == (n, 2) and latlon.dtype == torch.float64
    got = rays.cpu().numpy()
    ok = R.within_one_ulp(got, want)
    assert ok.all(), (np.argwhere(~ok)[:5], got[~ok][:5], want[~ok][:5])
    sun32 = np.asarray(s["sun_d"], np.float32)
    assert (got[:, 8:11].view(np.uint32) == sun32.view(np.uint32)).all()
    assert (got[:, 6].view(np.uint32) == 0).all()  # exactly +0
    assert (got[:, 7] == np.float32((s["max_alt"] - s["min_alt"]) / s["scene_range"])).all()
    err = np.abs(latlon.cpu().numpy() - want_ll).max()
    print(f"{name} {ysize} x {xsize}: latlon {err:.2e} deg")
    assert err <= 1e-11
    # a 13-column buffer (the image buffer's width): columns 11:13 keep their sentinel, the rest is the same bytes as before
    buf = torch.full((n, 13), -7.25, dtype=torch.float32, device=DEV)
    view = data.ortho_rays(device=DEV, out=buf, **s)
    assert view.shape == (n, 11) and view.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:, :11].view(torch.int32), rays.view(torch.int32)) and (buf[:, 11:] == -7.25).all()
    again = data.ortho_rays(device=DEV, **s)
    assert torch.equal(again.view(torch.int32), rays.view(torch.int32))


@pytest.mark.parametrize("name", ["jax", "cape_town"])
def test_points_along_the_rays_stay_in_their_cell(name):
    """Consistency with the depth -> UTM kernel: whatever depth a render returns, the point lies over its own cell at the closed-form
    altitude."""
    data, _, ops = _mods()
    s, want, _ = _reference(name, 37, 53)
    xoff, yoff, xsize, ysize, r = s["grid"]
    rays = data.ortho_rays(device=DEV, **s)
    far = float(np.float32((s["max_alt"] - s["min_alt"]) / s["scene_range"]))
    depth = torch.from_numpy(np.random.default_rng(4).uniform(0, far, xsize * ysize).astype(np.float32)).to(DEV)
    east, north, alt, _ = ops.depth_to_utm(rays, depth, s["center"], s["scene_range"], s["zone"])
    east, north, alt = east.cpu().numpy(), north.cpu().numpy(), alt.cpu().numpy()
    jj, cc = np.meshgrid(np.arange(ysize), np.arange(xsize), indexing="ij")
    assert (np.floor((east - xoff) / r) == cc.ravel()).all() and (np.floor((yoff - north) / r) == jj.ravel()).all()
    closed = s["max_alt"] - depth.cpu().numpy().astype(np.float64) * s["scene_range"]
    print(f"{name}: altitude against the closed form {np.abs(alt - closed).max():.2e} m")
    assert np.abs(alt - closed).max() <= 1e-3


# ---- ortho_dsm_from_depth ---------------------------------------------------------------------------------------------------------
def test_ortho_dsm_from_depth_recovers_a_height_field():
    _, dsm, _ = _mods()
    s = R.jax(40, 40)
    xoff, yoff, xsize, ysize, r = s["grid"]
    roi = np.array([xoff, yoff - ysize * r, float(xsize), r])  # the {aoi}_DSM.txt this grid comes from
    assert dsm.grid_from_roi(roi) == s["grid"]
    east, north = R.cell_centres(s["grid"])
    h = 12.0 + 9.0 * np.sin((east - xoff) / 5.0) * np.cos((yoff - north) / 3.0) - 20.0 * ((east - xoff) / (xsize * r)) ** 2
    assert h.min() >= s["min_alt"] and h.max() <= s["max_alt"]
    depth = ((s["max_alt"] - h) / s["scene_range"]).astype(np.float32)
    holes = np.zeros(h.shape, bool)
    holes[0, 0], holes[17, 3], holes[39, 39], holes[5, 22] = True, True, True, True
    depth[holes] = [np.nan, np.inf, -np.inf, np.nan]
    out = dsm.ortho_dsm_from_depth(torch.from_numpy(depth.ravel()).to(DEV), s["grid"], s["max_alt"], s["scene_range"], zone="17R", roi=roi)
    assert out.dsm.shape == (ysize, xsize) and out.dsm.dtype == torch.float32 and out.zone == "17R" and out.roi == tuple(roi)
    assert (out.xoff, out.yoff, out.resolution) == (xoff, yoff, r)
    got = out.dsm.cpu().numpy()
    assert (np.isnan(got) == holes).all()
    assert (out.weight.cpu().numpy() == np.where(holes, 0.0, 1.0)).all()
    # two fp32 roundings: the depth (relative 2^-24 of at most max_alt - min_alt) and the stored altitude (2^-24 of |h|)
    bound = 2.0**-24 * ((s["max_alt"] - s["min_alt"]) + np.abs(h).max()) * 1.01
    err = np.abs(got[~holes] - h[~holes]).max()
    mae, _, _, shift = dsm.dsm_mae(out, _d(h), register="z")
    print(f"raster error {err:.2e} m, MAE {mae:.2e} m, shift {shift:.2e} m (bound {bound:.2e} m)")
    assert err <= bound and mae <= bound


# ---- render_ortho_dsm -------------------------------------------------------------------------------------------------------------
def test_render_ortho_dsm_equals_its_three_steps():
    data, dsm, _ = _mods()
    from satnerf_amd import rendering
    from satnerf_amd.models import load_model

    args = O.default_args(n_samples=64, fc_units=256)
    torch.manual_seed(11)
    models = {"coarse": load_model(args).to(DEV).eval(), "t": torch.nn.Embedding(args.t_embbeding_vocab, args.t_embbeding_tau).to(DEV)}
    s = R.jax(24, 40)
    xsize, ysize = s["grid"][2], s["grid"][3]
    n = xsize * ysize
    common = (s["center"], s["scene_range"], s["min_alt"], s["max_alt"], s["sun_d"])
    torch.manual_seed(0)
    got, outputs = dsm.render_ortho_dsm(models, 3, args, *common, grid=s["grid"], zone=17)
    torch.manual_seed(0)
    rays = data.ortho_rays(device=DEV, **s)
    with torch.no_grad():
        by_hand = rendering.render_image_outputs(models, rays, torch.full((n,), 3, dtype=torch.int64, device=DEV), args)
    want = dsm.ortho_dsm_from_depth(by_hand["depth"], s["grid"], s["max_alt"], s["scene_range"], zone="17")
    assert torch.equal(got.dsm.view(torch.int32), want.dsm.view(torch.int32)) and torch.equal(got.weight, want.weight)
    for k in ("rgb", "depth", "albedo", "sun", "beta"):
        assert torch.equal(outputs[k], by_hand[k]), k
    raster = got.dsm.cpu().numpy()
    assert raster.shape == (ysize, xsize) and np.isfinite(raster).all()
    assert raster.min() >= s["min_alt"] and raster.max() <= s["max_alt"]
    assert outputs["rgb"].shape == (n, 3) and outputs["rgb"].view(ysize, xsize, 3).shape == (ysize, xsize, 3)
    # zone=None: the zone of the scene centre, and ts as a tensor
    torch.manual_seed(0)
    auto, _ = dsm.render_ortho_dsm(models, torch.full((n,), 3, dtype=torch.int64), args, *common, grid=s["grid"])
    assert auto.zone == "17R" and torch.equal(auto.dsm.view(torch.int32), got.dsm.view(torch.int32))
