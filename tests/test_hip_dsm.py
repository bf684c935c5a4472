"""DSM extraction on the GPU (csrc/dsm.hip through satnerf_amd.dsm): the UTM kernel and the rasteriser against the fp64 numpy
restatements of tests/test_dsm_host.py, determinism, and a known surface end to end."""
import math
import time

import numpy as np
import pytest
import torch

from oracle import satnerf_oracle as O
from tests.helpers import load_golden
from tests.test_dsm_host import rasterize_np, utm_forward_np, utm_inverse_np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INF = float("inf")


def _dsm():
    from satnerf_amd import dsm, ops

    return dsm, ops


def _d(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64).to(DEV)


def bit_equal(a, b):
    """Bitwise equality of two fp32 rasters (torch.equal treats their NaN cells as different)."""
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def ecef_from_geodetic(lat, lon, alt):
    a, e2 = 6378137.0, 6.69437999014e-3
    phi, lam = np.radians(lat), np.radians(lon)
    n = a / np.sqrt(1 - e2 * np.sin(phi) ** 2)
    return np.stack([(n + alt) * np.cos(phi) * np.cos(lam), (n + alt) * np.cos(phi) * np.sin(lam), (n * (1 - e2) + alt) * np.sin(phi)], -1)


def test_utm_kernel_matches_restatement_across_a_zone():
    dsm, _ = _dsm()
    lat, lon = np.meshgrid(np.linspace(-80, 84, 165), np.linspace(-84.5, -77.5, 71))  # zone 17 and half a degree beyond either edge
    lat, lon = lat.ravel(), lon.ravel()
    east, north = dsm.utm_from_latlon(_d(lat), _d(lon), zone=17)
    assert east.dtype == torch.float64 and east.is_cuda
    we, wn = utm_forward_np(lat, lon, 17)
    assert np.abs(east.cpu().numpy() - we).max() <= 1e-6 and np.abs(north.cpu().numpy() - wn).max() <= 1e-6
    assert (north.cpu().numpy()[lat < 0] < 0).all()  # false northing 0 in the south
    # zone from the first point (Cape Town: 34H) and the string form of the override
    e2, n2 = dsm.utm_from_latlon(_d([-33.9, -34.0]), _d([18.4, 18.5]))
    we2, wn2 = utm_forward_np(np.array([-33.9, -34.0]), np.array([18.4, 18.5]), 34)
    assert np.abs(e2.cpu().numpy() - we2).max() <= 1e-6 and np.abs(n2.cpu().numpy() - wn2).max() <= 1e-6
    e3, _ = dsm.utm_from_latlon(_d([-33.9]), _d([18.4]), zone="34H")
    assert torch.equal(e3, e2[:1])


def test_depth_path_equals_latlonalt_from_depth_bitwise():
    dsm, ops = _dsm()
    from satnerf_amd import rendering

    g = load_golden("latlonalt")
    rays, depth, center, rng = g["rays"].to(DEV), g["depth"].to(DEV), np.asarray(g["center"]), float(g["range"])
    lat, lon, alt = rendering.latlonalt_from_depth(rays, depth, center, rng)
    zone = dsm.utm_zone(lat[0].item(), lon[0].item())[0]
    east, north, alt2, zone_out = ops.depth_to_utm(rays, depth, center, rng)
    assert zone_out.cpu().tolist()[0] == zone
    assert torch.equal(alt2, alt)  # the shared geodetic arithmetic, bit for bit
    e_ref, n_ref = ops.utm_from_latlon(lat, lon, zone)
    assert torch.equal(east, e_ref) and torch.equal(north, n_ref)
    # the golden check of the existing kernel still holds
    assert np.abs(lat.cpu().numpy() - np.asarray(g["lats"])).max() < 1e-11


def _check_raster(east, north, alt, grid, radius, sigma):
    _, ops = _dsm()
    xoff, yoff, res, xsize, ysize = grid
    got, w = ops.dsm_rasterize(_d(east), _d(north), _d(alt), xoff, yoff, res, xsize, ysize, radius, sigma)
    want, ww = rasterize_np(east, north, alt, xoff, yoff, res, xsize, ysize, radius, sigma)
    got, w = got.cpu().numpy().astype(np.float64), w.cpu().numpy().astype(np.float64)
    assert (np.isnan(got) == np.isnan(want)).all()
    ok = ~np.isnan(want)
    # 1e-6 m before the fp32 store, plus that store's half ulp
    tol = (1e-6 if math.isinf(sigma) else 1e-4) + np.abs(want[ok]) * 2.0**-24
    assert (np.abs(got[ok] - want[ok]) <= tol).all(), np.abs(got[ok] - want[ok]).max()
    assert np.allclose(w, ww, rtol=2e-7, atol=1e-9)
    return got


@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("sigma", [INF, 1.5])
def test_rasterizer_matches_restatement(radius, sigma):
    rng = np.random.default_rng(100 + radius)
    xoff, yoff, res, xsize, ysize = 435000.0, 3354000.0, 0.5, 40, 30
    n = 3000
    # random cloud over a region a bit larger than the grid (points outside contribute nothing)
    east = xoff + rng.uniform(-3, xsize * res + 3, n)
    north = yoff - rng.uniform(-3, ysize * res + 3, n)
    alt = rng.uniform(-5, 50, n)
    # points exactly on cell edges and corners, on the grid's own edges, and non-finite ones
    k = rng.integers(0, 30, 200)
    east[:200] = xoff + k * res
    north[:200] = yoff - rng.integers(0, 30, 200) * res
    east[200:210] = xoff + xsize * res  # east edge: outside
    north[210:220] = yoff - ysize * res  # south edge: outside
    north[220:230] = yoff  # north edge: inside, row 0
    alt[230], east[231], north[232] = np.nan, np.inf, -np.inf
    _check_raster(east, north, alt, (xoff, yoff, res, xsize, ysize), radius, sigma)


@pytest.mark.parametrize("sigma", [INF, 1.5])
def test_rasterizer_is_deterministic_and_order_independent(sigma):
    _, ops = _dsm()
    rng = np.random.default_rng(7)
    n = 200000  # ~170 points per cell: heavy contention on every accumulator
    east, north, alt = rng.uniform(0, 17, n), rng.uniform(-17, 0, n), rng.uniform(0, 100, n)
    args = (0.0, 0.0, 0.5, 34, 34, 2, sigma)
    a = ops.dsm_rasterize(_d(east), _d(north), _d(alt), *args)
    b = ops.dsm_rasterize(_d(east), _d(north), _d(alt), *args)
    p = rng.permutation(n)
    c = ops.dsm_rasterize(_d(east[p]), _d(north[p]), _d(alt[p]), *args)
    for x, y in ((a, b), (a, c)):
        assert bit_equal(x[0], y[0]) and bit_equal(x[1], y[1])


def _scene(n_side=32, res=0.5, lat0=30.3, lon0=-81.7, seed=3):
    """Rays whose depth hits a known height field at the centres of an n_side^2 ROI grid near (lat0, lon0): one point per cell."""
    zone = 17
    e0, n0 = utm_forward_np(lat0, lon0, zone)
    x, y = math.floor(float(e0)), math.floor(float(n0))
    roi = np.array([x, y, n_side, res])  # {aoi}_DSM.txt: lower-left corner, size, resolution
    yoff = y + n_side * res
    jj, cc = np.meshgrid(np.arange(n_side), np.arange(n_side), indexing="ij")
    e_c, n_c = x + (cc + 0.5) * res, yoff - (jj + 0.5) * res
    heights = 12.0 + 4.0 * np.sin(cc / 5.0) * np.cos(jj / 7.0) + np.random.default_rng(seed).uniform(-0.5, 0.5, jj.shape)
    lat, lon = utm_inverse_np(e_c.ravel(), n_c.ravel(), zone)
    target = ecef_from_geodetic(lat, lon, heights.ravel())
    center = ecef_from_geodetic(np.array(lat0), np.array(lon0), np.array(0.0))
    scene_range = 600.0
    up = target / np.linalg.norm(target, axis=1, keepdims=True)
    origin = target + 500.0 * up + np.array([40.0, -25.0, 10.0])  # an off-nadir view
    d = target - origin
    depth = np.linalg.norm(d, axis=1) / scene_range
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((len(depth), 11), np.float32)
    rays[:, 0:3], rays[:, 3:6] = (origin - center) / scene_range, d
    rays[:, 7] = 2.0
    return torch.from_numpy(rays).to(DEV), torch.from_numpy(depth.astype(np.float32)).to(DEV), center, scene_range, roi, heights


def test_known_surface_end_to_end():
    dsm, _ = _dsm()
    rays, depth, center, scene_range, roi, heights = _scene()
    out = dsm.dsm_from_depth(rays, depth, center, scene_range, roi=roi, radius=0)
    assert out.zone == "17R" and out.dsm.shape == heights.shape and out.dsm.dtype == torch.float32
    assert out.transform == (0.5, 0.0, float(roi[0]), 0.0, -0.5, float(roi[1] + roi[2] * roi[3]))
    got = out.dsm.cpu().numpy()
    assert np.abs(got - heights).max() <= 1e-3, np.abs(got - heights).max()
    assert (out.weight.cpu().numpy() == 1).all()
    # same cloud through the auto grid: it covers the cloud, the ROI grid's cells sit inside it
    auto = dsm.dsm_from_depth(rays, depth.view(-1, 1), center, scene_range, resolution=0.5, radius=0)
    assert auto.xoff <= roi[0] and auto.yoff >= roi[1] + roi[2] * roi[3] - 0.5
    assert int(torch.isfinite(auto.dsm).sum()) == heights.size
    # Z registration: a constant offset is recovered, water (class 9) is excluded
    truth = torch.from_numpy(heights).to(DEV)
    mask = torch.zeros(heights.shape, dtype=torch.uint8, device=DEV)
    mask[:4, :] = 9
    truth_w = truth.clone()
    truth_w[:4, :] += 100.0  # would drag the shift if water were kept
    mae, err, rdsm, shift = dsm.dsm_mae(out.dsm + 0.37, truth_w, mask)
    assert mae <= 1e-3 and abs(shift + 0.37) <= 1e-3
    assert torch.isnan(err[:4]).all() and torch.isfinite(err[4:]).all() and rdsm.dtype == torch.float64
    mae2, _, _, _ = dsm.dsm_mae(out, truth)
    assert mae2 <= 1e-3
    with pytest.raises(ValueError):
        dsm.dsm_mae(auto, truth)  # not on the ROI grid
    with pytest.raises(ValueError):
        dsm.dsm_mae(out.dsm[:-1], truth)
    # zone override: same zone, same raster
    again = dsm.dsm_from_depth(rays, depth, center, scene_range, roi=roi, radius=0, zone=17)
    assert bit_equal(again.dsm, out.dsm) and again.zone == "17R"


def test_render_dsm_equals_dsm_from_depth_of_render_image_outputs():
    dsm, _ = _dsm()
    from satnerf_amd import rendering
    from satnerf_amd.models import load_model

    args = O.default_args(n_samples=64, mlp_mode="bf16x3")
    m = load_model(args)
    m.load_state_dict(O.procedural_satnerf_params(args.fc_units, args.t_embbeding_tau, seed=1))
    emb = torch.nn.Embedding(args.t_embbeding_vocab, args.t_embbeding_tau)
    emb.load_state_dict({"weight": O.procedural_uniform((args.t_embbeding_vocab, args.t_embbeding_tau), 1.0, 7)})
    models = {"coarse": m.to(DEV).eval(), "t": emb.to(DEV)}
    rays, ts = O.synthetic_rays(500, seed=31)
    rays, ts = rays.to(DEV), ts.to(DEV)
    center = ecef_from_geodetic(np.array(30.3), np.array(-81.7), np.array(0.0))
    g = torch.Generator().manual_seed(32)
    draws = [torch.rand(500, 64, generator=g).to(DEV), torch.randn(500, 64, generator=g).to(DEV)]
    with rendering.replay_rng(draws):
        got = dsm.render_dsm(models, rays, ts, args, center, 300.0, resolution=2.0)
    with torch.no_grad(), rendering.replay_rng(draws):
        depth = rendering.render_image_outputs(models, rays, ts, args)["depth"]
    want = dsm.dsm_from_depth(rays, depth, center, 300.0, resolution=2.0)
    assert bit_equal(got.dsm, want.dsm) and bit_equal(got.weight, want.weight)
    assert (got.xoff, got.yoff, got.zone) == (want.xoff, want.yoff, want.zone) and got.zone.startswith("17")
    assert int(torch.isfinite(got.dsm).sum()) > 0


def test_bounds_of_a_full_wave_plus_one_lane():
    """n = 65: the 65th point sits alone in the second wave, whose other lanes carry the neutral keys through the shuffles.  It holds
    the smallest easting; the largest easting belongs to a point whose altitude is NaN and must not count.  Exact against numpy."""
    _, ops = _dsm()
    g = np.random.default_rng(3)
    east, north, alt = g.uniform(-5e5, 5e5, 65), g.uniform(-3e6, 3e6, 65), g.uniform(-50.0, 50.0, 65)
    east[64], east[17], alt[17] = -6e5, 7e5, np.nan
    north[40] = -0.0
    ok = np.isfinite(alt)
    got = ops.dsm_bounds(_d(east), _d(north), _d(alt)).cpu().numpy()
    want = np.array([east[ok].min(), east[ok].max(), north[ok].min(), north[ok].max()])
    assert ok.sum() == 64 and want[0] == -6e5 and want[1] < 7e5
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), (got, want)


def test_edge_cases():
    dsm, _ = _dsm()
    rays, depth, center, scene_range, roi, heights = _scene(n_side=8)
    # zero rays: an all-NaN ROI raster; without a roi the grid cannot be sized
    z = dsm.dsm_from_depth(rays[:0], depth[:0], center, scene_range, roi=roi)
    assert z.dsm.shape == (8, 8) and torch.isnan(z.dsm).all() and (z.weight == 0).all()
    with pytest.raises(ValueError):
        dsm.dsm_from_depth(rays[:0], depth[:0], center, scene_range)
    # every point outside the ROI
    far = np.array(roi, dtype=np.float64)
    far[0] += 1000.0
    o = dsm.dsm_from_depth(rays, depth, center, scene_range, roi=far)
    assert torch.isnan(o.dsm).all() and o.zone == "17R"
    # CPU inputs, bad radius / sigma, zero-size roi
    with pytest.raises(ValueError):
        dsm.dsm_from_depth(rays.cpu(), depth.cpu(), center, scene_range, roi=roi)
    with pytest.raises(ValueError):
        dsm.utm_from_latlon(torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError):
        dsm.dsm_mae(torch.zeros(4, 4), torch.zeros(4, 4))
    with pytest.raises(ValueError):
        dsm.dsm_from_depth(rays, depth, center, scene_range, roi=roi, radius=5)
    with pytest.raises(ValueError):
        dsm.dsm_from_depth(rays, depth, center, scene_range, roi=roi, sigma=0.0)
    with pytest.raises(ValueError):
        dsm.dsm_from_depth(rays, depth, center, scene_range, roi=[roi[0], roi[1], 0, 0.5])
    with pytest.raises(ValueError):
        dsm.dsm_from_depth(rays, depth[:-1], center, scene_range, roi=roi)
    # a first ray whose depth is NaN: no zone to take, unless given
    bad = depth.clone()
    bad[0] = float("nan")
    with pytest.raises(ValueError):
        dsm.dsm_from_depth(rays, bad, center, scene_range, roi=roi)
    ok = dsm.dsm_from_depth(rays, bad, center, scene_range, roi=roi, zone=17, radius=0)
    assert int(torch.isnan(ok.dsm).sum()) == 1 and ok.zone == "17"


def test_full_image_512x512_matches_restatement():
    _, ops = _dsm()
    rng = np.random.default_rng(12)
    n = 512 * 512
    east = 435000.0 + rng.uniform(0, 256, n)
    north = 3354000.0 - rng.uniform(0, 256, n)
    alt = 10.0 + rng.normal(0, 3, n)
    grid = (435000.0, 3354000.0, 0.5, 512, 512)
    ed, nd, ad = _d(east), _d(north), _d(alt)
    ops.dsm_rasterize(ed, nd, ad, *grid, 1, INF)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.dsm_rasterize(ed, nd, ad, *grid, 1, INF)
    torch.cuda.synchronize()
    print(f"dsm_rasterize 512x512 points, radius 1: {(time.perf_counter() - t0) * 1e3:.3f} ms (wall, after a warm-up)")
    _check_raster(east, north, alt, grid, 1, INF)
