"""Cloud fusion on the GPU (csrc/cloud_grid.hip through satnerf_amd.ops / satnerf_amd.dsm): the reference's
recorded rasters, order independence, the scan's and the segment sort's boundaries against the numpy restatement of
tests/cloud_grid_reference.py, the stated departures, and the multi-view flow.

The sizes the kernels switch on (csrc/cloud_grid.hip): SCAN_BLOCK cells per scan workgroup, CARRY_CHUNK block sums per step of the
one-workgroup carry scan, segments up to WAVE_CAP keys sorted by one wave, up to CHUNK keys by one workgroup in LDS, longer ones in
CHUNK-sized pieces with the wide strides in global memory (strides >= CHUNK first appear above 2 CHUNK keys)."""
import math

import numpy as np
import pytest
import torch

from oracle import satnerf_oracle as O
from tests import cloud_grid_reference as R
from tests.test_dsm_host import utm_forward_np, utm_inverse_np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCAN_BLOCK, CARRY_CHUNK, WAVE_CAP, CHUNK = 1024, 256, 64, 4096


def _mods():
    from satnerf_amd import dsm, ops

    return dsm, ops


def _d(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def bit_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _against_restatement(east, north, alt, x0, y0, d, map_w, map_h, rule):
    """All four modes and the count of one cloud against the restatement: min / max / med bit for bit, avg within
    (2 n + 2) 2^-53 max|z| per cell."""
    _, ops = _mods()
    args = (x0, y0, d, map_w, map_h)
    bound = R.avg_bound_np(east, north, alt, *args, rule)
    for mode in R.MODES:
        got, count = ops.cloud_grid(_d(east), _d(north), _d(alt), *args, rule=rule, mode=mode)
        want, wcount = R.cloud_grid_np(east, north, alt, *args, rule, mode)
        got, count = got.cpu().numpy(), count.cpu().numpy()
        assert count.dtype == np.int32 and (count == wcount).all(), mode
        if mode == "avg":
            assert (np.isnan(got) == np.isnan(want)).all()
            ok = ~np.isnan(want)
            err = np.abs(got[ok] - want[ok])
            assert (err <= bound[ok]).all(), err.max()
        else:
            assert R.same_bits(got, want), mode


@pytest.mark.parametrize("name", R.FIXTURES)
def test_reference_fixtures(name):
    dsm, ops = _mods()
    g = R.load(name)
    xyz, bb, d = g["xyz"], g["bb"], float(g["definition"])
    map_w, map_h = R.map_size(bb, d)
    args = (xyz[:, 0], xyz[:, 1], xyz[:, 2], bb[0], bb[2], d, map_w, map_h, "nearest")
    bound = R.avg_bound_np(*args)
    cloud = _d(xyz)
    for mode in R.MODES:
        got = dsm.project_cloud_into_utm_grid(cloud, bb.tolist(), d, mode)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == g[mode].shape
        got = got.cpu().numpy()
        if mode == "avg":
            assert (np.isnan(got) == np.isnan(g["avg"])).all()
            ok = ~np.isnan(got)
            err = np.abs(got[ok] - g["avg"][ok])
            print(f"{name} avg: max |ours - ref| = {err.max():.3g}, smallest bound = {bound[ok].min():.3g}")
            assert (err <= bound[ok]).all(), err.max()
        else:
            assert R.same_bits(got, g[mode]), mode
    _, count = ops.cloud_grid(_d(xyz[:, 0]), _d(xyz[:, 1]), _d(xyz[:, 2]), bb[0], bb[2], d, map_w, map_h, rule="nearest", mode="med")
    assert (count.cpu().numpy() == R.cloud_grid_np(*args, "med")[1]).all()
    # a packed cloud with extra columns is split by the wrapper; the mask argument changes nothing
    wide = torch.cat([cloud, torch.ones(len(xyz), 2, dtype=torch.float64, device=DEV)], 1)
    assert bit_equal(dsm.project_cloud_into_utm_grid(wide, bb.tolist(), d, "med", mask=torch.ones(map_h, map_w, device=DEV)), _d(g["med"]))


def test_order_independence_and_dirty_scratch():
    _, ops = _mods()
    rng = np.random.default_rng(7)
    n = 200000  # ~170 points per cell on 34 x 34: every segment goes through the workgroup sort
    east, north, alt = rng.uniform(0, 17, n), rng.uniform(-17, 0, n), rng.uniform(0, 100, n)
    grid = (0.0, -17.0, 0.5, 34, 34)
    p = rng.permutation(n)
    e, nn, a = _d(east), _d(north), _d(alt)
    ep, np_, ap = _d(east[p]), _d(north[p]), _d(alt[p])
    nbytes = ops.cloud_grid_scratch(n, 34, 34)
    for mode in R.MODES:
        first = ops.cloud_grid(e, nn, a, *grid, mode=mode)
        perm = ops.cloud_grid(ep, np_, ap, *grid, mode=mode)
        scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
        out = torch.full((34, 34), -7.25, dtype=torch.float64, device=DEV)
        count = torch.full((34, 34), 12345, dtype=torch.int32, device=DEV)
        dirty = ops.cloud_grid(e, nn, a, *grid, mode=mode, scratch=scratch, out=out, count=count)
        for other in (perm, dirty):
            assert bit_equal(first[0], other[0]) and bit_equal(first[1], other[1]), mode
        assert int(first[1].sum()) > 0.9 * n
    _against_restatement(east, north, alt, *grid, "nearest")


def test_scan_block_boundaries():
    rng = np.random.default_rng(11)
    for side in (300, 600):  # 90 000 cells = 88 scan blocks; 360 000 cells = 352 block sums = two steps of the carry scan
        cells = side * side
        edges = np.arange(SCAN_BLOCK, cells, SCAN_BLOCK) if side == 300 else np.array([SCAN_BLOCK, CARRY_CHUNK * SCAN_BLOCK])
        target = np.unique(np.concatenate([[0, cells - 1], edges - 1, edges]))
        target = np.repeat(target, rng.integers(1, 4, len(target)))  # 1..3 points in each
        row, col = target // side, target % side
        # rule "floor" on a unit grid: output row = row, so `target` is the flat output cell
        east, north = col + rng.uniform(0.1, 0.9, len(target)), -(row + rng.uniform(0.1, 0.9, len(target)))
        alt = rng.normal(0, 30, len(target))
        _, ops = _mods()
        _, count = ops.cloud_grid(_d(east), _d(north), _d(alt), 0.0, 0.0, 1.0, side, side, rule="floor", mode="med")
        assert (np.flatnonzero(count.cpu().numpy().ravel()) == np.unique(target)).all()
        _against_restatement(east, north, alt, 0.0, 0.0, 1.0, side, side, "floor")


def test_segment_length_boundaries():
    rng = np.random.default_rng(13)
    # one cell per length: either side of the wave cap, of 256 (one key per thread), of the LDS chunk, and of 2 CHUNK (global strides)
    lengths = [WAVE_CAP - 1, WAVE_CAP, WAVE_CAP + 1, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1, 2, 3]
    east = np.concatenate([np.full(c, float(k)) for k, c in enumerate(lengths)])
    north = np.zeros(len(east))
    alt = rng.normal(10, 40, len(east))
    alt[rng.integers(0, len(alt), 500)] = 3.5  # duplicates
    p = rng.permutation(len(east))
    _against_restatement(east[p], north[p], alt[p], 0.0, 0.0, 1.0, len(lengths), 1, "nearest")


def test_one_cell_grid_and_tiny_clouds():
    _, ops = _mods()
    rng = np.random.default_rng(17)
    n = 5000
    east, north, alt = rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n), rng.normal(0, 100, n)
    _against_restatement(east, north, alt, 0.0, 0.0, 1.0, 1, 1, "nearest")
    # N = 0: an all-NaN raster and zero counts; N = 1
    empty = torch.empty(0, dtype=torch.float64, device=DEV)
    for mode in R.MODES:
        out, count = ops.cloud_grid(empty, empty, empty, 0.0, 0.0, 0.5, 7, 5, mode=mode)
        assert out.shape == (5, 7) and torch.isnan(out).all() and (count == 0).all()
    dsm, _ = _mods()
    out = dsm.project_cloud_into_utm_grid(torch.empty(0, 3, device=DEV), [0.0, 3.0, 0.0, 2.0], 0.5, "med")
    assert out.shape == (5, 7) and torch.isnan(out).all()
    _against_restatement(np.array([1.0]), np.array([0.5]), np.array([-4.0]), 0.0, 0.0, 0.5, 7, 5, "nearest")


def test_departures_non_finite_points_and_floor_edges():
    _, ops = _mods()
    rng = np.random.default_rng(19)
    n = 2000
    east, north, alt = rng.uniform(0, 10, n), rng.uniform(0, 8, n), rng.uniform(-5, 50, n)
    grid = (0.0, 0.0, 0.5, 21, 17)
    bad_e, bad_n, bad_a = [], [], []
    for v in (np.nan, np.inf, -np.inf):  # each of the three coordinates in turn, the other two well inside the grid
        bad_e += [v, 3.0, 3.0]
        bad_n += [4.0, v, 4.0]
        bad_a += [1e6, 1e6, v]
    e2, n2, a2 = np.concatenate([east, bad_e]), np.concatenate([north, bad_n]), np.concatenate([alt, bad_a])
    p = rng.permutation(len(e2))
    for rule, g in (("nearest", grid), ("floor", (0.0, 8.0, 0.5, 21, 17))):
        for mode in R.MODES:
            clean = ops.cloud_grid(_d(east), _d(north), _d(alt), *g, rule=rule, mode=mode)
            dirty = ops.cloud_grid(_d(e2[p]), _d(n2[p]), _d(a2[p]), *g, rule=rule, mode=mode)
            assert bit_equal(clean[0], dirty[0]) and bit_equal(clean[1], dirty[1]), (rule, mode)
    # floor: a point at exactly xoff + k r sits in column k, one at exactly yoff - j r in row j
    xoff, yoff, r, w, h = 435000.0, 3354000.0, 0.5, 12, 9
    k, j = np.arange(w), np.arange(h)
    east = np.concatenate([xoff + k * r, np.full(h, xoff + 0.1)])
    north = np.concatenate([np.full(w, yoff - 0.1), yoff - j * r])
    alt = np.arange(len(east), dtype=np.float64)
    out, count = ops.cloud_grid(_d(east), _d(north), _d(alt), xoff, yoff, r, w, h, rule="floor", mode="max")
    count = count.cpu().numpy()
    assert (count[0, 1:] == 1).all() and (count[1:, 0] == 1).all() and count[0, 0] == 2 and count.sum() == w + h
    assert (out[0, 1:].cpu().numpy() == np.arange(1, w)).all() and (out[1:, 0].cpu().numpy() == w + np.arange(1, h)).all()
    _against_restatement(east, north, alt, xoff, yoff, r, w, h, "floor")
    with pytest.raises(ValueError):
        ops.cloud_grid(_d(east), _d(north), _d(alt), xoff, yoff, r, w, h, rule="round")
    with pytest.raises(ValueError):
        ops.cloud_grid(_d(east), _d(north), _d(alt), xoff, yoff, r, w, h, mode="mean")
    with pytest.raises(ValueError):
        ops.cloud_grid(_d(east), _d(north), _d(alt), xoff, yoff, r, w, h, scratch=torch.empty(8, dtype=torch.uint8, device=DEV))


# ---- the multi-view flow ---------------------------------------------------------------------------------------------------------
def ecef_from_geodetic(lat, lon, alt):
    a, e2 = 6378137.0, 6.69437999014e-3
    phi, lam = np.radians(lat), np.radians(lon)
    n = a / np.sqrt(1 - e2 * np.sin(phi) ** 2)
    return np.stack([(n + alt) * np.cos(phi) * np.cos(lam), (n + alt) * np.cos(phi) * np.sin(lam), (n * (1 - e2) + alt) * np.sin(phi)], -1)


LAT0, LON0, RANGE = 30.3, -81.7, 600.0


def _view(offset, n_side=16, res=0.5, seed=3):
    """n_side^2 rays of one off-nadir view whose depth hits a known height field at the centres of an n_side^2 grid near
    (LAT0, LON0) (the scene of tests/test_hip_dsm.py): (rays (N, 11), depth (N,), center, roi, heights)."""
    zone = 17
    e0, n0 = utm_forward_np(LAT0, LON0, zone)
    x, y = math.floor(float(e0)), math.floor(float(n0))
    roi = np.array([x, y, n_side, res])
    yoff = y + n_side * res
    jj, cc = np.meshgrid(np.arange(n_side), np.arange(n_side), indexing="ij")
    e_c, n_c = x + (cc + 0.5) * res, yoff - (jj + 0.5) * res
    heights = 12.0 + 4.0 * np.sin(cc / 5.0) * np.cos(jj / 7.0) + np.random.default_rng(seed).uniform(-0.5, 0.5, jj.shape)
    lat, lon = utm_inverse_np(e_c.ravel(), n_c.ravel(), zone)
    target = ecef_from_geodetic(lat, lon, heights.ravel())
    center = ecef_from_geodetic(np.array(LAT0), np.array(LON0), np.array(0.0))
    up = target / np.linalg.norm(target, axis=1, keepdims=True)
    origin = target + 500.0 * up + np.asarray(offset, dtype=np.float64)
    d = target - origin
    depth = np.linalg.norm(d, axis=1) / RANGE
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((len(depth), 11), np.float32)
    rays[:, 0:3], rays[:, 3:6] = (origin - center) / RANGE, d
    rays[:, 7] = 2.0
    rays[:, 8:11] = (0.3, 0.2, 0.93)
    return torch.from_numpy(rays).to(DEV), torch.from_numpy(depth.astype(np.float32)).to(DEV), center, roi, heights


def test_dsm_from_clouds_list_and_roi_grid():
    dsm, ops = _mods()
    views = [_view(off) for off in ((40.0, -25.0, 10.0), (-30.0, 35.0, 5.0), (5.0, 60.0, -20.0))]
    center, roi, heights = views[0][2], views[0][3], views[0][4]
    clouds = [ops.depth_to_utm(rays, depth, center, RANGE, 17)[:3] for rays, depth, *_ in views]
    es, ns, zs = ([c[k] for c in clouds] for k in range(3))
    for mode in R.MODES:
        a = dsm.dsm_from_clouds(es, ns, zs, roi=roi, mode=mode, zone="17R")
        b = dsm.dsm_from_clouds(torch.cat(es), torch.cat(ns), torch.cat(zs), roi=roi, mode=mode, zone="17R")
        c = dsm.dsm_from_clouds(es[::-1], ns[::-1], zs[::-1], roi=roi, mode=mode, zone="17R")
        assert a.dsm.dtype == a.weight.dtype == torch.float32
        for other in (b, c):
            assert bit_equal(a.dsm, other.dsm) and bit_equal(a.weight, other.weight), mode
    # three views of one surface, one point per cell and view: the median is that surface
    med = dsm.dsm_from_clouds(es, ns, zs, roi=roi)
    assert (med.weight.cpu().numpy() == 3).all() and np.abs(med.dsm.cpu().numpy() - heights).max() <= 1e-3
    # the grid is dsm_from_depth's, with and without a roi
    ref = dsm.dsm_from_depth(views[0][0], views[0][1], center, RANGE, roi=roi, radius=0)
    assert (med.xoff, med.yoff, med.resolution, med.transform, med.roi) == (ref.xoff, ref.yoff, ref.resolution, ref.transform, ref.roi)
    assert med.dsm.shape == ref.dsm.shape and med.zone == ""
    auto = dsm.dsm_from_clouds(es[0], ns[0], zs[0], resolution=0.5, mode="max")
    ref_auto = dsm.dsm_from_depth(views[0][0], views[0][1], center, RANGE, resolution=0.5, radius=0)
    assert (auto.xoff, auto.yoff, auto.dsm.shape, auto.transform, auto.roi) == (ref_auto.xoff, ref_auto.yoff, ref_auto.dsm.shape, ref_auto.transform, None)
    both = torch.isfinite(ref_auto.dsm)  # one point per cell: max = the rasteriser's mean of one, up to its 2^-24 m fixed point
    assert (torch.isfinite(auto.dsm) == both).all() and (auto.dsm[both] - ref_auto.dsm[both]).abs().max().item() <= 2e-6
    with pytest.raises(ValueError):
        dsm.dsm_from_clouds(es[0][:0], ns[0][:0], zs[0][:0])
    with pytest.raises(ValueError):
        dsm.dsm_from_clouds(es, ns, zs[:2], roi=roi)
    z = dsm.dsm_from_clouds(es[0][:0], ns[0][:0], zs[0][:0], roi=roi)
    assert torch.isnan(z.dsm).all() and (z.weight == 0).all()


def test_render_fused_dsm_equals_the_hand_composition():
    dsm, ops = _mods()
    from satnerf_amd import rendering
    from satnerf_amd.models import load_model

    args = O.default_args(n_samples=64, mlp_mode="bf16x3")
    m = load_model(args)
    m.load_state_dict(O.procedural_satnerf_params(args.fc_units, args.t_embbeding_tau, seed=1))
    emb = torch.nn.Embedding(args.t_embbeding_vocab, args.t_embbeding_tau)
    emb.load_state_dict({"weight": O.procedural_uniform((args.t_embbeding_vocab, args.t_embbeding_tau), 1.0, 7)})
    models = {"coarse": m.to(DEV).eval(), "t": emb.to(DEV)}
    assert args.fc_units == 256
    built = [_view(off) for off in ((40.0, -25.0, 10.0), (-30.0, 35.0, 5.0))]
    center = built[0][2]
    views = [(rays, torch.full((rays.shape[0],), k, dtype=torch.long, device=DEV)) for k, (rays, *_) in enumerate(built)]

    # by hand: render each view, project with the first view's zone, fuse
    torch.manual_seed(5)
    clouds, zone = [], 0
    with torch.no_grad():
        for rays, ts in views:
            depth = rendering.render_image_outputs(models, rays, ts, args)["depth"]
            e, n, a, zone_out = ops.depth_to_utm(rays, depth, center, RANGE, zone)
            zone = zone or zone_out.cpu().tolist()[0]
            clouds.append((e, n, a))
    assert zone == 17
    es, ns, zs = ([c[k] for c in clouds] for k in range(3))
    auto = dsm.dsm_from_clouds(es, ns, zs, resolution=2.0)
    side = max(auto.dsm.shape)
    roi = [auto.xoff, auto.yoff - side * 2.0, side, 2.0]  # a square {aoi}_DSM.txt grid over the whole fused cloud
    for mode in ("med", "avg"):
        want = dsm.dsm_from_clouds(es, ns, zs, roi=roi, mode=mode, zone="17R")
        torch.manual_seed(5)
        got = dsm.render_fused_dsm(models, views, args, center, RANGE, mode=mode, roi=roi)
        assert bit_equal(got.dsm, want.dsm) and bit_equal(got.weight, want.weight), mode
        assert (got.xoff, got.yoff, got.zone, got.roi) == (want.xoff, want.yoff, "17R", want.roi)
        assert int(got.weight.sum()) == sum(r.shape[0] for r, _ in views) and int(torch.isfinite(got.dsm).sum()) > 0
    torch.manual_seed(5)
    free = dsm.render_fused_dsm(models, views, args, center, RANGE, resolution=2.0)
    assert bit_equal(free.dsm, auto.dsm) and (free.xoff, free.yoff) == (auto.xoff, auto.yoff)
    # the fused DSM feeds dsm_mae unchanged
    truth = torch.full(got.dsm.shape, 20.0, dtype=torch.float32, device=DEV)
    mae, err, rdsm, shift = dsm.dsm_mae(got, truth, register="z")
    assert math.isfinite(mae) and math.isfinite(shift) and err.shape == truth.shape
    assert (torch.isfinite(err) == torch.isfinite(got.dsm)).all()
