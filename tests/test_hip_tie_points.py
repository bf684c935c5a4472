"""Tie-point interpolation on the GPU (study_depth_supervision.py:18-203) against the numpy restatement
(tests/tie_point_reference.py, itself pinned to the reference by tests/test_tie_points_host.py): exact neighbour sets and IDW values,
adversarial kNN layouts, the reflect Gaussian, determinism, the error paths, and the tie-point DSMs end to end."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import rpc_oracle as R
from tests import depth_supervision_reference as D
from tests import tie_point_reference as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCENE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_supervision")


def _gpu_idw(pts, z, N, query=None, h=0, w=0):
    from satnerf_amd import ops

    q = None if query is None else torch.from_numpy(np.ascontiguousarray(query, np.float64)).to(DEV)
    out, idx = ops.idw_interpolate(torch.from_numpy(np.ascontiguousarray(pts, np.float64)).to(DEV),
                                   torch.from_numpy(np.asarray(z, np.float32)).to(DEV), N, query=q, height=h, width=w, want_indices=True)
    return out.cpu().numpy(), idx.cpu().numpy()


def _exact(pts, z, N, query=None, h=0, w=0):
    """GPU neighbours identical to brute force ((d^2, index) order) and values within 1e-12 max|z|."""
    got, gidx = _gpu_idw(pts, z, N, query, h, w)
    q = T.raster_queries(h, w) if query is None else query
    idx, d2 = T.knn(pts, q, N)
    assert np.array_equal(gidx, idx), np.argwhere(gidx != idx)[:5]
    want = T.idw_values(z, idx, d2)
    assert np.abs(got - want).max() <= 1e-12 * max(np.abs(z).max(), 1e-30)
    return got


def _scene_depths():
    from satnerf_amd import data

    images, pts3d, center, rng = D.load_scene(SCENE)
    _, depths, _ = data.depth_supervision_from_keypoints(images, pts3d, torch.from_numpy(center), float(rng), DEV)
    return images, depths[:, 0].cpu().numpy(), center, rng


def test_scene_rasters_match_brute_force():
    images, depth, _, _ = _scene_depths()
    off = 0
    for d in images:
        cr = np.asarray(d["keypoints"]["2d_coordinates"], np.float64)
        z = depth[off:off + cr.shape[0]]
        off += cr.shape[0]
        h, w = int(d["height"]), int(d["width"])
        valid = (cr[:, 0] < w) & (cr[:, 0] >= 0) & (cr[:, 1] < h) & (cr[:, 1] >= 0)
        _exact(cr[valid], z[valid], 8, h=h, w=w)


@pytest.mark.parametrize("N", [1, 3, 8, 16, 32])
def test_adversarial_knn(N):
    g = np.random.default_rng(N)
    h, w = 40, 56
    lattice = np.stack(np.meshgrid(np.arange(0, w, 4.0), np.arange(0, h, 4.0)), -1).reshape(-1, 2)
    cases = {
        "one_cell": np.stack([g.uniform(20, 20.001, 60), g.uniform(10, 10.001, 60)], 1),
        "corner": np.stack([g.uniform(0, 3, 80), g.uniform(0, 2, 80)], 1),
        "lattice": g.permutation(lattice),  # integer lattice: exact ties everywhere, on cell edges too
        "duplicates": np.concatenate([lattice[:40], lattice[:40], g.uniform(0, 50, (30, 2))]),
        "k_equals_n": g.uniform(0, 50, (N, 2)),
        "line": np.stack([g.uniform(0, w, 70), np.full(70, 13.0)], 1),  # zero extent in y
    }
    far = np.array([[-1e6, -1e6], [1e6, 3.0], [25.0, -2e5], [3e4, 3e4], [-0.5, -0.5], [w + 0.25, h - 1.0]])
    for name, pts in cases.items():
        if pts.shape[0] < N:
            continue
        z = g.normal(0.0, 5.0, pts.shape[0]).astype(np.float32)
        _exact(pts, z, N, h=h, w=w)
        _exact(pts, z, N, query=np.concatenate([far, g.uniform(-100, 150, (300, 2))]))


def test_exact_hits():
    pts = np.array([[3.0, 4.0], [10.0, 2.0], [7.5, 7.25], [0.0, 0.0], [11.0, 9.0], [3.0, 4.0]])
    z = np.array([1.5, -2.0, 4.0, 8.0, 3.25, 99.0], np.float32)
    for N in (1, 3, 5):
        got, _ = _gpu_idw(pts, z, N, h=10, w=12)
        for (c, r), v in ((pts[0], z[0]), (pts[1], z[1]), (pts[3], z[3]), (pts[4], z[4])):  # the duplicate at (3, 4) loses: index 5
            assert got[int(r) * 12 + int(c)] == np.float64(v)


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (17, 23), (29, 13), (120, 88)])
@pytest.mark.parametrize("sigma", [0.0, 0.5, 1.0, 3.0, 20.0])
def test_gaussian_matches_restatement(shape, sigma):
    from satnerf_amd import tie_points

    x = np.random.default_rng(shape[0] * 7 + shape[1]).normal(0.0, 1.0, shape)
    got = tie_points.gaussian_filter(torch.from_numpy(x).to(DEV), sigma).cpu().numpy()
    want = T.gaussian_filter(x, sigma)
    assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    got2 = tie_points.gaussian_filter(torch.from_numpy(x).to(DEV), (sigma, 2.0)).cpu().numpy()
    assert np.abs(got2 - T.gaussian_filter(x, [sigma, 2.0])).max() <= 1e-12 * np.abs(want).max()


def test_two_runs_are_bitwise_equal():
    from satnerf_amd import ops, tie_points

    g = np.random.default_rng(5)
    pts = torch.from_numpy(np.stack([g.uniform(0, 300, 3000), g.uniform(0, 200, 3000)], 1)).to(DEV)
    z = torch.from_numpy(g.normal(0, 1, 3000).astype(np.float32)).to(DEV)
    a = [ops.idw_interpolate(pts, z, 8, height=200, width=300, want_indices=True) for _ in range(2)]
    assert torch.equal(a[0][0].view(torch.int64), a[1][0].view(torch.int64)) and torch.equal(a[0][1], a[1][1])
    b = [tie_points.gaussian_filter(a[0][0].view(200, 300), 3.0) for _ in range(2)]
    assert torch.equal(b[0].view(torch.int64), b[1].view(torch.int64))
    _, seen = ops.idw_interpolate(pts, z, 8, height=200, width=300, want_visited=True)
    assert seen.float().mean().item() < 0.05 * 3000  # the grid, not a scan of every keypoint


def test_error_paths():
    from satnerf_amd import tie_points

    pts = torch.tensor([[1.0, 1.0], [2.0, 3.0], [5.0, 4.0], [50.0, 50.0]], dtype=torch.float64, device=DEV)
    vals = torch.ones(4, device=DEV)
    with pytest.raises(ValueError, match="img_x: 3 keypoints lie inside"):
        tie_points.interpolate_tie_points(10, 10, pts, vals, N=4, name="img_x")
    with pytest.raises(ValueError, match="empty"):
        tie_points.interpolate_tie_points(0, 10, pts, vals, N=2)
    with pytest.raises(ValueError, match="non-empty"):
        tie_points.gaussian_filter(torch.zeros(0, 5, dtype=torch.float64, device=DEV), 1.0)
    img = torch.zeros(8, 8, dtype=torch.float64, device=DEV)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            tie_points.gaussian_filter(img, bad)
    with pytest.raises(ValueError, match="MAX_RADIUS"):
        tie_points.gaussian_filter(img, 60.0)
    with pytest.raises(ValueError, match="GPU"):
        tie_points.idw_interpolation(pts.cpu(), vals.cpu(), pts.cpu())
    with pytest.raises(ValueError, match="GPU"):
        tie_points.gaussian_filter(img.cpu(), 1.0)
    with pytest.raises(ValueError, match="N = 8"):
        tie_points.idw_interpolation(pts, vals, pts)
    with pytest.raises(ValueError, match="float32"):
        tie_points.idw_interpolation(pts, vals.double(), pts, N=2)
    with pytest.raises(ValueError, match="finite"):
        tie_points.idw_interpolation(torch.tensor([[0.0, float("nan")], [1.0, 1.0]], dtype=torch.float64, device=DEV), vals[:2], pts, N=1)
    images, pts3d, center, rng = D.load_scene(SCENE)
    few = [dict(d) for d in images]
    few[2] = dict(few[2], height=3, width=3)
    with pytest.raises(ValueError, match="img_02.json: .* keypoints lie inside the 3 x 3 image"):
        tie_points.tie_point_dsms_from_keypoints(few, pts3d, torch.from_numpy(center), float(rng), device=DEV,
                                                 names=[f"img_{k:02d}.json" for k in range(len(few))])


def _roi_of_scene(pts3d, r=1.0):
    from satnerf_amd import dsm

    lat, lon, _ = D.ecef_to_latlon(pts3d[:, 0], pts3d[:, 1], pts3d[:, 2])
    e, n = dsm.utm_from_latlon(torch.from_numpy(lat).to(DEV), torch.from_numpy(lon).to(DEV))
    e, n = e.cpu().numpy(), n.cpu().numpy()
    size = int(np.ceil(max(e.max() - e.min(), n.max() - n.min()) / r)) + 20
    return np.array([np.floor(e.min()) - 10 * r, np.floor(n.min()) - 10 * r, size, r])


def test_tie_point_dsms_end_to_end():
    from satnerf_amd import data, dsm, tie_points

    images, pts3d, center, rng = D.load_scene(SCENE)
    roi = _roi_of_scene(pts3d)
    dsms, rasters = tie_points.tie_point_dsms(SCENE, roi=roi, return_depths=True)
    assert len(dsms) == len(images) == len(rasters)
    _, depth, _, _ = _scene_depths()
    off = 0
    for d, out, raster in zip(images, dsms, rasters):
        h, w = int(d["height"]), int(d["width"])
        rays = data.rays_from_rpc(d["rpc"], h, w, float(d["min_alt"]), float(d["max_alt"]), center, float(rng), float(d["sun_elevation"]),
                                  float(d["sun_azimuth"]), device=DEV)
        again = dsm.dsm_from_depth(rays, raster.reshape(-1), center, float(rng), roi=roi)
        assert torch.equal(out.dsm.view(torch.int32), again.dsm.view(torch.int32))
        # the restatement's raster: the IDW and Gaussian agree to ~1e-15 relative, so the fp32 depths are equal or one ulp apart; one
        # ulp of a normalised depth (~6e-8) times the range moves a point by < 1e-4 m, the gate is 1e-3 m
        cr = np.asarray(d["keypoints"]["2d_coordinates"], np.float64)
        want, _, _, _ = T.interpolate_tie_points(h, w, cr, depth[off:off + cr.shape[0]], smooth=1)
        off += cr.shape[0]
        assert np.abs(raster.cpu().numpy() - want.astype(np.float32)).max() <= 1e-6
        ref = dsm.dsm_from_depth(rays, torch.from_numpy(want.astype(np.float32).ravel()).to(DEV), center, float(rng), roi=roi)
        a, b = out.dsm.cpu().numpy(), ref.dsm.cpu().numpy()
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.isfinite(a).sum() > 1000
        assert np.nanmax(np.abs(a - b)) <= 1e-3


def test_plane_scene(tmp_path):
    """Tie points on a plane of constant altitude: every interpolated depth is a convex combination of keypoint depths (IDW weights
    and Gaussian taps are positive and sum to one), and with keypoints at the image corners the plane's own depth over the image lies in
    the same range.  An altitude changes by at most 1 m per m of depth, so each DSM cell lies within (max - min keypoint depth) x range
    of the plane, plus the fp32 quantisation of ECEF (0.5 m per coordinate) of the tie point and of the ray origin: 2 m."""
    from satnerf_amd import tie_points

    g = np.random.default_rng(11)
    alt0, root = 12.0, str(tmp_path)
    pts, names = [], []
    for t in range(2):
        h, w = 150 + 20 * t, 180
        rpc = R.synthetic_rpc(60 + t, height=h, width=w)
        col = np.concatenate([[1.0, w - 2.0, 1.0, w - 2.0], g.uniform(1, w - 2, 250)])
        row = np.concatenate([[1.0, 1.0, h - 2.0, h - 2.0], g.uniform(1, h - 2, 250)])
        lon, lat = R.localization(rpc, col, row, np.full(col.size, alt0))
        base = sum(len(p) for p in pts)
        pts.append(np.stack(R.latlon_to_ecef(lat, lon, np.full(col.size, alt0)), 1))
        kp = np.stack([col, row], 1) + np.clip(g.normal(0.0, 0.2, (col.size, 2)), -0.4, 0.4)  # a non-zero mean reprojection error
        d = {"img": f"img_{t:02d}.tif", "height": h, "width": w, "min_alt": -20.0, "max_alt": 60.0, "sun_elevation": 50.0,
             "sun_azimuth": 150.0, "rpc": {k: (v.tolist() if isinstance(v, np.ndarray) else float(v)) for k, v in rpc.items()},
             "keypoints": {"2d_coordinates": kp.tolist(), "pts3d_indices": list(range(base, base + col.size))}}
        names.append(f"img_{t:02d}.json")
        with open(os.path.join(root, names[-1]), "w") as f:
            json.dump(d, f)
    pts3d = np.concatenate(pts)
    np.save(os.path.join(root, "pts3d.npy"), pts3d)
    lo, hi = pts3d.min(0), pts3d.max(0)
    with open(os.path.join(root, "scene.loc"), "w") as f:
        json.dump({f"{a}_scale": float((hi[i] - lo[i]) / 2 + 50.0) for i, a in enumerate("XYZ")} |
                  {f"{a}_offset": float((hi[i] + lo[i]) / 2) for i, a in enumerate("XYZ")}, f)
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("\n".join(names))
    dsms, rasters = tie_points.tie_point_dsms(root, return_depths=True, device=DEV)
    from satnerf_amd import data

    _, depths, ts = data.load_depth_supervision(root, device=DEV)
    _, rng = data.read_scene_loc(root)
    for t, (out, raster) in enumerate(zip(dsms, rasters)):
        dk = depths[ts == t, 0]
        assert raster.min() >= dk.min() - 1e-6 and raster.max() <= dk.max() + 1e-6
        bound = (dk.max() - dk.min()).item() * rng + 2.0
        cells = out.dsm[torch.isfinite(out.dsm)]
        assert cells.numel() > 1000 and (cells - alt0).abs().max().item() <= bound, ((cells - alt0).abs().max().item(), bound)
