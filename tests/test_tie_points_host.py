"""The numpy restatement of the tie-point interpolation (tests/tie_point_reference.py) against what the reference's own
study_depth_supervision functions returned (tests/golden/tie_points/, written by make_tie_point_golden.py with scipy 1.15.3): the
same neighbour sets as cKDTree, IDW within 1e-12 x max|z|, the reflect Gaussian within 1e-12 relative.  CPU only."""
import os

import numpy as np
import pytest

from tests import tie_point_reference as T

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tie_points", "reference.npz")


@pytest.fixture(scope="module")
def g():
    z = np.load(FIX, allow_pickle=False)
    return {k: z[k] for k in z.files}


def same_neighbours(mine, d2, theirs):
    """cKDTree's order on exact distance ties is unspecified: compare as sets, and where the N-th distance is tied with a point left
    out, only the part strictly inside that distance.  Returns the rows whose sets agree: only there must the values agree too (a
    different tied neighbour carries a different z -- the one departure)."""
    assert mine.shape == theirs.shape
    agree = np.ones(mine.shape[0], dtype=bool)
    for i in range(mine.shape[0]):
        if set(mine[i]) != set(theirs[i]):
            inner = d2[i] < d2[i, -1]
            assert set(mine[i][inner]) <= set(theirs[i]), (i, mine[i], theirs[i])
            agree[i] = False
    return agree


def close(a, b, scale):
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    m = ~np.isnan(b)
    assert np.abs(a[m] - b[m]).max(initial=0.0) <= 1e-12 * scale


@pytest.mark.parametrize("t", [0, 3, 7])
def test_scene_images(g, t):
    p = f"scene{t}_"
    h, w = (int(v) for v in g[p + "hw"])
    heat, raw, idx, valid = T.interpolate_tie_points(h, w, g[p + "pts2d"], g[p + "depth"], smooth=1)
    zmax = np.abs(g[p + "depth"][valid]).max()
    crop = g[p + "crop"]
    assert np.array_equal(crop, T.crop_index(h, w))
    close(raw.ravel()[crop], g[p + "idw_crop"], zmax)
    close(heat.ravel()[crop], g[p + "heat_crop"], zmax)
    s = g[p + "nn_sample"]
    _, d2 = T.knn(g[p + "pts2d"][valid], T.raster_queries(h, w)[s], 8)
    assert same_neighbours(idx[s], d2, g[p + "nn"]).all()
    err_heat, _, _, _ = T.interpolate_tie_points(h, w, g[p + "pts2d"], g[p + "err"])  # the heatmap's default smooth 20
    close(err_heat.ravel()[crop], g[p + "err_heat20_crop"], np.abs(g[p + "err"][valid]).max())


@pytest.mark.parametrize("N", [1, 3, 8])
def test_synthetic_rasters(g, N):
    h, w = (int(v) for v in g[f"syn{N}_hw"])
    pts, z = g[f"syn{N}_pts2d"], g[f"syn{N}_z"]
    vals, idx = T.idw_interpolation(pts, z, T.raster_queries(h, w), N)
    _, d2 = T.knn(pts, T.raster_queries(h, w), N)
    agree = same_neighbours(idx, d2, g[f"syn{N}_nn"])
    # duplicated keypoints share z, so a tie between them changes the set but not the value
    agree |= (np.sort(z[idx], axis=1) == np.sort(z[g[f"syn{N}_nn"]], axis=1)).all(1)
    assert agree.mean() > 0.95
    close(vals[agree], g[f"syn{N}_idw"][agree], np.abs(z).max())
    on_pixel = (pts[:, 0] == np.round(pts[:, 0])) & (pts[:, 1] == np.round(pts[:, 1]))
    assert on_pixel.sum() >= 5
    for k in np.nonzero(on_pixel)[0]:  # a query on a keypoint takes z exactly: that of the lowest index at that position
        first = np.nonzero((pts[:, 0] == pts[k, 0]) & (pts[:, 1] == pts[k, 1]))[0][0]
        assert vals[int(pts[k, 1]) * w + int(pts[k, 0])] == np.float64(z[first])


def test_queries_outside_the_image(g):
    vals, idx = T.idw_interpolation(g["out_pts2d"], g["out_z"], g["out_query"])
    _, d2 = T.knn(g["out_pts2d"], g["out_query"], 8)
    assert same_neighbours(idx, d2, g["out_nn"]).all()
    close(vals, g["out_idw"], np.abs(g["out_z"]).max())


@pytest.mark.parametrize("sigma", [0.0, 0.5, 1.0, 3.0, 20.0])
def test_heatmap_gaussian_radius_beyond_the_image(g, sigma):
    heat, _, _, valid = T.interpolate_tie_points(23, 17, g["heat_pts2d"], g["heat_values"], smooth=sigma)
    assert 0 < valid.sum() < valid.size
    want = g[f"heat_sigma{sigma:g}"]
    assert np.abs(heat - want).max() <= 1e-12 * np.abs(want).max()
