"""Ray casting against a DSM raster on the GPU: sr_heightfield_blockmax, sr_heightfield_cast and
sr_heightfield_shadow against the brute-force reference of tests/heightfield_reference.py (which is not a walk), the two-level walk
against the plain one bit for bit, the scene-frame rays against sr_depth_to_utm and against the all-numpy chain, and the three functions
of satnerf_amd.dsm built on them.

Comparisons with the reference leave out the rays it calls unstable (grazes and corner touches: the cell changes when the heights move
by delta or the segment moves by delta east or north); tests/test_heightfield_host.py holds those to at most 1 % of every input.
On the stable rays the cell is equal and |ds| |B - A| <= 1e-9 m: both sides are fp64 on coordinates below 1e3 m, where the spacing is
1e-13 m."""
import functools

import numpy as np
import pytest
import torch

from tests import heightfield_reference as H
from tests import sun_rays_reference as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCENES = ["jax", "cape_town"]


def _t(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def _scene_dsm(name):
    from satnerf_amd import dsm

    s = S.scene(name)["s"]
    xoff, yoff, _, _, r = s["grid"]
    hgt = _t(H.scene_raster(name))
    return dsm.DSM(hgt, torch.ones_like(hgt), xoff, yoff, r, f"{s['zone']}{'R' if name == 'jax' else 'H'}"), s


def _compare(got_s, got_cell, want_s, want_cell, stable, length, what):
    """test 2's comparison: equal cells (misses included) and |ds| |B - A| <= 1e-9 m on the stable rays"""
    got_s, got_cell = got_s.cpu().numpy(), got_cell.cpu().numpy()
    assert stable.mean() >= 0.99
    bad = stable & (got_cell != want_cell)
    assert not bad.any(), (what, np.flatnonzero(bad)[:5], got_cell[bad][:5], want_cell[bad][:5])
    assert (np.isnan(got_s) == (got_cell < 0)).all()
    hit = stable & (want_cell >= 0)
    err = (np.abs(got_s - want_s) * length)[hit].max() if hit.any() else 0.0
    print(f"{what}: {hit.sum()} stable hits, {(stable & (want_cell < 0)).sum()} stable misses, {(~stable).sum()} unstable; "
          f"max |ds| |B - A| = {err:.2e} m")
    assert err <= 1e-9


# ---- 1: block maxima --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(H.RASTERS))
def test_block_maxima_equal_numpys(name):
    from satnerf_amd import ops

    hgt = H.raster(name)
    bm, top = ops.heightfield_blockmax(_t(hgt))
    want_bm, want_top = H.blockmax_np(hgt)
    assert bm.shape == want_bm.shape and bm.dtype == torch.float32 and top.shape == (1,)
    assert (bm.cpu().numpy().view(np.uint32) == want_bm.view(np.uint32)).all()
    assert top.cpu().numpy().view(np.uint32)[0] == np.float32(want_top).view(np.uint32)
    if H.RASTERS[name][2] is not None:
        assert np.isneginf(want_bm[H.RASTERS[name][2]])  # the all-NaN block


def test_block_maxima_of_an_empty_raster_are_minus_infinity():
    from satnerf_amd import ops

    bm, top = ops.heightfield_blockmax(torch.full((17, 5), float("nan"), device=DEV))
    assert bool(torch.isneginf(bm).all()) and bm.shape == (2, 1) and bool(torch.isneginf(top).all())


# ---- 2: grid-frame segments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accelerate", [False, True])
@pytest.mark.parametrize("name", H.SEGMENT_RASTERS)
def test_segments_match_the_brute_force(name, accelerate):
    from satnerf_amd import ops

    A, B = H.segments(name)
    stable, want_s, want_cell = H.segment_truth(name)
    depth, cell, s, seg = ops.heightfield_cast(_t(H.raster(name)), H.RES, seg_a=_t(A, torch.float64), seg_b=_t(B, torch.float64),
                                               accelerate=accelerate, want_s=True)
    assert depth.dtype == torch.float32 and cell.dtype == torch.int32 and s.dtype == torch.float64 and seg is None
    _compare(s, cell, want_s, want_cell, stable, np.linalg.norm(B - A, axis=1), f"{name} accelerate={accelerate}")
    assert torch.equal(_bits(depth), _bits(s.float()))  # with segments the depth is s, rounded once


def test_invalid_segments_are_misses():
    from satnerf_amd import ops

    A, B = (x[:300].copy() for x in H.segments("37x53"))
    bad = [1, 2, 63, 64, 255, 256, 299]
    A[1, 0], A[2, 2], B[63, 1], B[64, 0], A[255, 1], B[256, 2], B[299, 0] = np.nan, np.inf, -np.inf, np.nan, 1e308, np.nan, -1e308
    B[255, 1] = -1e308  # finite ends whose difference is not
    for accelerate in (False, True):
        depth, cell, s, _ = ops.heightfield_cast(_t(H.raster("37x53")), H.RES, seg_a=_t(A, torch.float64), seg_b=_t(B, torch.float64),
                                                 accelerate=accelerate, want_s=True)
        cell = cell.cpu().numpy()
        assert (cell[bad] == -1).all() and bool(torch.isnan(depth[bad]).all()) and bool(torch.isnan(s[bad]).all())
        keep = np.setdiff1d(np.arange(300), bad)
        assert (cell[keep] == H.segment_truth("37x53")[2][keep])[H.segment_truth("37x53")[0][keep]].all()


# ---- 3: plain against two-level --------------------------------------------------------------------------------------------------------------
def _both(call):
    plain, fast = call(False), call(True)
    for p, f in zip(plain, fast):
        if p is not None:
            assert torch.equal(_bits(p), _bits(f))
    return plain


@pytest.mark.parametrize("name", sorted(H.RASTERS))
def test_two_level_walk_is_bit_identical_on_segments(name):
    from satnerf_amd import ops

    hgt = _t(H.raster(name))
    A, B = H.segments(name)
    Ae, Be = H.edge_segments(name)  # exact diagonals and cell edges: unstable by construction, equal all the same
    a, b = _t(np.concatenate([A, Ae]), torch.float64), _t(np.concatenate([B, Be]), torch.float64)
    depth, cell, s, _ = _both(lambda acc: ops.heightfield_cast(hgt, H.RES, seg_a=a, seg_b=b, accelerate=acc, want_s=True))
    want = H.cast_np(H.raster(name), H.RES, Ae, Be)[1]  # the tie rule itself: the reference agrees on these lines too
    assert (cell[len(A):].cpu().numpy() == want).all()


@pytest.mark.parametrize("name", SCENES)
def test_two_level_walk_is_bit_identical_on_scene_rays(name):
    from satnerf_amd import ops

    d, s = _scene_dsm(name)
    rays = _t(H.scene_rays(name))
    _both(lambda acc: ops.heightfield_cast(d.dsm, d.resolution, rays=rays, center=s["center"], scene_range=s["scene_range"], zone=s["zone"],
                                           xoff=d.xoff, yoff=d.yoff, accelerate=acc, want_s=True, want_seg=True))


@pytest.mark.parametrize("name,elevation,azimuth", H.SHADOW_CASES)
def test_two_level_walk_is_bit_identical_on_shadow_masks(name, elevation, azimuth):
    from satnerf_amd import ops

    hgt = _t(H.raster(name))
    for bias in (0.0, 0.25):
        _both(lambda acc: (ops.heightfield_shadow(hgt, H.RES, S.sun_direction(elevation, azimuth), bias=bias, accelerate=acc),))


# ---- 4: scene-frame rays ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_scene_rays_walk_the_segment_depth_to_utm_gives(name):
    from satnerf_amd import ops

    d, s = _scene_dsm(name)
    rays_np = H.scene_cast_inputs(name)[0]
    rays = _t(rays_np)
    scene = (s["center"], s["scene_range"])
    depth, cell, sg, seg = ops.heightfield_cast(d.dsm, d.resolution, rays=rays, center=scene[0], scene_range=scene[1], zone=s["zone"],
                                                xoff=d.xoff, yoff=d.yoff, want_s=True, want_seg=True)
    ends = [torch.stack(ops.depth_to_utm(rays, rays[:, col].contiguous(), *scene, zone=s["zone"])[:3], 1) for col in (6, 7)]
    assert torch.equal(_bits(seg), _bits(torch.cat(ends, 1)))  # bit for bit
    if name == "cape_town":
        assert bool((seg[:, 1] < 0).all())  # zone 34 south: negative northings
    # test 2's comparison on the GPU's own end points
    U = seg.cpu().numpy()
    A, B = H.to_grid(U[:, 0:3], d.xoff, d.yoff), H.to_grid(U[:, 3:6], d.xoff, d.yoff)
    stable, want_s, want_cell = H.stable_np(H.scene_raster(name), d.resolution, A, B, H.DELTA)
    _compare(sg, cell, want_s, want_cell, stable, np.linalg.norm(B - A, axis=1), name)
    # the depth: near + s (far - near) in fp64, rounded once
    near, far = rays_np[:, 6].astype(np.float64), rays_np[:, 7].astype(np.float64)
    want_depth = (near + sg.cpu().numpy() * (far - near)).astype(np.float32)
    assert (depth.cpu().numpy().view(np.uint32) == want_depth.view(np.uint32))[cell.cpu().numpy() >= 0].all()
    nadir = np.arange(len(rays_np)) < -(-37 * 53 // H.SCENE_STEP)
    own = (np.arange(37 * 53)[::H.SCENE_STEP])  # a nadir ray over a finite cell sees that cell
    finite = np.isfinite(H.scene_raster(name).ravel()[own])
    assert (cell.cpu().numpy()[nadir][finite] == own[finite]).all()


def test_invalid_scene_rays_are_misses():
    from satnerf_amd import dsm

    d, s = _scene_dsm("jax")
    rays = H.scene_rays("jax")[:300].copy()
    bad = [0, 1, 63, 64, 255, 299]
    rays[0, 0], rays[1, 4], rays[63, 6], rays[64, 7], rays[255, 2] = np.nan, np.inf, np.nan, -np.inf, -np.inf
    rays[299, 6], rays[299, 7] = rays[299, 7], rays[299, 6]  # far < near
    out = dsm.cast_rays(d, _t(rays), s["center"], s["scene_range"])
    clean = dsm.cast_rays(d, _t(H.scene_rays("jax")[:300]), s["center"], s["scene_range"])
    keep = np.setdiff1d(np.arange(300), bad)
    assert not bool(out["hit"][bad].any()) and bool((out["cell"][bad] == -1).all()) and bool(torch.isnan(out["depth"][bad]).all())
    assert torch.equal(out["cell"][keep], clean["cell"][keep]) and torch.equal(_bits(out["depth"][keep]), _bits(clean["depth"][keep]))


# ---- 5: dsm.cast_rays end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_cast_rays_matches_the_numpy_chain(name):
    """Against utm_forward_np and the brute force: equal cells on the rays stable at 1e-5 m, and |dt| <= 2e-6 m / scene_range + one fp32
    ulp of t -- the project's own 1e-6 m agreement of utm_from_latlon with numpy, at either end of the segment."""
    from satnerf_amd import dsm

    d, s = _scene_dsm(name)
    rays_np = H.scene_cast_inputs(name)[0]
    stable, want_s, want_cell = H.scene_truth(name)
    assert stable.mean() >= 0.99
    out = dsm.cast_rays(d, _t(rays_np), s["center"], s["scene_range"])  # the zone comes from the DSM
    assert set(out) == {"depth", "cell", "hit"} and out["hit"].dtype == torch.bool and out["depth"].shape == (len(rays_np),)
    cell, depth = out["cell"].cpu().numpy(), out["depth"].cpu().numpy().astype(np.float64)
    assert (out["hit"].cpu().numpy() == (cell >= 0)).all()
    bad = stable & (cell != want_cell)
    assert not bad.any(), (np.flatnonzero(bad)[:5], cell[bad][:5], want_cell[bad][:5])
    near, far = rays_np[:, 6].astype(np.float64), rays_np[:, 7].astype(np.float64)
    want_t = near + want_s * (far - near)
    hit = stable & (want_cell >= 0)
    err = np.abs(depth - want_t)[hit]
    tol = (2e-6 / s["scene_range"] + np.spacing(want_t.astype(np.float32)).astype(np.float64))[hit]
    print(f"{name}: {hit.sum()} stable hits, max |dt| = {err.max():.2e} (scene units; {err.max() * s['scene_range']:.2e} m), "
          f"worst err / tol = {(err / tol).max():.3f}")
    assert (err <= tol).all()
    same = dsm.cast_rays(d, _t(rays_np), s["center"], s["scene_range"], zone=s["zone"], accelerate=False)
    assert torch.equal(same["cell"], out["cell"]) and torch.equal(_bits(same["depth"]), _bits(out["depth"]))


# ---- 6: shadow masks ------------------------------------------------------------------------------------------------------------------------------
def _dsm_of(hgt, r=H.RES):
    from satnerf_amd import dsm

    hgt = _t(hgt)
    return dsm.DSM(hgt, torch.ones_like(hgt), 1000.25, 2000.0, r, "17R")


@pytest.mark.parametrize("name,elevation,azimuth", H.SHADOW_CASES)
def test_shadow_mask_matches_the_brute_force(name, elevation, azimuth):
    from satnerf_amd import data, dsm

    want, stable = H.shadow_truth(name, elevation, azimuth)
    assert stable.mean() >= 0.99
    sun = S.sun_direction(elevation, azimuth)
    got = dsm.shadow_mask(_dsm_of(H.raster(name)), sun)
    assert got.dtype == torch.float32 and got.shape == want.shape
    g = got.cpu().numpy()
    assert (np.isnan(g) == np.isnan(H.raster(name))).all()
    solid = stable & ~np.isnan(want)
    assert (g[solid] == want[solid]).all(), np.argwhere(solid & (g != want))[:5]
    assert set(np.unique(g[~np.isnan(g)])) <= {0.0, 1.0}
    top = np.nanmax(H.raster(name))
    assert (g[H.raster(name) == top] == 1.0).all()  # a cell at the global maximum is lit
    # the fp32 tensor data.sun_direction returns is taken as it is: a direction 1e-8 away, the same cells empty
    other = dsm.shadow_mask(_dsm_of(H.raster(name)), data.sun_direction(elevation, azimuth), accelerate=False)
    assert torch.equal(torch.isnan(other), torch.isnan(got))


def test_flat_raster_is_lit_and_a_bias_lifts_shadows():
    from satnerf_amd import dsm

    flat = np.full((37, 21), 3.0, np.float32)
    flat[5, 6] = np.nan
    got = dsm.shadow_mask(_dsm_of(flat), S.sun_direction(8, 140)).cpu().numpy()
    assert np.isnan(got[5, 6]) and (got[np.isfinite(flat)] == 1.0).all()
    step = np.zeros((1, 20), np.float32)
    step[0, 12:] = 4.0  # sun in the east at 45 degrees: the cells within 4 m of the wall are shadowed
    assert dsm.shadow_mask(_dsm_of(step), (1.0, 0.0, 1.0)).cpu().numpy()[0].tolist() == [1.0] * 4 + [0.0] * 8 + [1.0] * 8
    assert dsm.shadow_mask(_dsm_of(step), (1.0, 0.0, 1.0), bias=1.0).cpu().numpy()[0].tolist() == [1.0] * 6 + [0.0] * 6 + [1.0] * 8
    assert dsm.shadow_mask(_dsm_of(step), (1.0, 0.0, 1.0), bias=4.0).cpu().numpy()[0].tolist() == [1.0] * 20
    with pytest.raises(ValueError, match="horizon"):
        dsm.shadow_mask(_dsm_of(step), (1.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="horizon"):
        dsm.shadow_mask(_dsm_of(step), (1.0, 0.0, -0.2))
    with pytest.raises(ValueError, match="bias"):
        dsm.shadow_mask(_dsm_of(step), (1.0, 0.0, 1.0), bias=-1.0)


@pytest.mark.parametrize("elevation,azimuth", [(60.0, 40.0), (25.0, 140.0), (8.0, 40.0)])
def test_a_towers_shadow_has_length_h_over_tan_elevation(elevation, azimuth):
    """One tower of one cell on flat ground.  A ground cell is shadowed when its ray enters the tower's square no farther than L = h /
    tan(elevation) away; the tower's centre projects onto that ray at most r / sqrt(2) behind the entry.  So the farthest shadowed
    centre, measured along the sun's azimuth from the tower's centre, lies at most r / sqrt(2) beyond L, and -- the shadow being a
    band at least r wide, which holds a cell centre in every stretch of sqrt(2) r -- no more than sqrt(2) r short of it."""
    from satnerf_amd import dsm

    r, h, n = 0.5, 4.0, 141
    length = h / np.tan(np.radians(elevation))
    assert length < 0.45 * n * r
    hgt = np.zeros((n, n), np.float32)
    hgt[n // 2, n // 2] = h
    got = dsm.shadow_mask(_dsm_of(hgt, r), S.sun_direction(elevation, azimuth)).cpu().numpy()
    jj, cc = np.nonzero(got == 0.0)
    assert len(jj) > 0 and got[n // 2, n // 2] == 1.0
    az = np.radians(azimuth)
    # east = (c - c0) r, north = -(j - j0) r; the shadow falls away from the sun
    reach = -((cc - n // 2) * r * np.sin(az) - (jj - n // 2) * r * np.cos(az))
    print(f"elevation {elevation}: shadow reaches {reach.max():.3f} m, h / tan = {length:.3f} m, {len(jj)} cells")
    assert length - np.sqrt(2) * r <= reach.max() <= length + r / np.sqrt(2)
    assert reach.min() > 0


# ---- 7: the DSM's shadows in a view's pixels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_sun_visibility_from_dsm(name):
    from satnerf_amd import data, dsm

    d, s = _scene_dsm(name)
    sc = S.scene(name)
    rays, depth = sc["rays"].copy(), sc["depth"].copy()
    depth[[3, 70, 300]] = np.nan, np.inf, -np.inf
    rays[5, 8:11] = (0.3, 0.4, -0.1)  # this ray's own sun is below the horizon
    scene = (s["center"], s["scene_range"], s["max_alt"])
    for sun in (None, tuple(sc["sun"])):
        got = dsm.sun_visibility_from_dsm(d, _t(rays), _t(depth), *scene, sun_d=sun, n_samples=64)
        rows, valid = data.sun_rays(_t(rays), _t(depth), *scene, sun_d=sun, n_samples=64, return_valid=True)
        hit = dsm.cast_rays(d, rows, s["center"], s["scene_range"])["hit"]
        assert got.shape == (len(rays),) and got.dtype == torch.float32
        bad = [3, 70, 300] + ([5] if sun is None else [])
        assert not bool(valid[bad].any()) and int((~valid).sum()) == len(bad) and bool(torch.isnan(got[~valid]).all())
        assert torch.equal(got[valid], torch.where(hit, 0.0, 1.0).float()[valid])
        assert 0.0 < float(got[valid].mean()) < 1.0  # both outcomes occur
    fixed = dsm.sun_visibility_from_dsm(d, _t(rays), _t(depth), *scene, sun_d=tuple(sc["sun"]), bias=0.004)
    assert fixed.shape == got.shape and bool(torch.isnan(fixed[[3, 70, 300]]).all())
