"""Orthorectification onto a DSM raster on the GPU: sr_orthorectify and the functions of satnerf_amd.dsm and
satnerf_amd.evaluate built on it against the fp64 numpy reference of tests/orthorectify_reference.py.

colrow is held to eps_px = 1e-11 degrees (what tests/test_hip_ortho.py holds sr_utm_to_latlon to) times the largest partial derivative
of the camera's projection by latitude and longitude over the raster, plus 1e-9 px: derived, not tuned.  Statuses are compared on
the cells the reference calls stable (tests/test_orthorectify_host.py holds the others to 1 %), the two walks bit for bit on every
cell.  Colours are checked from the GPU's own colrow: fed to the numpy samplers it must give every visible cell's colour to within
one fp32 neighbour.  Accumulators and means are compared bit for bit with numpy's accumulation of the GPU's per-view outputs."""
import numpy as np
import pytest
import torch

from tests import ortho_reference as R
from tests import orthorectify_reference as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


def _t(x, dtype=None):
    t = torch.from_numpy(np.array(x, order="C"))  # a copy: the shared inputs are read-only
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _bits(t):
    t = t.contiguous()
    return t.view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[t.element_size()]) if t.dtype != torch.bool else t


def _equal_f32(got, want):
    """Bit-equal fp32 arrays, a NaN matching any NaN (the sign and payload of 0 / 0 are the platform's)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    return bool(((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all())


def _same(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


def _dsm(hgt, grid, zone="17R"):
    from satnerf_amd import dsm

    h = _t(np.asarray(hgt, np.float32))
    return dsm.DSM(h, torch.ones_like(h), grid[0], grid[1], grid[2], zone)


def _case_dsm(name):
    c = T.case(name)
    return _dsm(c["hgt"], c["grid"], f"{c['zone']}{c['letter']}"), c


def _check_colors(got, image, mode, what):
    """The colours of ``got`` (a dict of numpy arrays) against the numpy samplers at the GPU's own colrow."""
    status, colrow, color = got["status"], got["colrow"], got["color"]
    want = T.colors_np(image, status, colrow[:, :, 0], colrow[:, :, 1], mode)
    assert color.dtype == np.float32 and color.shape == want.shape
    assert np.isnan(color[status != T.VISIBLE]).all()
    vis = status == T.VISIBLE
    w, g = want[vis], color[vis]
    nan = np.isnan(w)
    assert (np.isnan(g) == nan).all(), what
    ok = R.within_one_ulp(g[~nan], w[~nan])
    exact = (g[~nan] == w[~nan].astype(np.float32)).mean() if (~nan).any() else 1.0
    print(f"{what}: {vis.sum()} visible cells, {nan.sum()} NaN values, {exact:.4f} of the rest equal to float32(reference)")
    assert ok.all(), (what, np.abs(g[~nan].astype(np.float64) - w[~nan]).max())
    return nan.sum()


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- 1 - 3: colrow, status, the two walks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(T.CASES))
def test_colrow_and_status_match_the_reference(name):
    from satnerf_amd import dsm

    d, c = _case_dsm(name)
    t = T.truth(name)
    image = _t(c["image"])
    fast = dsm.orthorectify(d, image, c["rpc"], accelerate=True)
    plain = dsm.orthorectify(d, image, c["rpc"], accelerate=False)
    assert _same(plain, fast)  # every cell, the unstable ones included
    ysize, xsize = c["hgt"].shape
    channels = T.pixel_values(c["image"]).shape[2]
    assert fast["color"].shape == (ysize, xsize, channels) and fast["color"].dtype == torch.float32
    assert fast["status"].shape == (ysize, xsize) and fast["status"].dtype == torch.uint8
    assert fast["colrow"].shape == (ysize, xsize, 2) and fast["colrow"].dtype == torch.float64 and fast["visible"].dtype == torch.bool
    got = _np(fast)
    assert (got["visible"] == (got["status"] == T.VISIBLE)).all()
    finite = np.isfinite(c["hgt"])
    assert np.isnan(got["colrow"][~finite]).all() and np.isfinite(got["colrow"][finite]).all()  # written outside the image, too
    err = max(np.abs(got["colrow"][:, :, 0] - t["col"])[finite].max(), np.abs(got["colrow"][:, :, 1] - t["row"])[finite].max())
    print(f"{name}: max |colrow - reference| = {err:.3e} px = {err / t['eps']:.3e} of eps_px = {t['eps']:.3e}")
    assert err <= t["eps"]
    stable = ~T.unstable(name)
    assert stable.mean() >= 0.99
    bad = stable & (got["status"] != t["status"])
    assert not bad.any(), (np.argwhere(bad)[:5], got["status"][bad][:5], t["status"][bad][:5])


@pytest.mark.parametrize("name", ["jax_0.3", "cape_town"])
def test_a_bias_lifts_the_start(name):
    from satnerf_amd import dsm

    d, c = _case_dsm(name)
    t = T.truth(name, 1.0)
    got = _np(dsm.orthorectify(d, _t(c["image"]), c["rpc"], bias=1.0))
    stable = ~T.unstable_np(t["col"], t["row"], t["cast_stable"], c["width"], c["height"], t["eps"])
    assert stable.mean() >= 0.99 and (got["status"] == t["status"])[stable].all()
    assert (t["status"] != T.truth(name)["status"]).any()  # the bias changes something


# ---- 4: colours -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("name", sorted(T.CASES))
def test_colours_match_the_samplers_at_the_gpus_own_colrow(name, mode):
    from satnerf_amd import dsm

    d, c = _case_dsm(name)
    got = _np(dsm.orthorectify(d, _t(c["image"]), c["rpc"], mode=mode))
    n_nan = _check_colors(got, c["image"], mode, f"{name} {mode}")
    if name == "cape_town" and mode != "nearest":
        assert n_nan > 0  # the NaN pixel lies under a visible cell's taps and propagates


@pytest.mark.parametrize("mode", T.MODES)
def test_both_pixel_formats_and_strided_images(mode):
    """The uint8 image of a case as fp32 values v / 255 gives the same colours (the division happens in fp64 either way only for uint8:
    the fp32 image is checked against its own reference), and a 3-channel view of a 4-channel buffer is read through its strides."""
    from satnerf_amd import ops

    c = T.case("jax_0.3")
    hgt = _t(c["hgt"])
    args = (hgt, c["grid"][2], c["grid"][0], c["grid"][1], c["zone"], c["rpc"])
    as_f32 = (c["image"].astype(np.float32) / np.float32(255.0)).astype(np.float32)
    color, status, colrow = ops.orthorectify(*args, _t(as_f32), mode=mode)
    _check_colors(dict(color=color.cpu().numpy(), status=status.cpu().numpy(), colrow=colrow.cpu().numpy()), as_f32, mode, f"fp32 {mode}")
    wide = torch.zeros(c["height"], c["width"] + 3, 4, dtype=torch.uint8, device=DEV)
    view = wide[:, 2:2 + c["width"], :3]
    view.copy_(_t(c["image"]))
    assert not view.is_contiguous()
    c2, s2, r2 = ops.orthorectify(*args, view, mode=mode)
    c1, s1, r1 = ops.orthorectify(*args, _t(c["image"]), mode=mode)
    assert torch.equal(_bits(c1), _bits(c2)) and torch.equal(s1, s2) and torch.equal(_bits(r1), _bits(r2))


def test_the_two_launches_alone_give_the_same_bits():
    from satnerf_amd import ops

    c = T.case("hole_0.8")
    hgt, image = _t(c["hgt"]), _t(c["image"])
    args = (hgt, c["grid"][2], c["grid"][0], c["grid"][1], c["zone"], c["rpc"], image)
    whole = ops.orthorectify(*args, mode="bicubic")
    scratch = torch.empty(ops.orthorectify_scratch(hgt.shape[1], hgt.shape[0]), dtype=torch.uint8, device=DEV)
    color = torch.full_like(whole[0], 7.0)
    status = torch.full_like(whole[1], 9)
    _, _, colrow = ops.orthorectify(*args, mode="bicubic", scratch=scratch, color=color, status=status, stage="project")
    assert bool((status == 9).all()) and bool((color == 7.0).all())  # the projection writes neither
    for accelerate in (True, False, True):  # the second launch can run again and again on one projection
        ops.orthorectify(*args, mode="bicubic", accelerate=accelerate, scratch=scratch, color=color, status=status, colrow=colrow, stage="sample")
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(whole, (color, status, colrow)))


# ---- 5: mosaic ------------------------------------------------------------------------------------------------------------------------------
def test_mosaic_is_numpys_accumulation_in_view_order():
    from satnerf_amd import dsm

    d, c = _case_dsm("jax_0.3")
    views = [(_t(image), rpc) for image, rpc in T.mosaic_views()]
    single = [_np(dsm.orthorectify(d, image, rpc, mode="bicubic")) for image, rpc in views]
    total, count, mean = T.mosaic_np([s["color"] for s in single], [s["status"] for s in single])
    got = dsm.ortho_mosaic(d, views, mode="bicubic")
    assert got["count"].dtype == torch.int32 and got["color"].dtype == torch.float32
    assert (got["count"].cpu().numpy() == count).all()
    assert _equal_f32(got["color"].cpu().numpy(), mean)
    assert all((count == k).any() for k in range(4)) and np.isnan(mean[count == 0]).all() and np.isfinite(mean[count > 0]).all()
    for min_views in (2, 3):
        masked = dsm.ortho_mosaic(d, views, mode="bicubic", min_views=min_views)
        want = np.where((count >= min_views)[:, :, None], mean, np.float32(NAN))
        assert _equal_f32(masked["color"].cpu().numpy(), want) and (masked["count"].cpu().numpy() == count).all()
    again = dsm.ortho_mosaic(d, views, mode="bicubic")
    assert _same(got, again)
    other_order = dsm.ortho_mosaic(d, views[::-1], mode="bicubic")
    assert torch.equal(other_order["count"], got["count"])


def test_accumulators_hold_the_fp64_sums():
    from satnerf_amd import ops

    c = T.case("jax_0.3")
    hgt = _t(c["hgt"])
    ysize, xsize = hgt.shape
    total = torch.zeros(ysize, xsize, 3, dtype=torch.float64, device=DEV)
    count = torch.zeros(ysize, xsize, dtype=torch.int32, device=DEV)
    colors, statuses = [], []
    for image, rpc in T.mosaic_views():
        color, status, _ = ops.orthorectify(hgt, c["grid"][2], c["grid"][0], c["grid"][1], c["zone"], rpc, _t(image), sum=total, count=count)
        colors.append(color.cpu().numpy()), statuses.append(status.cpu().numpy())
    want_total, want_count, _ = T.mosaic_np(colors, statuses)
    assert (total.cpu().numpy().view(np.uint64) == want_total.view(np.uint64)).all() and (count.cpu().numpy() == want_count).all()
    with pytest.raises(ValueError, match="both accumulators"):
        ops.orthorectify(hgt, c["grid"][2], c["grid"][0], c["grid"][1], c["zone"], c["rpc"], _t(c["image"]), sum=total)


# ---- 6: hand-built cases --------------------------------------------------------------------------------------------------------------------
def test_a_flat_raster_has_no_occluded_cell():
    from satnerf_amd import dsm

    for name in ("jax_0.3", "hole_0.8"):
        c = T.case(name)
        flat = np.where(np.isfinite(c["hgt"]), np.float32(11.0), np.float32(NAN))
        for accelerate in (True, False):
            status = dsm.orthorectify(_dsm(flat, c["grid"]), _t(c["image"]), c["rpc"], accelerate=accelerate)["status"].cpu().numpy()
            assert (status == T.status_np(flat, c["grid"], c["zone"], c["rpc"], delta=None)[0]).all()
            assert not (status == T.OCCLUDED).any() and (status == T.VISIBLE).any() and (status == T.OUTSIDE).any()


def test_a_tower_hides_the_cells_behind_it_and_stands_visible():
    from satnerf_amd import dsm

    hgt, grid, zone, rpc = T.tower_case()
    image = _t(T.image_u8(rpc["_height"], rpc["_width"], 3, 7))
    for accelerate in (True, False):
        status = dsm.orthorectify(_dsm(hgt, grid), image, rpc, accelerate=accelerate)["status"].cpu().numpy()
        T.check_tower(status)  # the global maximum visible included
        assert (status == T.status_np(hgt, grid, zone, rpc)[0]).all()


def test_the_global_maximum_is_visible():
    from satnerf_amd import dsm

    checked = 0
    for name in sorted(T.CASES):
        d, c = _case_dsm(name)
        status = dsm.orthorectify(d, _t(c["image"]), c["rpc"])["status"].cpu().numpy()
        at = (c["hgt"] == np.nanmax(c["hgt"])) & (status != T.OUTSIDE)
        assert (status[at] == T.VISIBLE).all()
        checked += bool(at.any())
    assert checked >= 2


def test_a_camera_on_the_cell_centres_reproduces_its_image():
    from satnerf_amd import dsm

    hgt, grid, zone, rpc, image = T.grid_camera_case()
    ysize, xsize = hgt.shape
    out = dsm.orthorectify(_dsm(hgt, grid), _t(image), rpc, mode="nearest")
    assert bool(out["visible"].all())
    want = (image[2:2 + ysize, 2:2 + xsize].astype(np.float64) / 255.0).astype(np.float32)
    assert (out["color"].cpu().numpy() == want).all()


def test_one_cell_all_nan_and_one_pixel():
    from satnerf_amd import dsm

    d, c = _case_dsm("one_cell")
    out = dsm.orthorectify(d, _t(c["image"]), c["rpc"])
    assert out["status"].tolist() == [[T.VISIBLE]] and bool(torch.isfinite(out["color"]).all())
    empty = np.full((21, 19), NAN, np.float32)
    for accelerate in (True, False):  # gmax is -inf: nothing is projected and nothing is walked
        out = dsm.orthorectify(_dsm(empty, c["grid"]), _t(c["image"]), c["rpc"], accelerate=accelerate)
        assert bool((out["status"] == T.EMPTY).all()) and bool(torch.isnan(out["color"]).all()) and bool(torch.isnan(out["colrow"]).all())
    # a 1 x 1 image covers the single point (0, 0): a cell is inside only if it projects exactly there
    d, c = _case_dsm("jax_0.3")
    pixel = torch.full((1, 1, 3), 128, dtype=torch.uint8, device=DEV)
    out = _np(dsm.orthorectify(d, pixel, c["rpc"], mode="bicubic"))
    hit = (out["colrow"][:, :, 0] == 0) & (out["colrow"][:, :, 1] == 0)
    assert np.isin(out["status"][~hit], (T.EMPTY, T.OUTSIDE)).all() and np.isnan(out["color"][~hit]).all()
    # ... and sampled anywhere by an affine camera that sends every cell to (0, 0), it is the pixel's value
    hgt, grid, zone, rpc, _ = T.grid_camera_case()
    flat = dict(rpc, col_num=np.zeros(20), row_num=np.zeros(20))
    for mode in T.MODES:
        out = dsm.orthorectify(_dsm(hgt, grid), pixel, flat, mode=mode)
        assert bool(out["visible"].all()) and bool((out["color"] == np.float32(128 / 255.0)).all())
    gray = dsm.orthorectify(_dsm(hgt, grid), torch.full((1, 1), 0.25, device=DEV), flat)  # (H, W) gains its channel
    assert gray["color"].shape == hgt.shape + (1,) and bool((gray["color"] == 0.25).all())


def test_errors_with_a_gpu_at_hand():
    from satnerf_amd import dsm

    d, c = _case_dsm("one_cell")
    cpu = dsm.DSM(d.dsm.cpu(), d.weight.cpu(), d.xoff, d.yoff, d.resolution, d.zone)
    with pytest.raises(ValueError, match="GPU"):
        dsm.orthorectify(cpu, _t(c["image"]), c["rpc"])
    with pytest.raises(ValueError, match="GPU"):
        dsm.orthorectify(d, torch.from_numpy(np.array(c["image"])), c["rpc"])
    with pytest.raises(ValueError, match="same channel count"):
        dsm.ortho_mosaic(d, [(_t(c["image"]), c["rpc"]), (_t(c["image"][:, :, :1]), c["rpc"])])
    with pytest.raises(ValueError, match="20 RPC00B"):
        dsm.orthorectify(d, _t(c["image"]), dict(c["rpc"], col_num=[0.0] * 19))


# ---- the dataset and the metric ---------------------------------------------------------------------------------------------------------------
def test_a_dataset_split_becomes_a_mosaic(tmp_path):
    from satnerf_amd import data, dsm
    from tests.test_orthorectify_host import write_dataset

    root = str(tmp_path)
    write_dataset(root)
    d, c = _case_dsm("jax_0.3")
    for split, downscale in (("train", 1.0), ("train", 2.0), ("val", 1.0)):
        metas, _ = data._split_images(root, split, downscale)
        rgbs = data.load_colors(root, root + "/imgs", split=split, img_downscale=downscale, device=DEV)
        views, off = [], 0
        for k, (meta, h, w) in enumerate(metas):
            rows = rgbs[off:off + h * w] if split == "train" else rgbs[k]
            off += h * w
            views.append((rows.view(h, w, 3), data.rescale_rpc(meta["rpc"], 1.0 / downscale)))
        want = dsm.ortho_mosaic(d, views, mode="bilinear", min_views=1)
        got = dsm.orthorectify_dataset(d, root, root + "/imgs", split=split, img_downscale=downscale, mode="bilinear", min_views=1)
        assert _same(want, got) and int(got["count"].max()) == len(metas)  # the cameras of synthetic_rpc see the whole raster


def test_ortho_psnr_scores_the_cells_the_views_see():
    from satnerf_amd import dsm, evaluate

    d, c = _case_dsm("jax_0.3")
    views = [(_t(image), rpc) for image, rpc in T.mosaic_views()]
    mosaic = dsm.ortho_mosaic(d, views)
    color, count = mosaic["color"].cpu().numpy().astype(np.float64), mosaic["count"].cpu().numpy()
    rng = np.random.default_rng(5)
    rgb = rng.uniform(0, 1, color.shape).astype(np.float32)
    rgb[3, 4] = np.nan  # a cell the render left empty counts nowhere
    for min_views in (1, 2):
        valid = (count >= min_views) & np.isfinite(color).all(-1) & np.isfinite(rgb).all(-1)
        want = -10 * np.log10(((rgb.astype(np.float64) - color)[valid] ** 2).mean())
        for shaped in (rgb, rgb.reshape(-1, 3)):
            got = evaluate.ortho_psnr(_t(shaped), mosaic, min_views=min_views)
            assert got.dtype == torch.float32 and got.dim() == 0 and abs(got.item() - want) <= 1e-5 * abs(want)
    assert torch.isnan(evaluate.ortho_psnr(_t(rgb), mosaic, min_views=4)).item()
    with pytest.raises(ValueError, match="colours"):
        evaluate.ortho_psnr(_t(rgb[:, :, :2]), mosaic)
