"""Evaluation image products on the GPU (csrc/image_products.hip through satnerf_amd.visualize / satnerf_amd.evaluate; DESIGN.md
section 7.10) against the numpy restatements of tests/image_products_reference.py, the recorded scipy output and the bytes recorded
from the reference's own functions (tests/golden/make_image_products_golden.py).  Every output is
defined in integers or in single rounded fp32 operations, so every comparison is bit equality."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import satnerf_oracle as O
from tests import image_products_reference as IP

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_products", "reference.npz")


def _vis():
    from satnerf_amd import visualize

    return visualize


def _bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def lut():
    return np.random.default_rng(77).integers(0, 256, (256, 3), dtype=np.uint8)  # a random table: every index tells


def _holes(rng, h, w, keep):
    img = rng.standard_normal((h, w)).astype(np.float32)
    img[rng.random((h, w)) >= keep] = np.nan
    return img


def _fill_cases(golden):
    rng = np.random.default_rng(21)
    corner = np.full((64, 48), np.nan, np.float32)
    corner[63, 0] = 2.5
    # longer than the 1024 pixels of a row one workgroup fills, than the 256 it takes per pass and than one 32-row mask word; valid at
    # the two ends only, so the row scan runs the whole width
    ends = np.full((3, 4133), np.nan, np.float32)
    ends[1, 0], ends[2, 4132] = -7.0, 9.0
    cross = np.full((3, 3), np.nan, np.float32)
    cross[0, 1], cross[1, 0], cross[1, 2], cross[2, 1] = 1, 2, 3, 4
    one_row, one_col = _holes(rng, 1, 40, 0.2), _holes(rng, 40, 1, 0.2)
    one_row[0, 7], one_col[33, 0] = 1.0, 2.0  # at least one valid pixel each
    return {"1x1": np.array([[3.25]], np.float32), "1x40": one_row, "40x1": one_col, "sparse": golden["sparse_image"],
            "dense": golden["dense_image"], "corner": corner, "ends": ends, "ends_T": np.ascontiguousarray(ends.T), "cross": cross,
            "two_tiles": _holes(rng, 70, 45, 0.03)}


@pytest.mark.parametrize("name", ["1x1", "1x40", "40x1", "sparse", "dense", "corner", "ends", "ends_T", "cross", "two_tiles"])
def test_fill_equals_the_brute_force_restatement(golden, name):
    img = _fill_cases(golden)[name]
    want, want_index, missing, _ = IP.brute_fill(img)
    got, index = _vis().fill_nans_nearest(_dev(img), return_index=True)
    assert got.dtype == torch.float32 and index.dtype == torch.int32 and tuple(got.shape) == tuple(index.shape) == img.shape
    assert np.array_equal(index.cpu().numpy(), want_index), name
    assert np.array_equal(_bits(got), _bits(want)), name
    assert np.array_equal(_bits(_vis().fill_nans_nearest(_dev(img))), _bits(want))  # without the index output
    if name == "cross":
        assert got[1, 1].item() == 1 and got[0, 0].item() == 1 and got[2, 2].item() == 3 and got[2, 0].item() == 2  # row, then column
    if name == "ends":
        assert len(missing) == 3 * 4133 - 2 and got[0, 2066].item() == -7.0 and got[0, 2067].item() == 9.0


def test_fill_leaves_valid_pixels_and_all_nan_images_alone():
    rng = np.random.default_rng(22)
    img = rng.standard_normal((33, 65)).astype(np.float32)
    img[0, 0], img[5, 5], img[32, 64], img[7, 1] = -0.0, np.inf, -np.inf, 0.0
    got, index = _vis().fill_nans_nearest(_dev(img), return_index=True)
    assert np.array_equal(_bits(got), _bits(img)) and np.array_equal(index.cpu().numpy().ravel(), np.arange(33 * 65))
    nan = np.full((9, 70), np.nan, np.float32)
    nan.view(np.uint32)[3, 4] = 0xffc12345  # a NaN with its own sign and payload: it comes back as it went in
    got, index = _vis().fill_nans_nearest(_dev(nan), return_index=True)
    assert np.array_equal(_bits(got), _bits(nan)) and (index == -1).all().item()
    empty = _vis().fill_nans_nearest(torch.empty(0, 5, device=DEV))
    assert tuple(empty.shape) == (0, 5)


def test_fill_reads_strided_views_in_place():
    from satnerf_amd import ops

    rng = np.random.default_rng(23)
    h, w = 21, 34
    buf = rng.standard_normal((h * w, 13)).astype(np.float32)
    buf[rng.random((h * w, 13)) < 0.7] = np.nan
    t = _dev(buf)
    column = t[:, 5].view(h, w)  # a column of the (N, 13) image buffer
    assert not column.is_contiguous() and column.data_ptr() == t.data_ptr() + 20
    want = _vis().fill_nans_nearest(column.contiguous(), return_index=True)
    got = _vis().fill_nans_nearest(column, return_index=True)
    assert torch.equal(got[1], want[1]) and np.array_equal(_bits(got[0]), _bits(want[0]))
    assert np.array_equal(_bits(got[0]), _bits(IP.brute_fill(buf[:, 5].reshape(h, w))[0]))
    flipped = column.t()  # (w, h), row stride 13, column stride 13 w
    assert np.array_equal(_bits(_vis().fill_nans_nearest(flipped)), _bits(IP.brute_fill(buf[:, 5].reshape(h, w).T)[0]))
    with pytest.raises(ValueError, match="overlap"):
        ops.nearest_fill(want[0], out=want[0])
    with pytest.raises(ValueError, match="overlap"):
        ops.nearest_fill(t[:, 5].view(h, w), out=t.view(-1)[: h * w].view(h, w))
    window = column[3:17, 6:29]
    assert np.array_equal(_bits(_vis().fill_nans_nearest(window)), _bits(IP.brute_fill(buf[:, 5].reshape(h, w)[3:17, 6:29])[0]))


@pytest.mark.parametrize("name", sorted(IP.FIXTURES))
def test_fill_against_the_recorded_scipy_output(golden, name):
    img = golden[name + "_image"]
    _, _, missing, sets = IP.brute_fill(img)
    got = _vis().fill_nans_nearest(_dev(img)).cpu().numpy()
    ambiguous = IP.check_against_scipy(img, golden[name + "_scipy"], got, missing, sets)  # membership everywhere, equality where unique
    print(f"{name}: scipy {golden['scipy_version']}, {100 * ambiguous:.1f} % of {len(missing)} filled pixels have several sources")
    if name == "sparse":
        assert ambiguous <= 0.20


def _check_colorize(x_dev, x_np, lut, nan_to_zero=False, vmin=None, vmax=None):
    """index, strip (at a column offset of a wider strip) and chw of one image against the restatement."""
    from satnerf_amd import ops

    want = IP.index_image(x_np, nan_to_zero, vmin, vmax)
    rows, cols = x_np.shape
    strip = torch.full((rows, cols + 5, 3), 7, dtype=torch.uint8, device=DEV)
    got = ops.colorize(x_dev, _dev(lut), nan_to_zero=nan_to_zero, vmin=vmin, vmax=vmax, want_index=True, strip=strip, strip_col0=2, want_chw=True)
    assert np.array_equal(got["index"].cpu().numpy(), want)
    s = strip.cpu().numpy()
    assert np.array_equal(s[:, 2:2 + cols], lut[want]) and (s[:, :2] == 7).all() and (s[:, 2 + cols:] == 7).all()
    assert np.array_equal(_bits(got["chw"]), _bits(IP.colors_chw(want, lut)))
    only = ops.colorize(x_dev, nan_to_zero=nan_to_zero, vmin=vmin, vmax=vmax, want_index=True)  # the index alone needs no table
    assert np.array_equal(only["index"].cpu().numpy(), want) and only["strip"] is None and only["chw"] is None
    return want


BOUNDS = [(None, None), (80.3, None), (None, 120.7), (80.3, 120.7)]  # narrower than the data below


@pytest.mark.parametrize("vmin,vmax", BOUNDS)
def test_colorize_equals_the_restatement(lut, vmin, vmax):
    rng = np.random.default_rng(31)
    for shape in ((5, 7), (37, 53), (40, 300)):
        x = (rng.standard_normal(shape) * 30 + 100).astype(np.float32)
        assert x.min() < 80.3 and x.max() > 120.7
        idx = _check_colorize(_dev(x), x, lut, vmin=vmin, vmax=vmax)
        assert idx.min() == 0 and idx.max() >= 253
    x = (rng.standard_normal((37, 53)) * 30 + 100).astype(np.float32)
    r0, r1, c0, c1 = _vis().crop_window(37, 53)
    _check_colorize(_dev(x)[r0:r1, c0:c1], x[r0:r1, c0:c1], lut, vmin=vmin, vmax=vmax)  # the crop window, read in place
    const = np.full((6, 9), 12.5, np.float32)
    _check_colorize(_dev(const), const, lut, vmin=vmin, vmax=vmax)


@pytest.mark.parametrize("tag", sorted(IP.BOUNDS))
def test_dsm_strip_gives_the_bytes_the_reference_returned(golden, tag):
    """hstack_dsm_tifs_v1's recorded output (crop, scipy fill of holes with one nearest neighbour per pixel, normalisation under numpy
    2; identity colour map) against dsm_strip with the identity table -- the kernels against the reference itself."""
    identity = _dev(np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1))
    for name in ("wide", "narrow", "large", "constant", "tiny"):  # tiny: where (ma - mi) + 1e-8f in fp32 and in fp64 give other bytes
        vmin, vmax = IP.recorded_bounds(name, tag)
        got = _vis().dsm_strip([_dev(golden["color_" + name])], identity, vmin=vmin, vmax=vmax).cpu().numpy()
        want = golden[f"color_{name}_{tag}"]
        assert got.shape == want.shape + (3,) and all(np.array_equal(got[:, :, k], want) for k in range(3)), name


def test_depth_and_unit_strips_give_the_bytes_the_reference_returned(golden):
    identity = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    for name in ("nan", "inf"):
        got = _vis().visualize_depth(_dev(golden["depth_" + name]), _dev(identity))
        assert np.array_equal(_bits(got), _bits(IP.colors_chw(golden[f"depth_{name}_index"], identity))), name
    units = [_dev(u) for u in IP.unit_images()]
    assert np.array_equal(_vis().sun_strip(units).cpu().numpy(), golden["unit_sun_strip"])
    assert np.array_equal(_vis().rgb_strip(units).cpu().numpy(), golden["unit_rgb_strip"])
    assert np.array_equal(_vis().rgb_strip(units[:1], crop=False).cpu().numpy(), golden["unit_rgb_strip_uncropped"])


@pytest.mark.parametrize("nan_to_zero", [False, True])
def test_colorize_nan_policies_and_buffer_columns(lut, nan_to_zero):
    rng = np.random.default_rng(32)
    h, w = 19, 23
    buf = (rng.random((h * w, 13)) * 40 + 3).astype(np.float32)
    buf[rng.random((h * w, 13)) < 0.1] = np.nan
    buf[40, 8] = np.inf
    t = _dev(buf)
    x_np = buf[:, 8].reshape(h, w)
    for vmin, vmax in ((None, None), (10.0, 30.0)):
        idx = _check_colorize(t[:, 8].view(h, w), x_np, lut, nan_to_zero=nan_to_zero, vmin=vmin, vmax=vmax)
        assert (idx[np.isnan(x_np)] == 0).all()  # nan_to_zero: NaN -> 0 = the minimum; kept: y is NaN -> index 0
    if nan_to_zero:
        got = _vis().visualize_depth(t[:, 8].view(h, w), _dev(lut))
        assert tuple(got.shape) == (3, h, w) and np.array_equal(_bits(got), _bits(IP.colors_chw(IP.index_image(x_np, True), lut)))
        neg = x_np.copy()
        neg[1, 40 // w + 1] = np.nan
        neg[np.isinf(neg)] = -np.inf  # -inf -> -FLT_MAX: the minimum
        _check_colorize(_dev(neg), neg, lut, nan_to_zero=True)


def test_strips_equal_the_restatement(lut):
    rng = np.random.default_rng(33)
    vis = _vis()
    shapes = ((37, 53), (37, 40), (36, 21))  # one cropped height (18), three widths
    dsms = []
    for k, (h, w) in enumerate(shapes):
        d = (rng.standard_normal((h, w)) * (5 + 20 * k) + 50 * k).astype(np.float32)  # three different ranges
        d[rng.random((h, w)) < 0.3] = np.nan
        dsms.append(d)
    for crop in (True, False):
        use = dsms if crop else [d[:30] for d in dsms]
        got = vis.dsm_strip([_dev(d) for d in use], _dev(lut), crop=crop)
        want = IP.dsm_strip(use, lut, crop)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want)
    got = vis.dsm_strip([_dev(d) for d in dsms], _dev(lut), vmin=10.0, vmax=60.0)
    assert np.array_equal(got.cpu().numpy(), IP.dsm_strip(dsms, lut, True, 10.0, 60.0))
    suns = [rng.random((h, w, 1)).astype(np.float32) for h, w in shapes]  # one channel
    suns[0][0:12, 0:20, 0] = [[0.0, 1.0, 1 / 255, 254.5 / 255] * 5] * 12
    rgbs = [rng.random((h, w, 3)).astype(np.float32) for h, w in shapes]  # three channels
    for crop in (True, False):
        s = vis.sun_strip([_dev(i) for i in (suns if crop else suns[:1])], crop=crop)
        want = IP.sun_strip(suns if crop else suns[:1], crop)
        assert s.dtype == torch.uint8 and tuple(s.shape) == want.shape and np.array_equal(s.cpu().numpy(), want)
        c = vis.rgb_strip([_dev(i) for i in (rgbs if crop else rgbs[:1])], crop=crop)
        want = IP.rgb_strip(rgbs if crop else rgbs[:1], crop)
        assert c.dtype == torch.uint8 and tuple(c.shape) == want.shape and np.array_equal(c.cpu().numpy(), want)
    buf = _dev(rng.random((37 * 53, 13)).astype(np.float32))  # columns of the image buffer, read in place
    assert np.array_equal(vis.rgb_strip([buf[:, 0:3].view(37, 53, 3)]).cpu().numpy(), IP.rgb_strip([buf[:, 0:3].cpu().numpy().reshape(37, 53, 3)]))
    assert np.array_equal(vis.sun_strip([buf[:, 5:6].view(37, 53, 1)]).cpu().numpy(), IP.sun_strip([buf[:, 5:6].cpu().numpy().reshape(37, 53, 1)]))
    with pytest.raises(ValueError, match="share their height"):
        vis.sun_strip([_dev(suns[0]), _dev(suns[0][:20])])
    with pytest.raises(ValueError, match="share their height"):
        vis.dsm_strip([_dev(dsms[0]), _dev(dsms[0][:20])], _dev(lut))


def _ecef(lat, lon, alt):
    a, e2 = 6378137.0, 6.69437999014e-3
    phi, lam = math.radians(lat), math.radians(lon)
    n = a / math.sqrt(1 - e2 * math.sin(phi) ** 2)
    return np.array([(n + alt) * math.cos(phi) * math.cos(lam), (n + alt) * math.cos(phi) * math.sin(lam), (n * (1 - e2) + alt) * math.sin(phi)])


def test_sun_sweep(lut):
    """The render has no perturb switch (it always jitters its stratified depths, from the RNG hook), so there is no perturb = 0 to
    set.  Every call here, direct or inside the sweep, replays the same recorded draws (noise_std = 0), so both sides sample the same
    depths; chunk = 128 splits the 16 x 12
    image into one full and one ragged chunk."""
    from satnerf_amd import evaluate, rendering
    from satnerf_amd.models import load_model

    h, w, n_interp = 16, 12, 3
    n = h * w
    args = O.default_args(n_samples=64, noise_std=0.0, chunk=128, mlp_mode="bf16x3")
    m = load_model(args)
    m.load_state_dict(O.procedural_satnerf_params(256, args.t_embbeding_tau, seed=1))
    emb = torch.nn.Embedding(args.t_embbeding_vocab, args.t_embbeding_tau)
    emb.load_state_dict({"weight": O.procedural_uniform((args.t_embbeding_vocab, args.t_embbeding_tau), 1.0, 7)})
    models = {"coarse": m.to(DEV).eval(), "t": emb.to(DEV)}
    rays, _ = O.synthetic_rays(n, seed=41)
    rays, ts = rays.to(DEV), torch.full((n,), 3, dtype=torch.int64, device=DEV)
    g = torch.Generator().manual_seed(42)
    per_call = []
    for size in (128, n - 128):
        per_call += [torch.rand(size, 64, generator=g).to(DEV), torch.zeros(size, 64, device=DEV)]
    center, scene_range = _ecef(30.3, -81.7, 0.0), 300.0

    def direction(el, az):
        el, az = np.radians(el), np.radians(az)
        flat = np.cos(el)  # the horizontal part, split east / north by the azimuth (clockwise from north)
        return np.array([flat * np.sin(az), flat * np.cos(az), np.sin(el)])

    upper, lower = direction(81.0, 140.0), direction(79.5, 170.0)  # incidence angles 9 .. 10.5: either side of 10
    with rendering.replay_rng(per_call * n_interp):
        res = evaluate.sun_interp(models, rays, ts, args, h, w, upper, lower, center, scene_range, n_interp=n_interp, lut=_dev(lut))
    want_dirs, want_angles = IP.sweep(upper, lower, n_interp)
    assert res["angles"] == want_angles and np.array_equal(res["sun_dirs"], want_dirs)
    assert want_angles[0] > 10 > want_angles[-1]
    order = IP.strip_order(want_angles)
    assert res["order"] == order and order != list(range(n_interp))  # "10.xx" sorts before "9.xx"
    host = []
    for k, sun_d in enumerate(want_dirs):
        direct = rays.clone()
        direct[:, 8:11] = torch.from_numpy(sun_d.astype(np.float32)).to(DEV)
        with torch.no_grad(), rendering.replay_rng(per_call):
            out = rendering.render_image_outputs(models, direct, ts, args)
        alts = rendering.latlonalt_from_depth(direct, out["depth"], center, scene_range)[2].float().view(h, w)
        for key in ("rgb", "depth", "acc", "sun", "albedo", "beta", "sky"):
            assert torch.equal(res["outputs"][k][key], out[key]), (k, key)
        assert torch.equal(res["alts"][k], alts)
        host.append({"sun": out["sun"].cpu().numpy().reshape(h, w, 1), "albedo": out["albedo"].cpu().numpy().reshape(h, w, 3),
                     "rgb": out["rgb"].cpu().numpy().reshape(h, w, 3), "alts": alts.cpu().numpy()})
    assert not torch.equal(res["outputs"][0]["sun"], res["outputs"][2]["sun"])  # the sun direction reaches the model

    def strips(layout):
        return {"sun": IP.sun_strip([host[k]["sun"] for k in layout]), "albedo": IP.rgb_strip([host[k]["albedo"] for k in layout]),
                "rgb": IP.rgb_strip([host[k]["rgb"] for k in layout]), "depth": IP.dsm_strip([host[k]["alts"] for k in layout], lut)}

    for key, want in strips(order).items():
        assert tuple(res["strips"][key].shape) == want.shape and np.array_equal(res["strips"][key].cpu().numpy(), want), key
    assert res["strips"]["sun"].shape == (8, 3 * 6) and res["strips"]["depth"].shape == (8, 3 * 6, 3)
    with rendering.replay_rng(per_call * n_interp):
        swept = evaluate.sun_interp(models, rays, ts, args, h, w, upper, lower, center, scene_range, n_interp=n_interp, order="sweep")
    assert swept["order"] == [0, 1, 2] and "depth" not in swept["strips"]
    for key, want in strips([0, 1, 2]).items():
        if key != "depth":
            assert np.array_equal(swept["strips"][key].cpu().numpy(), want), key
    with pytest.raises(ValueError):
        evaluate.sun_interp(models, rays, ts, args, h + 1, w, upper, lower, center, scene_range)
    with pytest.raises(ValueError, match="order"):
        evaluate.sun_interp(models, rays, ts, args, h, w, upper, lower, center, scene_range, order="sorted")
