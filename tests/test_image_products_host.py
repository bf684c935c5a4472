"""Evaluation image products, host side: the committed golden against scipy where it is installed, the
brute-force fill of tests/image_products_reference.py against scipy's griddata output under the two tie-aware checks, the index
restatement against the reference's own lines run under numpy, crop windows, the strip order, the sweep's host arithmetic, and the
new entries' error paths and declarations (none of which touches a device)."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest

from tests import image_products_reference as IP

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "image_products", "reference.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def fills(golden):
    """The brute-force fill of each fixture, computed once."""
    return {name: IP.brute_fill(golden[name + "_image"]) for name in IP.FIXTURES}


def test_golden_is_current_where_scipy_is_installed(golden):
    pytest.importorskip("scipy")
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_image_products_golden", os.path.join(HERE, "golden", "make_image_products_golden.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    fresh = maker.build_fill()  # the part that needs scipy alone; the bytes recorded from the reference are checked below
    assert set(fresh) <= set(golden)
    for name in IP.FIXTURES:
        assert np.array_equal(fresh[name + "_image"].view(np.uint32), golden[name + "_image"].view(np.uint32))
        # scipy's values on missing pixels may legitimately move between versions where several pixels are equidistant: membership is
        # what test_restatement_agrees_with_scipy holds them to; a fresh run on the recording version reproduces the file exactly
        if str(fresh["scipy_version"]) == str(golden["scipy_version"]):
            assert np.array_equal(fresh[name + "_scipy"].view(np.uint32), golden[name + "_scipy"].view(np.uint32))


@pytest.mark.parametrize("name", sorted(IP.FIXTURES))
def test_restatement_agrees_with_scipy(golden, fills, name):
    img = golden[name + "_image"]
    assert img.shape == (37, 53) and np.isnan(img[:3]).all() and np.isnan(img[:, -2:]).all() and np.isnan(img[12:21, 20:34]).all()
    filled, index, missing, sets = fills[name]
    assert len(missing) == int(np.isnan(img).sum()) and not np.isnan(filled).any()
    assert all(len(s) >= 1 for s in sets)  # no pixel is exempt from the membership check
    ambiguous = IP.check_against_scipy(img, golden[name + "_scipy"], filled, missing, sets)
    print(f"{name}: {len(missing)} filled pixels, {100 * ambiguous:.1f} % with several equidistant sources")
    if name == "sparse":
        assert ambiguous <= 0.20  # the fixture that carries the equality check
    # the index names the pixel whose bits were taken, at the least distance
    r, c = np.divmod(index, 53)
    assert np.array_equal(filled.view(np.uint32), img.view(np.uint32)[r, c])


def test_fill_restatement_breaks_ties_by_row_then_column():
    img = np.full((3, 3), np.nan, np.float32)
    img[0, 1], img[1, 0], img[1, 2], img[2, 1] = 1, 2, 3, 4  # four pixels at distance 1 from the centre
    filled, index, missing, sets = IP.brute_fill(img)
    assert filled[1, 1] == 1 and index[1, 1] == 1 and sets[missing.index((1, 1))] == {int(np.float32(v).view(np.uint32)) for v in (1, 2, 3, 4)}
    assert filled[0, 0] == 1 and filled[2, 2] == 3 and filled[2, 0] == 2  # (0,1) before (1,0); (1,2) before (2,1); (1,0) before (2,1)
    none = IP.brute_fill(np.full((2, 2), np.nan, np.float32))
    assert np.isnan(none[0]).all() and (none[1] == -1).all()


@pytest.mark.parametrize("tag", sorted(IP.BOUNDS))
def test_index_restatement_gives_the_bytes_the_reference_returned(golden, tag):
    """The reference's hstack_dsm_tifs_v1, run under numpy 2 with an identity colour map when the golden was recorded (crop, scipy fill
    of a hole with one nearest neighbour per pixel, normalisation), against fill + index of the restatement."""
    assert int(str(golden["numpy_version"]).split(".")[0]) >= 2  # NEP 50: a Python float stays weak beside an fp32 value
    for name in ("wide", "narrow", "large", "constant", "tiny"):
        img, want = golden["color_" + name], golden[f"color_{name}_{tag}"]
        filled = IP.brute_fill(IP.crop(img))[0]
        assert want.dtype == np.uint8 and want.shape == filled.shape
        assert np.array_equal(IP.index_image(filled, False, *IP.recorded_bounds(name, tag)), want), name
    assert golden["color_wide_" + tag].min() == 0 and golden["color_wide_" + tag].max() >= 254
    if tag == "measured":
        assert not golden["color_constant_measured"].any()  # a constant image: d = 1e-8f, every index 0
        # d = fp32(fp32(ma - mi) + 1e-8f), not the fp64 sum: the two differ on this image
        x = IP.crop(golden["color_tiny"])
        fp64_sum = (np.float32(255) * ((x - x.min()) / np.float32(float(x.max()) - float(x.min()) + 1e-8))).astype(np.uint8)
        assert not np.array_equal(fp64_sum, golden["color_tiny_measured"])


def test_depth_index_restatement_gives_the_bytes_visualize_depth_returned(golden):
    for name in ("nan", "inf"):  # np.nan_to_num: NaN -> 0, +inf -> FLT_MAX
        assert np.array_equal(IP.index_image(golden["depth_" + name], True), golden[f"depth_{name}_index"])
    assert golden["depth_inf_index"][4, 4] >= 254 and golden["depth_inf_index"][2, 3] == 0


def test_strip_restatements_give_the_bytes_the_reference_returned(golden):
    units = IP.unit_images()
    assert golden["unit_sun_strip"].shape == (18, 56) and golden["unit_rgb_strip"].shape == (18, 56, 3)
    assert np.array_equal(IP.sun_strip(units), golden["unit_sun_strip"])
    assert np.array_equal(IP.rgb_strip(units), golden["unit_rgb_strip"])
    assert np.array_equal(IP.rgb_strip(units[:1], False), golden["unit_rgb_strip_uncropped"])
    assert {0, 1, 254, 255} <= set(golden["unit_sun_strip"].ravel().tolist())  # 0, 1 / 255, 254.5 / 255 and 1 are in the window


def test_crop_windows_for_odd_sizes():
    from satnerf_amd import visualize

    for h, w in ((1, 1), (2, 3), (5, 7), (37, 53), (800, 800), (801, 799), (3, 8191)):
        r0, r1, c0, c1 = visualize.crop_window(h, w)
        assert (r0, r1, c0, c1) == IP.crop_window(h, w) == (h // 4, 3 * h // 4, w // 4, 3 * w // 4)
        assert 0 <= r0 <= r1 <= h and 0 <= c0 <= c1 <= w
    assert visualize.crop_window(37, 53) == (9, 27, 13, 39) and visualize.crop_window(5, 7) == (1, 3, 1, 5)
    assert visualize.crop_window(1, 1) == (0, 0, 0, 0)


def test_strip_order_is_a_string_sort_of_the_file_names():
    from satnerf_amd import evaluate

    angles = [9.5, 10.2, 25.0, 7.25, 100.0, 10.196]
    order = evaluate.reference_strip_order(angles)
    assert order == IP.strip_order(angles) == [1, 5, 4, 2, 3, 0]  # "10.20" twice in sweep order, "100.00" ('.' sorts before '0'), "25.00", ..
    assert order.index(1) < order.index(0)  # 10.20 before 9.50
    assert evaluate.reference_strip_order([3.0, 2.0, 1.0]) == [2, 1, 0]
    assert evaluate.reference_strip_order([]) == []


def test_sweep_host_arithmetic(tmp_path):
    from satnerf_amd import evaluate

    suns = {"a": (60.0, 150.0), "b": (35.5, 170.25), "c": (72.25, 140.0), "d": (50.0, 10.0)}  # elevation, azimuth in degrees
    for name, (el, az) in suns.items():
        with open(tmp_path / (name + ".json"), "w") as f:
            json.dump({"sun_elevation": str(el) if name == "a" else el, "sun_azimuth": az, "img": name + ".tif"}, f)
    (tmp_path / "notes.txt").write_text("not a json")
    upper, lower = evaluate.sun_direction_bounds(str(tmp_path))

    def direction(el, az):
        el, az = np.radians(el), np.radians(az)
        flat = np.cos(el)  # the horizontal part, split east / north by the azimuth (clockwise from north)
        return np.array([flat * np.sin(az), flat * np.cos(az), np.sin(el)])

    assert np.array_equal(upper, direction(*suns["c"])) and np.array_equal(lower, direction(*suns["b"]))  # incidence = 90 - elevation
    assert abs(evaluate.solar_incidence_angle(upper) - (90 - 72.25)) < 1e-9
    assert evaluate.solar_incidence_angle(upper) == IP.incidence_angle(upper)
    dirs, angles = evaluate.interpolated_sun_directions(upper, lower)
    want_dirs, want_angles = IP.sweep(upper, lower, 10)
    assert dirs.dtype == np.float64 and dirs.shape == (10, 3) and np.array_equal(dirs, want_dirs) and angles == want_angles
    assert np.array_equal(dirs[0], lower) and np.array_equal(dirs[-1], upper)  # alpha = 0 is the tilted sun
    assert np.linalg.norm(dirs[5]) < 1 - 1e-4  # not normalised
    assert angles == sorted(angles, reverse=True)
    with pytest.raises(ValueError, match="json"):
        evaluate.sun_direction_bounds(str(tmp_path / "empty"))
    with pytest.raises(ValueError, match="n_interp"):
        evaluate.interpolated_sun_directions(upper, lower, 0)


def test_cpu_tensors_are_refused():
    import torch

    from satnerf_amd import visualize

    img, lut = torch.zeros(8, 8), torch.zeros(256, 3, dtype=torch.uint8)
    for call in (lambda: visualize.fill_nans_nearest(img), lambda: visualize.visualize_depth(img, lut), lambda: visualize.dsm_strip([img], lut),
                 lambda: visualize.sun_strip([img]), lambda: visualize.rgb_strip([torch.zeros(8, 8, 3)])):
        with pytest.raises(ValueError, match="GPU"):
            call()
    with pytest.raises(ValueError, match="at least one"):
        visualize.sun_strip([])


def _lib_handle():
    from satnerf_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.lib()


def test_bad_arguments_are_refused_before_any_launch():
    """Every call below stops at a host-side check (or at an empty image), so the made-up pointers are never dereferenced."""
    lib = _lib_handle()
    err = lambda: lib.sr_last_error().decode()
    img, out, scr, lut = 0x1000, 0x2000, 0x3000, 0x4000
    nbytes = ctypes.c_int64(-1)
    assert lib.sr_nearest_fill_scratch(37, 53, ctypes.byref(nbytes)) == 0 and nbytes.value >= 2 * 37 * 53
    need = nbytes.value
    assert lib.sr_nearest_fill_scratch(0, 53, ctypes.byref(nbytes)) == 0 and nbytes.value == 0
    assert lib.sr_nearest_fill_scratch(8193, 53, ctypes.byref(nbytes)) != 0 and "0..8192" in err()
    assert lib.sr_nearest_fill_scratch(37, 53, None) != 0 and "null pointer" in err()
    f = lib.sr_nearest_fill
    assert f(img, 37, 8193, 53, 1, scr, need, out, None, None) != 0 and "0..8192" in err()
    assert f(img, -1, 53, 53, 1, scr, need, out, None, None) != 0 and "0..8192" in err()
    assert f(img, 37, 53, 0, 1, scr, need, out, None, None) != 0 and "strides" in err()
    assert f(img, 37, 53, 53, -13, scr, need, out, None, None) != 0 and "strides" in err()
    assert f(None, 37, 53, 53, 1, scr, need, out, None, None) != 0 and "null pointer" in err()
    assert f(img, 37, 53, 53, 1, scr, need, None, None, None) != 0 and "null pointer" in err()
    assert f(img, 37, 53, 53, 1, None, need, out, None, None) != 0 and "null pointer" in err()
    assert f(img, 37, 53, 53, 1, scr + 1, need, out, None, None) != 0 and "aligned" in err()
    assert f(img, 37, 53, 53, 1, scr, need - 1, out, None, None) != 0 and "scratch holds" in err()
    assert f(None, 0, 53, 53, 1, None, 0, None, None, None) == 0 and f(None, 37, 0, 1, 1, None, 0, None, None, None) == 0  # empty: nothing to do

    assert lib.sr_colorize_scratch(0, ctypes.byref(nbytes)) == 0 and nbytes.value == 8
    assert lib.sr_colorize_scratch(3, ctypes.byref(nbytes)) == 0 and nbytes.value == 0
    assert lib.sr_colorize_scratch(4, ctypes.byref(nbytes)) != 0 and "bounds" in err()
    g = lib.sr_colorize
    ok = dict(image=img, rows=5, cols=7, rs=7, cs=1, nz=0, bounds=0, vmin=0.0, vmax=0.0, denom=0.0, lut=lut, index=out, strip=None, scols=0,
              scol0=0, chw=None, scratch=scr, sbytes=8, stream=None)

    def colorize(**kw):
        return g(*{**ok, **kw}.values())

    assert colorize(rows=-1) != 0 and "window" in err()
    assert colorize(cols=65536) != 0 and "window" in err()
    assert colorize(cs=0) != 0 and "strides" in err()
    assert colorize(nz=2) != 0 and "nan_to_zero" in err()
    assert colorize(bounds=4) != 0 and "bounds" in err()
    assert colorize(bounds=1, vmin=float("nan")) != 0 and "vmin" in err()
    assert colorize(bounds=2, vmax=float("nan")) != 0 and "vmax" in err()
    assert colorize(index=None) != 0 and "no output" in err()
    assert colorize(lut=None, chw=out) != 0 and "lut" in err()
    assert colorize(strip=out, scols=10, scol0=4) != 0 and "do not fit" in err()
    assert colorize(strip=out, scols=10, scol0=-1) != 0 and "do not fit" in err()
    assert colorize(image=None) != 0 and "null pointer" in err()
    assert colorize(scratch=None) != 0 and "scratch" in err()
    assert colorize(scratch=scr + 2) != 0 and "aligned" in err()
    assert colorize(sbytes=4) != 0 and "scratch holds" in err()
    assert colorize(rows=0, image=None, scratch=None, sbytes=0) == 0 and colorize(cols=0, image=None) == 0

    u = lib.sr_unit_to_u8
    assert u(img, 5, 7, 2, 21, 3, 1, out, 7, 0, None) != 0 and "channels" in err()
    assert u(img, 5, 7, 3, 21, 3, 0, out, 7, 0, None) != 0 and "channel stride" in err()
    assert u(img, 5, 70000, 3, 21, 3, 1, out, 70000, 0, None) != 0 and "window" in err()
    assert u(img, 5, 7, 3, 21, 0, 1, out, 7, 0, None) != 0 and "strides" in err()
    assert u(img, 5, 7, 3, 21, 3, 1, out, 7, 1, None) != 0 and "do not fit" in err()
    assert u(None, 5, 7, 3, 21, 3, 1, out, 7, 0, None) != 0 and "null pointer" in err()
    assert u(img, 5, 7, 3, 21, 3, 1, None, 7, 0, None) != 0 and "null pointer" in err()
    assert u(None, 0, 7, 3, 21, 3, 1, None, 7, 0, None) == 0 and u(None, 5, 0, 1, 1, 1, 1, None, 0, 0, None) == 0


def test_abi_declared_in_header_and_binding():
    from satnerf_amd import _lib, evaluate, ops, visualize

    with open(os.path.join(REPO, "include", "satrender.h")) as f:
        header = " ".join(f.read().split())
    for decl in ("int sr_nearest_fill_scratch(int h, int w, int64_t* bytes);",
                 "int sr_nearest_fill(const float* image, int h, int w, int64_t row_stride, int64_t col_stride, void* scratch, "
                 "int64_t scratch_bytes, float* out, int32_t* index, void* stream);",
                 "int sr_colorize_scratch(int bounds, int64_t* bytes);",
                 "int sr_unit_to_u8(const float* image, int rows, int cols, int channels, int64_t row_stride, int64_t col_stride, "
                 "int64_t chan_stride, uint8_t* strip, int64_t strip_cols, int64_t strip_col0, void* stream);"):
        assert decl in header, decl
    for said in ("scipy raises there", "numpy's cast is undefined", "infinite y gives index 0", "study_solar_interpolation.py:53-68"):
        assert said in header, said
    v, i, i64, f32 = _lib._vp, _lib._i, _lib._i64, _lib._f
    assert _lib.SIGNATURES["sr_nearest_fill"] == (i, [v, i, i, i64, i64, v, i64, v, v, v])
    assert _lib.SIGNATURES["sr_colorize"] == (i, [v, i, i, i64, i64, i, i, f32, f32, f32, v, v, v, i64, i64, v, v, i64, v])
    assert _lib.SIGNATURES["sr_unit_to_u8"] == (i, [v, i, i, i, i64, i64, i64, v, i64, i64, v])
    assert list(inspect.signature(visualize.fill_nans_nearest).parameters) == ["image", "return_index"]
    assert list(inspect.signature(visualize.visualize_depth).parameters) == ["depth", "lut"]
    assert list(inspect.signature(visualize.dsm_strip).parameters) == ["images", "lut", "crop", "vmin", "vmax"]
    assert list(inspect.signature(visualize.sun_strip).parameters) == ["images", "crop"]
    assert list(inspect.signature(visualize.rgb_strip).parameters) == ["images", "crop"]
    assert list(inspect.signature(evaluate.sun_interp).parameters) == ["models", "rays", "ts", "args", "h", "w", "upper", "lower", "center",
                                                                       "scene_range", "n_interp", "lut", "order"]
    assert ops.colorize_denominator(80.3, 120.7) == float(np.float32(120.7 - 80.3 + 1e-8))


def test_lut_from_matplotlib_is_matplotlibs_table():
    matplotlib = pytest.importorskip("matplotlib")
    from satnerf_amd import visualize

    table = visualize.lut_from_matplotlib("viridis", device="cpu")
    assert table.dtype.is_floating_point is False and tuple(table.shape) == (256, 3)
    want = (np.asarray(matplotlib.colormaps["viridis"].colors) * 255).astype(np.uint8)  # bytes=True truncates x * 255
    assert np.abs(table.numpy().astype(int) - want.astype(int)).max() <= 1
    assert "not OpenCV's" in visualize.lut_from_matplotlib.__doc__
