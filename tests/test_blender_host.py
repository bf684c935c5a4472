"""The Blender loader, host side: the integer restatement of Pillow's Lanczos resize (tests/blender_reference.py)
against Pillow's stored bytes and, where Pillow is installed, against Pillow itself; ops.lanczos_tables against the restatement's tables;
the restated blend and rays against the reference's own BlenderDataset output (tests/golden/blender/reference.npz); load_blender's
ordering and checks with the kernels replaced by the restatement; argument errors of both entries; and the declarations.

Ray bound: the reference's fp32 chain rounds at most eight times on quantities no larger than the unit result, 8 x 2^-24 = 2^-21
absolute on a direction component; origins, near and far are copies and must be exact."""
import os

import numpy as np
import pytest
import torch

from tests import blender_reference as B

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
RAY_BOUND = 2.0 ** -21


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "blender", "reference.npz"), allow_pickle=False))


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("k", range(len(B.FIXTURE_SHAPES)))
def test_restatement_equals_the_stored_pillow_bytes(golden, k):
    h, w, oh, ow = B.FIXTURE_SHAPES[k]
    src, want = golden[f"resize{k}_src"], golden[f"resize{k}_out"]
    assert src.shape == (h, w, 4) and want.shape == (oh, ow, 4)
    assert _same_bits(src, B.random_rgba(h, w, seed=k))  # the stored input is the seeded one
    a = want[..., 3]
    assert (a == 0).any() and (a == 255).any() and ((a > 0) & (a < 255)).any()  # both un-premultiply branches
    assert _same_bits(B.resize_rgba(src, oh, ow), want)


@pytest.mark.parametrize("h,w,oh,ow", B.FIXTURE_SHAPES + [(800, 800, 400, 400), (20, 20, 20, 20), (1, 1, 2, 3)])
def test_restatement_equals_pillow_itself(h, w, oh, ow):
    Image = pytest.importorskip("PIL.Image")
    src = B.random_rgba(h, w, seed=7)
    want = np.asarray(Image.fromarray(src, "RGBA").resize((ow, oh), Image.LANCZOS))
    got = B.resize_rgba(src, oh, ow)
    assert _same_bits(got, want)
    if (h, w) == (oh, ow):
        assert _same_bits(got, src)  # a same-size resize is a copy: no premultiply round trip


@pytest.mark.parametrize("n_in,n_out", [(16, 8), (53, 17), (13, 26), (800, 400), (47, 47)])
def test_lanczos_tables_equal_the_restatement(n_in, n_out):
    from satnerf_amd import ops

    bounds, coef = ops.lanczos_tables(n_in, n_out)
    want_bounds, want_coef = B.tables(n_in, n_out)
    assert bounds.dtype == coef.dtype == np.int32 and _same_bits(bounds, want_bounds) and _same_bits(coef, want_coef)
    assert coef.shape[1] == 2 * int(np.ceil(3.0 * max(n_in / n_out, 1.0))) + 1
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= n_in).all() and (bounds[:, 1] <= coef.shape[1]).all()
    assert np.abs(coef.sum(1) - (1 << 22)).max() <= coef.shape[1]  # normalised: the rounded coefficients sum to 2^22 within a unit per tap
    assert ops.lanczos_tables(n_in, n_out)[1] is coef and not coef.flags.writeable  # cached
    with pytest.raises(ValueError):
        ops.lanczos_tables(0, 4)


def test_restated_blend_and_mask_equal_the_reference(golden):
    n = 64
    for t in range(golden["all_rgbs"].shape[0] // n):
        rgbs, _ = B.blend(B.resize_rgba(golden["images"][t], 8, 8))
        assert _same_bits(rgbs, golden["all_rgbs"][t * n:(t + 1) * n])
    rgbs, mask = B.blend(B.resize_rgba(golden["images"][4], 8, 8))
    assert _same_bits(rgbs, golden["val1_rgbs"]) and _same_bits(mask, golden["val1_valid_mask"])
    assert mask.any() and not mask.all()
    assert (golden["all_rgbs"] == 1.0).any() and (golden["all_rgbs"] < 1.0).any()


def _check_rays(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert _same_bits(got[:, [0, 1, 2, 6, 7]], want[:, [0, 1, 2, 6, 7]])
    err = np.abs(got[:, 3:6].astype(np.float64) - want[:, 3:6]).max()
    print(f"direction error {err:.3e} (bound {RAY_BOUND:.3e})")
    assert err <= RAY_BOUND


def test_restated_rays_agree_with_the_reference(golden):
    f = B.focal(float(golden["camera_angle_x"]), 8)
    assert f == float(golden["focal"])
    for t in range(3):
        rays = B.pinhole_rays(8, 8, f, f, 4.0, 4.0, golden["transform_matrix"][t][:3, :4], 2.0, 6.0)
        _check_rays(rays, golden["all_rays"][t * 64:(t + 1) * 64])
        assert np.abs(np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=1) - 1).max() < 1e-6
    _check_rays(B.pinhole_rays(8, 8, f, f, 4.0, 4.0, golden["transform_matrix"][4][:3, :4], 2.0, 6.0), golden["val1_rays"])
    assert _same_bits(golden["all_ts"], np.repeat(np.arange(3, dtype=np.float32), 64)) and not golden["val1_ts"].any()


def _scene(tmp_path, golden, n_val=None):
    images = {}
    B.write_scene(str(tmp_path), golden, images, n_val=n_val)
    return str(tmp_path), images.__getitem__


def test_load_blender_follows_the_reference_with_the_kernels_restated(tmp_path, monkeypatch, golden):
    from satnerf_amd import data, ops

    calls, ray_calls = [], []
    monkeypatch.setattr(ops, "blender_colors", B.blender_colors_stub(calls))
    monkeypatch.setattr(ops, "pinhole_rays", B.pinhole_rays_stub(ray_calls))
    root, reader = _scene(tmp_path, golden, n_val=11)
    rays, rgbs, ts = data.load_blender(root, "train", img_wh=(8, 8), device="cpu", reader=reader)
    assert _same_bits(rgbs.numpy(), golden["all_rgbs"])
    _check_rays(rays.numpy(), golden["all_rays"])
    assert ts.dtype == torch.int64 and _same_bits(ts.numpy(), golden["all_ts"].astype(np.int64))
    assert calls == [(16, 16, 8, 8, "hwc")] * 3 and ray_calls == [(8, 8, float(golden["focal"]), 4.0, 4.0)] * 3
    # a reader that returns CHW gives the same colours
    again = data.load_blender(root, "train", img_wh=(8, 8), device="cpu", reader=lambda p: np.transpose(reader(p), (2, 0, 1)))
    assert torch.equal(again[1], rgbs) and calls[-1] == (16, 16, 8, 8, "chw")
    val = data.load_blender(root, "val", img_wh=(8, 8), device="cpu", reader=reader)
    assert len(val) == 8  # the JSON lists 11 frames
    for v in val:
        assert sorted(v) == ["c2w", "rays", "rgbs", "ts", "valid_mask"]
        assert v["rays"].shape == (64, 8) and v["rgbs"].shape == (64, 3) and v["c2w"].shape == (3, 4)
        assert v["ts"].dtype == torch.int64 and v["ts"].shape == (64,) and not v["ts"].any() and v["valid_mask"].dtype == torch.bool
    v = val[1]
    assert _same_bits(v["rgbs"].numpy(), golden["val1_rgbs"]) and _same_bits(v["valid_mask"].numpy(), golden["val1_valid_mask"])
    assert _same_bits(v["c2w"].numpy(), golden["val1_c2w"])
    _check_rays(v["rays"].numpy(), golden["val1_rays"])
    # test_train reads transforms_train.json; frame idx != 0 keeps its index as ts
    tt = data.load_blender(root, "test_train", img_wh=(8, 8), device="cpu", reader=reader)
    assert [int(v["ts"][0]) for v in tt] == [0, 1, 2] and all((v["ts"] == v["ts"][0]).all() for v in tt)
    assert _same_bits(tt[2]["rgbs"].numpy(), golden["all_rgbs"][128:])


def test_load_blender_names_the_file_it_cannot_use(tmp_path, monkeypatch, golden):
    from satnerf_amd import data, ops

    monkeypatch.setattr(ops, "blender_colors", B.blender_colors_stub([]))
    monkeypatch.setattr(ops, "pinhole_rays", B.pinhole_rays_stub([]))
    root, reader = _scene(tmp_path, golden)
    with pytest.raises(ValueError, match=r"r_0\.png does not have exactly four bands"):
        data.load_blender(root, "train", img_wh=(8, 8), device="cpu", reader=lambda p: reader(p)[:, :, :3])
    with pytest.raises(ValueError, match=r"r_0\.png does not have exactly four bands"):
        data.load_blender(root, "train", img_wh=(8, 8), device="cpu", reader=lambda p: reader(p)[:, :, 0])
    with pytest.raises(ValueError, match=r"r_0\.png is not an 8-bit image"):
        data.load_blender(root, "val", img_wh=(8, 8), device="cpu", reader=lambda p: reader(p).astype(np.uint16) * 257)
    with pytest.raises(ValueError, match="img_wh must be square"):
        data.load_blender(root, "train", img_wh=(8, 6), device="cpu", reader=reader)
    # the layout must be readable off the shape: exactly one of the first and last axes is 4
    with pytest.raises(ValueError, match=r"r_0\.png has shape \(4, 16, 4\), which reads as"):
        data.load_blender(root, "train", img_wh=(8, 8), device="cpu", reader=lambda p: reader(p)[:4])
    with pytest.raises(ValueError, match=r"r_0\.png does not have exactly four bands"):
        data.load_blender(root, "train", img_wh=(8, 8), device="cpu", reader=lambda p: reader(p)[:5, :, :3])


def test_blender_colors_from_image_takes_host_arrays_and_tensors(monkeypatch):
    from satnerf_amd import data, ops

    calls = []
    monkeypatch.setattr(ops, "blender_colors", B.blender_colors_stub(calls))
    img = B.random_rgba(9, 13)
    img.setflags(write=False)  # as Pillow hands its pixels out
    want, want_mask = B.blend(B.resize_rgba(img, 5, 6))
    rgbs, mask = data.blender_colors_from_image(img, 5, 6, device="cpu", layout="hwc")
    assert _same_bits(rgbs.numpy(), want) and _same_bits(mask.numpy(), want_mask)
    rgbs, _ = data.blender_colors_from_image(torch.from_numpy(img.copy()).permute(2, 0, 1), 5, 6, device="cpu", layout="chw")
    assert _same_bits(rgbs.numpy(), want)
    out = torch.zeros(30, 3)
    assert data.blender_colors_from_image(img, 5, 6, device="cpu", out=out, layout="hwc")[0] is out and _same_bits(out.numpy(), want)
    with pytest.raises(ValueError, match="uint8"):
        data.blender_colors_from_image(img.astype(np.float32), 5, 6, device="cpu")


def _lib_built():
    from satnerf_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.lib()


def test_bad_arguments_of_blender_colors_are_refused_before_any_launch():
    """Host-side checks of sr_blender_colors: they return before anything touches a device, so this runs without one."""
    import ctypes as C

    lib = _lib_built()
    f = lib.sr_blender_colors
    err = lambda: lib.sr_last_error().decode()
    src, tab, out = 0x1000, 0x2000, 0x3000  # never dereferenced: every call below stops at a check

    def call(src=src, sh=16, sw=16, strides=(64, 4, 1), oh=8, ow=8, cw=tab, kw=13, ch=tab, kh=13, scratch=tab, nbytes=512, rgbs=out,
             mask=None, rgba=None, stages=0):
        return f(src, sh, sw, strides[0], strides[1], strides[2], oh, ow, cw, kw, ch, kh, scratch, nbytes, rgbs, mask, rgba, stages, None)

    assert call(sh=0) != 0 and "source sides" in err()
    assert call(sw=65537) != 0 and "source sides" in err()
    assert call(oh=-1) != 0 and "output sides" in err()
    assert call(strides=(64, 0, 1)) != 0 and "strides" in err()
    assert call(strides=(0, 4, 1)) != 0 and "strides" in err()
    assert call(src=None) != 0 and "null pointer" in err()
    assert call(rgbs=None) != 0 and "null pointer" in err()
    assert call(cw=None) != 0 and "null coefficient table for the horizontal" in err()
    assert call(ch=None) != 0 and "null coefficient table for the vertical" in err()
    assert call(kw=7) != 0 and "ksize 7 does not fit the resize 16 -> 8 (ksize 13)" in err()
    assert call(kh=15) != 0 and "ksize 15 does not fit the resize 16 -> 8 (ksize 13)" in err()
    assert call(sh=37, oh=11, kh=13) != 0 and "37 -> 11 (ksize 23)" in err()  # a table built for another pair of sizes
    assert call(nbytes=511) != 0 and "scratch holds 511 bytes, 512 are needed" in err()
    assert call(scratch=None) != 0 and "scratch" in err()
    assert call(scratch=0x2002) != 0 and "scratch" in err()
    assert call(rgba=0x3001) != 0 and "rgba must be 4-byte aligned" in err()
    assert call(stages=2) != 0 and "stages" in err()
    assert call(src=None, rgbs=None, cw=None, ch=None, scratch=None, oh=0) == 0  # an empty output: nothing to do, pointers or not
    assert call(src=None, rgbs=None, cw=None, ch=None, scratch=None, ow=0) == 0
    # the scratch query: the (src_h, out_w, 4) intermediate when both passes run, nothing otherwise
    n = C.c_int64(-1)
    q = lib.sr_blender_colors_scratch
    assert q(800, 800, 400, 400, C.byref(n)) == 0 and n.value == 4 * 800 * 400
    assert q(64, 64, 64, 32, C.byref(n)) == 0 and n.value == 0
    assert q(33, 47, 5, 47, C.byref(n)) == 0 and n.value == 0
    assert q(20, 20, 20, 20, C.byref(n)) == 0 and n.value == 0
    assert q(20, 20, 0, 7, C.byref(n)) == 0 and n.value == 0
    assert q(0, 20, 5, 7, C.byref(n)) != 0 and "source sides" in err()
    assert q(20, 20, 5, 7, None) != 0 and "null pointer" in err()


def test_bad_arguments_of_pinhole_rays_are_refused_before_any_launch():
    import ctypes as C

    lib = _lib_built()
    f = lib.sr_pinhole_rays
    err = lambda: lib.sr_last_error().decode()
    c2w = (C.c_float * 12)(*range(12))
    out = 0x1000
    assert f(-1, 8, 10.0, 10.0, 4.0, 4.0, c2w, 2.0, 6.0, out, None) != 0 and "grid" in err()
    assert f(8, 8, 10.0, 10.0, 4.0, 4.0, None, 2.0, 6.0, out, None) != 0 and "null c2w" in err()
    assert f(8, 8, 0.0, 10.0, 4.0, 4.0, c2w, 2.0, 6.0, out, None) != 0 and "fx and fy" in err()
    assert f(8, 8, 10.0, float("nan"), 4.0, 4.0, c2w, 2.0, 6.0, out, None) != 0 and "fx and fy" in err()
    assert f(8, 8, 10.0, 10.0, 4.0, 4.0, c2w, 2.0, 6.0, None, None) != 0 and "16-byte aligned" in err()
    assert f(8, 8, 10.0, 10.0, 4.0, 4.0, c2w, 2.0, 6.0, 0x1008, None) != 0 and "16-byte aligned" in err()
    assert f(0, 8, 10.0, 10.0, 4.0, 4.0, c2w, 2.0, 6.0, None, None) == 0  # an empty grid: nothing to do
    assert f(8, 0, 10.0, 10.0, 4.0, 4.0, c2w, 2.0, 6.0, None, None) == 0


def test_abi_declared_in_header_and_binding():
    import inspect

    from satnerf_amd import _lib, data, ops

    with open(os.path.join(REPO, "include", "satrender.h")) as f:
        header = " ".join(f.read().split())
    assert "int sr_blender_colors_scratch(int src_h, int src_w, int out_h, int out_w, int64_t* bytes);" in header
    assert ("int sr_blender_colors(const uint8_t* src, int src_h, int src_w, int64_t row_stride, int64_t pix_stride, int64_t chan_stride, "
            "int out_h, int out_w, const int32_t* coef_w, int ksize_w, const int32_t* coef_h, int ksize_h, void* scratch, "
            "int64_t scratch_bytes, float* rgbs, uint8_t* valid_mask, uint8_t* rgba, int stages, void* stream);") in header
    assert ("int sr_pinhole_rays(int h, int w, float fx, float fy, float cx, float cy, const float* c2w, float near, float far, float* out, "
            "void* stream);") in header
    assert "datasets/blender.py:12-209" in header and "MULDIV255" in header and "2^22" in header
    i, i64, vp, fl = _lib._i, _lib._i64, _lib._vp, _lib._f
    assert _lib.SIGNATURES["sr_blender_colors"] == (i, [vp, i, i, i64, i64, i64, i, i, vp, i, vp, i, vp, i64, vp, vp, vp, i, vp])
    res, args = _lib.SIGNATURES["sr_blender_colors_scratch"]
    assert res is i and args[:4] == [i, i, i, i] and len(args) == 5
    res, args = _lib.SIGNATURES["sr_pinhole_rays"]
    assert res is i and args[:6] == [i, i, fl, fl, fl, fl] and args[7:] == [fl, fl, vp, vp]
    assert list(inspect.signature(ops.lanczos_tables).parameters) == ["n_in", "n_out"]
    assert list(inspect.signature(ops.blender_colors_scratch).parameters) == ["src_h", "src_w", "out_h", "out_w"]
    assert list(inspect.signature(ops.blender_colors).parameters) == ["image_u8", "out_h", "out_w", "out", "layout", "want_rgba"]
    assert list(inspect.signature(ops.pinhole_rays).parameters) == ["h", "w", "fx", "fy", "cx", "cy", "c2w", "near", "far", "out"]
    assert list(inspect.signature(data.blender_colors_from_image).parameters)[:4] == ["image", "h", "w", "device"]
    assert list(inspect.signature(data.blender_rays).parameters)[:7] == ["h", "w", "focal", "c2w", "near", "far", "device"]
    assert list(inspect.signature(data.load_blender).parameters) == ["root_dir", "split", "img_wh", "device", "reader"]
