"""NeRF-W's perturbations of a Blender scene, host side: the numpy restatement (tests/blender_perturb_reference.py)
against what the reference's own ``add_perturbation`` gave (tests/golden/blender_perturb/reference.npz: hashes of whole images, crops at
the strip's corners, pixel counts); ``data.blender_perturbation`` against the parameters the reference drew; ``load_blender_perturbed``
against the reference's ``BlenderDataset(..., perturbation=...)`` with the kernels replaced by the restatements; the argument checks of
``sr_blender_perturb``; and the declarations.

Every comparison of bytes and colours is bit equality.  Ray directions keep the sibling file's bound against the reference's fp32
chain, 2^-21 absolute (tests/test_blender_host.py); origins, near and far are exact."""
import os

import numpy as np
import pytest
import torch

from tests import blender_perturb_reference as P
from tests import blender_reference as B

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
RAY_BOUND = 2.0 ** -21
WH = P.SCENE_WH
N = WH * WH


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "blender_perturb", "reference.npz"), allow_pickle=False))


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_input_formula_covers_every_byte_and_both_alpha_runs():
    for (h, w), frame in zip(P.SIZES, P.SEEDS):
        img = P.pattern_rgba(h, w, frame)
        assert img.shape == (h, w, 4) and img.dtype == np.uint8
        assert all(len(np.unique(img[..., k])) == 256 for k in range(4))
        blocks = img[:h // 32 * 32, :w // 32 * 32, 3].reshape(h // 32, 32, w // 32, 32)
        assert (blocks == 0).all((1, 3)).any() and (blocks == 255).all((1, 3)).any()


@pytest.mark.parametrize("i", range(len(P.SIZES)))
def test_restatement_equals_the_reference(golden, i):
    h, w = P.SIZES[i]
    for j, seed in enumerate(P.SEEDS):
        src = P.pattern_rgba(h, w, frame=seed)
        assert _same_bits(P.sha256(src), golden["hash_in"][i, j])
        for k, variant in enumerate(P.VARIANTS):
            got = P.perturbed(src, seed, variant)
            assert (got != src).any(-1).sum() == golden["touched"][i, j, k], (h, w, seed, variant)
            assert _same_bits(P.crops(got, int(golden["left"][j]), int(golden["top"][j])), golden["crops"][i, j, k]), (h, w, seed, variant)
            assert _same_bits(P.sha256(got), golden["hash_out"][i, j, k]), (h, w, seed, variant)


def test_fixture_covers_what_the_cases_are_for(golden):
    occ = P.VARIANTS.index(("occ",))
    t = golden["touched"][:, :, occ]
    sizes = {s: i for i, s in enumerate(P.SIZES)}
    assert (t[sizes[(416, 416)]] > 0).all() and (t[sizes[(416, 416)]] < 201 * 201).all()  # every strip drawn, and clipped
    assert [int(v > 0) for v in t[sizes[(333, 417)]]] == [0, 1, 0, 0, 1]  # seeds 2 and 99 draw, the others lie below the image
    assert not t[sizes[(100, 120)]].any()  # everything outside
    assert t[sizes[(800, 800)], P.SEEDS.index(3)] == 201 * 201  # the whole strip
    # the shared column of rectangles 0 and 1 shows rectangle 1's colour: the later one wins
    i, j = sizes[(800, 800)], P.SEEDS.index(3)
    crop = golden["crops"][i, j, occ, 4]
    assert _same_bits(crop[P.CROP // 2, P.CROP // 2, :3], golden["colours"][j, 1]) and crop[P.CROP // 2, P.CROP // 2, 3] == 255
    assert _same_bits(crop[P.CROP // 2, P.CROP // 2 - 1, :3], golden["colours"][j, 0])


@pytest.mark.parametrize("j", range(len(P.SEEDS)))
def test_blender_perturbation_returns_what_the_reference_draws(golden, j):
    from satnerf_amd import data

    seed = P.SEEDS[j]
    want_lut = P.color_lut(golden["s"][j], golden["b"][j])
    want_rects, want_fills = P.occluders(int(golden["left"][j]), int(golden["top"][j]), golden["colours"][j])
    np.random.seed(12345)
    before = np.random.get_state()
    lut, rects, fills = data.blender_perturbation(seed, ["color", "occ"])
    after = np.random.get_state()
    assert before[0] == after[0] and _same_bits(before[1], after[1]) and before[2:] == after[2:]  # the global generator is left alone
    assert lut.dtype == np.uint8 and _same_bits(lut, want_lut) and lut.flags.c_contiguous
    assert _same_bits(lut[3], np.arange(256, dtype=np.uint8))  # alpha: the identity
    assert rects.dtype == np.int32 and _same_bits(rects, want_rects) and fills.dtype == np.uint8 and _same_bits(fills, want_fills)
    assert (fills[:, 3] == 255).all()
    lut, rects, fills = data.blender_perturbation(seed, ["color"])
    assert _same_bits(lut, want_lut) and rects is None and fills is None
    lut, rects, fills = data.blender_perturbation(seed, ("occ",))
    assert lut is None and _same_bits(rects, want_rects) and _same_bits(fills, want_fills)
    assert data.blender_perturbation(seed, []) == (None, None, None)
    # the restatement's own draws are the stored ones too
    p = P.params(seed)
    assert _same_bits(p["s"], golden["s"][j]) and _same_bits(p["b"], golden["b"][j]) and _same_bits(p["colours"], golden["colours"][j])
    assert (p["left"], p["top"]) == (int(golden["left"][j]), int(golden["top"][j]))


def test_an_unknown_perturbation_is_refused(tmp_path):
    from satnerf_amd import data

    for bad in (["blur"], ["color", "noise"], "color"):
        with pytest.raises(ValueError, match='Only "color" and "occ" perturbations are supported!'):
            data.blender_perturbation(1, bad)
    with pytest.raises(ValueError, match='Only "color" and "occ" perturbations are supported!'):
        data.load_blender_perturbed(str(tmp_path), ["occ", "rain"], device="cpu")  # before any file is looked for


def _check_rays(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert _same_bits(got[:, [0, 1, 2, 6, 7]], want[:, [0, 1, 2, 6, 7]])
    err = np.abs(got[:, 3:6].astype(np.float64) - want[:, 3:6]).max()
    print(f"direction error {err:.3e} (bound {RAY_BOUND:.3e})")
    assert err <= RAY_BOUND


@pytest.fixture
def stubbed(tmp_path, monkeypatch, golden):
    """The fixture scene on disk, its reader, and the three kernels replaced by their restatements; ``calls`` records the
    perturbation calls."""
    from satnerf_amd import ops

    calls = []
    monkeypatch.setattr(ops, "blender_colors", B.blender_colors_stub([]))
    monkeypatch.setattr(ops, "pinhole_rays", B.pinhole_rays_stub([]))
    monkeypatch.setattr(ops, "blender_perturb", P.blender_perturb_stub(calls))
    images = {}
    P.write_scene(str(tmp_path), golden, images)
    return str(tmp_path), images.__getitem__, calls


@pytest.mark.parametrize("variant", P.VARIANTS, ids="+".join)
def test_load_blender_perturbed_follows_the_reference_with_the_kernels_restated(stubbed, golden, variant):
    from satnerf_amd import data

    root, reader, calls = stubbed
    v = "+".join(variant)
    clean = data.load_blender(root, "train", img_wh=(WH, WH), device="cpu", reader=reader)
    assert calls == []  # load_blender perturbs nothing
    rays, rgbs, ts = data.load_blender_perturbed(root, list(variant), "train", img_wh=(WH, WH), device="cpu", reader=reader)
    assert calls == [("hwc", "color" in variant, 10 if "occ" in variant else 0, False)] * (P.SCENE_TRAIN - 1)  # every frame but the first
    assert _same_bits(rgbs.numpy(), golden[f"{v}_all_rgbs"])
    assert torch.equal(rgbs[:N], clean[1][:N]) and not torch.equal(rgbs[N:2 * N], clean[1][N:2 * N])  # frame 0 is unperturbed
    assert torch.equal(rays, clean[0])
    assert ts.dtype == torch.int64 and _same_bits(ts.numpy(), golden[f"{v}_all_ts"].astype(np.int64))
    assert _same_bits(ts.numpy(), np.repeat(np.arange(P.SCENE_TRAIN), N))
    # a reader that returns CHW gives the same colours
    again = data.load_blender_perturbed(root, variant, "train", img_wh=(WH, WH), device="cpu", reader=lambda p: np.transpose(reader(p), (2, 0, 1)))
    assert torch.equal(again[1], rgbs) and calls[-1][0] == "chw"
    # test_train: frame idx != 0 is perturbed with seed idx and keeps idx as ts; every dict carries the unperturbed image too
    del calls[:]
    tt = data.load_blender_perturbed(root, list(variant), "test_train", img_wh=(WH, WH), device="cpu", reader=reader)
    assert len(tt) == P.SCENE_TRAIN and len(calls) == P.SCENE_TRAIN - 1
    for d in tt:
        assert sorted(d) == list(golden["test_train0_keys_perturbed"])
    assert [int(d["ts"][0]) for d in tt] == list(range(P.SCENE_TRAIN)) and all((d["ts"] == d["ts"][0]).all() for d in tt)
    d = tt[2]
    assert _same_bits(d["rgbs"].numpy(), golden[f"{v}_tt2_rgbs"]) and _same_bits(d["valid_mask"].numpy(), golden[f"{v}_tt2_valid_mask"])
    assert _same_bits(d["original_rgbs"].numpy(), golden["tt2_original_rgbs"])
    assert _same_bits(d["original_valid_mask"].numpy(), golden["tt2_original_valid_mask"])
    assert _same_bits(d["ts"].numpy(), golden["tt2_ts"]) and _same_bits(d["c2w"].numpy(), golden["tt2_c2w"])
    _check_rays(d["rays"].numpy(), golden["tt2_rays"])
    assert _same_bits(d["rgbs"].numpy(), rgbs[2 * N:3 * N].numpy())  # the training set's frame 2
    assert torch.equal(d["original_rgbs"], clean[1][2 * N:3 * N]) and not torch.equal(d["original_rgbs"], d["rgbs"])
    assert torch.equal(tt[0]["original_rgbs"], tt[0]["rgbs"]) and torch.equal(tt[0]["original_valid_mask"], tt[0]["valid_mask"])
    assert tt[0]["original_rgbs"].data_ptr() != tt[0]["rgbs"].data_ptr()
    if "occ" in variant:  # the occluders are opaque: pixels that were transparent become valid
        assert (d["valid_mask"] & ~d["original_valid_mask"]).any()
    else:
        assert torch.equal(d["valid_mask"], d["original_valid_mask"])


def test_val_and_the_empty_perturbation_are_load_blender(stubbed, golden):
    from satnerf_amd import data

    root, reader, calls = stubbed

    def same(a, b):
        if isinstance(a, tuple):
            return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
        return len(a) == len(b) and all(sorted(x) == sorted(y) and all(torch.equal(x[k], y[k]) for k in x) for x, y in zip(a, b))

    for split in ("train", "val", "test_train"):
        want = data.load_blender(root, split, img_wh=(WH, WH), device="cpu", reader=reader)
        for perturbation in ((), []):
            assert same(data.load_blender_perturbed(root, perturbation, split, img_wh=(WH, WH), device="cpu", reader=reader), want)
    assert sorted(want[0]) == list(golden["test_train0_keys_clean"])  # no extras without a perturbation
    want = data.load_blender(root, "val", img_wh=(WH, WH), device="cpu", reader=reader)
    assert same(data.load_blender_perturbed(root, ["color", "occ"], "val", img_wh=(WH, WH), device="cpu", reader=reader), want)
    assert calls == []  # nothing above perturbs


def test_blender_colors_from_image_perturbs_a_copy(monkeypatch):
    from satnerf_amd import data, ops

    calls = []
    monkeypatch.setattr(ops, "blender_colors", B.blender_colors_stub([]))
    monkeypatch.setattr(ops, "blender_perturb", P.blender_perturb_stub(calls))
    img = P.pattern_rgba(64, 48, frame=2)
    keep = img.copy()
    rects, fills = np.array([[5, 7, 30, 40]], np.int32), np.array([[1, 2, 3, 255]], np.uint8)
    want, want_mask = B.blend(B.resize_rgba(P.perturb(img, None, rects, fills), 16, 12))
    rgbs, mask = data.blender_colors_from_image(img, 16, 12, device="cpu", layout="hwc", perturb=(None, rects, fills))
    assert _same_bits(rgbs.numpy(), want) and _same_bits(mask.numpy(), want_mask)
    assert _same_bits(img, keep) and calls == [("hwc", False, 1, False)]  # the caller's bytes are as they were
    rgbs, _ = data.blender_colors_from_image(img, 16, 12, device="cpu", layout="hwc", perturb=(None, None, None))
    assert len(calls) == 1 and _same_bits(rgbs.numpy(), B.blend(B.resize_rgba(img, 16, 12))[0])


def _lib_built():
    from satnerf_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.lib()


def test_bad_arguments_of_blender_perturb_are_refused_before_any_launch():
    """Host-side checks of sr_blender_perturb: they return before anything touches a device, so this runs without one."""
    import ctypes as C

    lib = _lib_built()
    f = lib.sr_blender_perturb
    err = lambda: lib.sr_last_error().decode()
    img, other = 0x10000, 0x80000  # never dereferenced: every call below stops at a check
    lut = (C.c_uint8 * 1024)()
    rects, fills = (C.c_int32 * 64)(), (C.c_uint8 * 64)()
    as_p = lambda a: a if a is None or isinstance(a, int) else C.addressof(a)

    def call(src=img, dst=img, h=16, w=16, strides=(64, 4, 1), lut=lut, rects=rects, fills=fills, n=10):
        return f(src, dst, h, w, strides[0], strides[1], strides[2], as_p(lut), as_p(rects), as_p(fills), n, None)

    assert call(src=None) != 0 and "null image" in err()
    assert call(dst=None) != 0 and "null image" in err()
    assert call(h=0) != 0 and "sides must lie in 1..65536 (got 0 x 16)" in err()
    assert call(w=65537) != 0 and "sides must lie in 1..65536 (got 16 x 65537)" in err()
    assert call(strides=(0, 4, 1)) != 0 and "strides must be positive byte counts up to 2^40 (got row 0, pixel 4, channel 1)" in err()
    assert call(strides=(2 ** 40 + 1, 4, 1)) != 0 and "strides must be positive" in err()
    assert call(strides=(64, 4, 2 ** 62)) != 0 and "strides must be positive" in err()
    assert call(strides=(64, -4, 1)) != 0 and "pixel -4" in err()
    assert call(strides=(16, 1, 0)) != 0 and "channel 0" in err()
    assert call(n=-1) != 0 and "n_rects must lie in 0..16 (got -1)" in err()
    assert call(n=17) != 0 and "n_rects must lie in 0..16 (got 17)" in err()
    assert call(rects=None) != 0 and "null rects or fills with n_rects = 10" in err()
    assert call(fills=None, n=1) != 0 and "null rects or fills with n_rects = 1" in err()
    assert call(dst=img + 512) != 0 and "dst must be src itself or not overlap it (the image spans 1024 bytes)" in err()
    assert call(src=other, dst=other - 1023) != 0 and "overlap" in err()


def test_abi_declared_in_header_and_binding():
    import inspect

    from satnerf_amd import _lib, data, ops

    with open(os.path.join(REPO, "include", "satrender.h")) as f:
        header = " ".join(f.read().split())
    assert ("int sr_blender_perturb(const uint8_t* src, uint8_t* dst, int h, int w, int64_t row_stride, int64_t pix_stride, "
            "int64_t chan_stride, const uint8_t* lut, const int32_t* rects, const uint8_t* fills, int n_rects, void* stream);") in header
    assert "datasets/blender.py:61-79" in header and "a later rectangle wins" in header
    i, i64, vp = _lib._i, _lib._i64, _lib._vp
    assert _lib.SIGNATURES["sr_blender_perturb"] == (i, [vp, vp, i, i, i64, i64, i64, vp, vp, vp, i, vp])
    assert list(inspect.signature(ops.blender_perturb).parameters) == ["image_u8", "lut", "rects", "fills", "layout", "out"]
    assert list(inspect.signature(data.blender_perturbation).parameters) == ["seed", "perturbation"]
    assert list(inspect.signature(data.blender_colors_from_image).parameters) == ["image", "h", "w", "device", "out", "layout", "perturb"]
    assert list(inspect.signature(data.load_blender_perturbed).parameters) == ["root_dir", "perturbation", "split", "img_wh", "device", "reader"]
    sig = inspect.signature(data.load_blender_perturbed).parameters
    assert (sig["split"].default, sig["img_wh"].default, sig["device"].default, sig["reader"].default) == ("train", (400, 400), "cuda", None)
