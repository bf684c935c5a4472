#!/usr/bin/env python3
"""Generate the DSM-registration fixtures under tests/golden/dsmr/ by RUNNING THE REFERENCE's dsmr.py.

Runs only in the build container (needs /root/reference, read-only).  ``dsmr.py`` imports numba and rasterio; neither is needed
for the functions called here, so both are stubbed (``numba.jit`` = the identity) and ``downsample2x``, ``mean_std``, ``ncc``,
``recursive_ncc`` and ``apply_shift_`` run as plain Python on (1, H, W) arrays.  The inputs are fp32 rasters (what the reference
reads from a GeoTIFF) and are handed to the reference as fp64 COPIES: numba types every accumulator fp64, while plain Python under
NumPy 2 would accumulate ``0 + np.float32`` in fp32.  On fp64 copies the plain-Python arithmetic is numba's, operation for operation.

Only DATA is written.  Each fixture holds the inputs, every level's downsampled images (``su{k}`` / ``sv{k}``, k >= 1), NCC maps
(``ncc{k}``, [y][x] over start +- irange) and start shifts (``start{k}`` = (dx, dy)), the final shift and coefficients, and the
``apply_shift_`` output (fp32, as the reference's ``zeros_like`` of an fp32 raster).  The ``metric`` fixture adds the water mask,
the reference's fp32 ``err`` and its ``np.nanmean(abs(err))``.

Every level's best NCC must beat its runner-up by >= 1e-9, so the chosen shift is a fair equality gate for any summation order.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_dsmr_golden.py            # rewrite every fixture (a few minutes)
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_dsmr_golden.py --check    # regenerate in memory, compare bit for bit
"""
import argparse
import importlib.util
import io
import os
import sys
import types
import zipfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "dsmr")
REF = "/root/reference"
sys.dont_write_bytecode = True
MARGIN = 1e-9


def _load_dsmr():
    numba = types.ModuleType("numba")
    numba.jit = lambda f=None, **k: f if f is not None else (lambda g: g)
    rasterio = types.ModuleType("rasterio")
    saved = {m: sys.modules.get(m) for m in ("numba", "rasterio")}
    sys.modules.update(numba=numba, rasterio=rasterio)
    try:
        spec = importlib.util.spec_from_file_location("ref_dsmr", os.path.join(REF, "dsmr.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for m, v in saved.items():
            if v is None:
                sys.modules.pop(m, None)
            else:
                sys.modules[m] = v
    return mod


D = _load_dsmr()
MODE = {"check": False, "failures": []}


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    if MODE["check"]:
        z = np.load(path, allow_pickle=False)
        bad = sorted(set(z.files) ^ set(arrays))
        for k in sorted(set(z.files) & set(arrays)):
            a, b = np.asarray(arrays[k]), z[k]
            if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
                bad.append(k)
        print(f"{name}.npz  {'OK: ' + str(len(arrays)) + ' arrays bit-equal' if not bad else 'MISMATCH: ' + ', '.join(bad)}", flush=True)
        if bad:
            MODE["failures"].append((name, bad))
        return
    os.makedirs(OUT, exist_ok=True)
    # np.savez_compressed with fixed member timestamps: equal arrays -> equal file bytes
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    print(f"{name}.npz  {os.path.getsize(path) / 1024:.0f} KiB", flush=True)


# ---- synthetic DSMs --------------------------------------------------------------------------------------------------------------
def city(rng, h, w, n_boxes):
    """Boxes of 4..40 m on a gentle slope, with a little roof noise: an (h, w) fp64 height field."""
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    z = 20.0 + 0.05 * ii - 0.03 * jj + 2.0 * np.sin(ii / 23.0) * np.cos(jj / 31.0)
    for _ in range(n_boxes):
        bh, bw = rng.integers(6, 28, size=2)
        y0, x0 = rng.integers(0, h - bh), rng.integers(0, w - bw)
        z[y0:y0 + bh, x0:x0 + bw] += rng.uniform(4.0, 40.0)
    return z + rng.normal(0.0, 0.05, size=z.shape)


def pair(rng, hu, wu, hv, wv, dx, dy, dz, n_boxes, pad=40):
    """u = a crop of a city; v the same city seen so that v[j + dy, i + dx] = u[j, i] + dz (+ noise), both fp32."""
    field = city(rng, max(hu, hv) + 2 * pad, max(wu, wv) + 2 * pad, n_boxes)
    u = field[pad:pad + hu, pad:pad + wu]
    v = field[pad - dy:pad - dy + hv, pad - dx:pad - dx + wv] + dz + rng.normal(0.0, 0.02, size=(hv, wv))
    return u.astype(np.float32), v.astype(np.float32)


def holes(rng, img, n_nan, n_inf):
    img = img.copy()
    h, w = img.shape
    for _ in range(n_nan):  # NaN blobs (occlusions / no-data)
        bh, bw = rng.integers(2, 9, size=2)
        y0, x0 = rng.integers(0, h - bh), rng.integers(0, w - bw)
        img[y0:y0 + bh, x0:x0 + bw] = np.nan
    for k in range(n_inf):
        img[rng.integers(0, h), rng.integers(0, w)] = np.inf if k % 2 == 0 else -np.inf
    return img


# ---- the reference, level by level -----------------------------------------------------------------------------------------------
def scan(u, v, irange, sx, sy):
    """ncc(u, v, x, y) over y in sy +- irange (outer), x in sx +- irange (inner), and compute_ncc's winner (first strict max)."""
    n = 2 * irange + 1
    m = np.empty((n, n))
    best, dx, dy = -np.inf, sx, sy
    for a, y in enumerate(range(sy - irange, sy + irange + 1)):
        for b, x in enumerate(range(sx - irange, sx + irange + 1)):
            m[a, b] = D.ncc(u, v, x, y)
            if m[a, b] > best:
                best, dx, dy = m[a, b], x, y
    top = np.sort(m.ravel())[::-1]
    assert np.isfinite(top).all(), "a candidate shift has an undefined NCC"
    assert top[0] - top[1] >= MARGIN, f"NCC winner margin {top[0] - top[1]:.3g} < {MARGIN}"
    return m, dx, dy


def register(u32, v32, irange=5, scaling=False):
    """recursive_ncc + compute_shift's coefficients + apply_shift_, with every level's intermediate state."""
    u, v = u32.astype(np.float64)[None], v32.astype(np.float64)[None]
    levels = [(u, v)]
    while min(levels[-1][0].shape[-2:]) > 100:
        levels.append((D.downsample2x(levels[-1][0]), D.downsample2x(levels[-1][1])))
    out = {"u": u32, "v": v32, "irange": np.int32(irange), "scaling": np.int32(scaling), "levels": np.int32(len(levels))}
    sx = sy = 0
    for k in range(len(levels) - 1, -1, -1):
        su, sv = levels[k]
        if k:
            out[f"su{k}"], out[f"sv{k}"] = su[0], sv[0]
        m, dx, dy = scan(su, sv, irange, sx, sy)
        out[f"ncc{k}"], out[f"start{k}"] = m, np.array([sx, sy], np.int32)
        sx, sy = (2 * dx, 2 * dy) if k else (dx, dy)
    assert (dx, dy) == D.recursive_ncc(u, v, irange), "level-by-level search disagrees with recursive_ncc"
    muu, muv, sigu, sigv, xcorr = D.mean_std(u, v, dx, dy)
    a = sigu / sigv if scaling else 1
    b = muu - muv * a
    out["shift"] = np.array([dx, dy], np.int32)
    out["coef"] = np.array([a, b, muu, muv, sigu, sigv, xcorr], np.float64)
    out["apply"] = D.apply_shift_(v, np.zeros((1,) + v32.shape, np.float32), dx, dy, a, b, 0, 0)[0]
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def case_city(rng):
    u, v = pair(rng, 150, 180, 150, 180, 3, -2, 1.3, 40)
    return register(holes(rng, u, 12, 4), holes(rng, v, 12, 3))


def case_three_level(rng):
    u, v = pair(rng, 220, 300, 220, 300, 14, -9, -2.1, 90)  # |dx| > irange: only the coarse levels can find it
    return register(holes(rng, u, 6, 0), v)


def case_odd_unequal(rng):
    u, v = pair(rng, 103, 121, 110, 117, -4, 3, 0.6, 40)  # odd u, v taller and narrower: item 2's edge rule on both
    return register(holes(rng, u, 4, 1), holes(rng, v, 4, 0))


def case_scaling(rng):
    u, v = pair(rng, 90, 110, 90, 110, 2, 4, 0.0, 30)
    return register(u, (0.8 * v.astype(np.float64) + 3.0).astype(np.float32), scaling=True)


def case_metric(rng):
    """sat_utils.dsm_pointwise_diff's dsmr branch (sat_utils.py:141-178): water to NaN in pred, register, err = rdsm - gt."""
    gt, pred = pair(rng, 130, 140, 130, 140, -2, 1, 0.9, 35)
    mask = np.full(gt.shape, 6, np.uint8)
    mask[90:120, 10:60] = 9  # a lake
    mask[5:12, 100:130] = 9
    pred = pred.copy()
    pred[mask == 9] = np.nan
    out = register(gt, pred)
    err = out["apply"] - gt  # fp32 - fp32
    out.update(mask=mask, err=err, mae=np.array(np.nanmean(np.abs(err.ravel())), np.float32))
    return out


CASES = {"dsmr_city": case_city, "dsmr_three_level": case_three_level, "dsmr_odd_unequal": case_odd_unequal,
         "dsmr_scaling": case_scaling, "dsmr_metric": case_metric}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", default=None, help="comma-separated fixture names (default: all): " + " ".join(CASES))
    ap.add_argument("--check", action="store_true", help="write nothing: regenerate in memory and compare with the committed fixtures, bit for bit")
    a = ap.parse_args()
    MODE["check"] = a.check
    names = list(CASES) if a.only is None else a.only.split(",")
    for name in names:
        save(name, **CASES[name](np.random.default_rng(zlib.crc32(name.encode()))))
    if os.path.isdir(OUT):
        extra = sorted(set(f[:-4] for f in os.listdir(OUT) if f.endswith(".npz")) - set(CASES))
        assert not extra, f"fixtures without a recipe: {extra}"
    if MODE["failures"]:
        print("FAILED:", MODE["failures"])
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
