#!/usr/bin/env python3
"""Generate the cloud-fusion fixtures under tests/golden/cloud_grid/ by RUNNING THE REFERENCE's eval_s2p.project_cloud_into_utm_grid.

Runs only in the build container (needs /root/reference, read-only).  ``eval_s2p.py`` imports rasterio, osgeo.gdal and sat_utils at
module level; the function called here touches none of them, so all three are stubbed.  Only DATA is written: per fixture the cloud
``xyz`` (N, 3) fp64, ``bb`` = [xmin, xmax, ymin, ymax], ``definition``, and the reference's four rasters ``min`` / ``max`` / ``avg`` /
``med`` (map_h, map_w) fp64, already flipped (row 0 north), NaN where no point landed.

No fixture holds a non-finite value, and none puts -0.0 and +0.0 altitudes into one cell (the reference's answer would then depend
on argsort's tie order).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cloud_grid_golden.py            # rewrite every fixture
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cloud_grid_golden.py --check    # regenerate in memory, compare bit for bit
"""
import argparse
import contextlib
import importlib.util
import io
import os
import sys
import types
import zipfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cloud_grid")
REF = "/root/reference"
sys.dont_write_bytecode = True
MODES = ("min", "max", "avg", "med")


def _load_eval_s2p():
    rasterio, osgeo, gdal, sat_utils = (types.ModuleType(m) for m in ("rasterio", "osgeo", "osgeo.gdal", "sat_utils"))
    osgeo.gdal = gdal
    sat_utils.compute_mae_and_save_dsm_diff = None
    stubs = {"rasterio": rasterio, "osgeo": osgeo, "osgeo.gdal": gdal, "sat_utils": sat_utils}
    saved = {m: sys.modules.get(m) for m in stubs}
    sys.modules.update(stubs)
    try:
        spec = importlib.util.spec_from_file_location("ref_eval_s2p", os.path.join(REF, "eval_s2p.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for m, v in saved.items():
            if v is None:
                sys.modules.pop(m, None)
            else:
                sys.modules[m] = v
    return mod


S = _load_eval_s2p()
STATE = {"check": False, "failures": []}


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    if STATE["check"]:
        z = np.load(path, allow_pickle=False)
        bad = sorted(set(z.files) ^ set(arrays))
        for k in sorted(set(z.files) & set(arrays)):
            a, b = np.asarray(arrays[k]), z[k]
            if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
                bad.append(k)
        print(f"{name}.npz  {'OK: ' + str(len(arrays)) + ' arrays bit-equal' if not bad else 'MISMATCH: ' + ', '.join(bad)}", flush=True)
        if bad:
            STATE["failures"].append((name, bad))
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


def run(xyz, bb, definition):
    """The reference's four rasters for one cloud (its 'less than 3 points' print is swallowed)."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    assert np.isfinite(xyz).all()
    out = {"xyz": xyz, "bb": np.asarray(bb, np.float64), "definition": np.float64(definition)}
    for mode in MODES:
        with contextlib.redirect_stdout(io.StringIO()):
            out[mode] = S.project_cloud_into_utm_grid(xyz.copy(), list(bb), definition, mode)
        assert out[mode].dtype == np.float64
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def case_ties(rng):
    """definition 0.5 (half-cells exact in binary): every quarter step from three before the origin to three past the last cell
    centre, in both axes.  x0 - 0.25 rounds to -0 (kept, column 0); the last centre + 0.25 is kept or dropped by half-even."""
    bb, d = [100.0, 102.0, 50.0, 51.5], 0.5  # a 4 x 5 map
    xs = bb[0] + 0.25 * np.arange(-3, 2 * 4 + 4)
    ys = bb[2] + 0.25 * np.arange(-3, 2 * 3 + 4)
    xx, yy = (a.ravel() for a in np.meshgrid(xs, ys))
    xx, yy = np.tile(xx, 3), np.tile(yy, 3)
    extra = np.array([[101.0, 51.75], [101.0, 49.75]])  # dropped (row 3.5 -> 4); row -0.5 -> -0, kept
    xy = np.concatenate([np.stack([xx, yy], 1), extra])
    xy = xy[rng.permutation(len(xy))]
    return run(np.column_stack([xy, rng.uniform(-3.0, 25.0, len(xy))]), bb, d)


def case_city(rng):
    """~4000 points on a 40 x 30 grid: a block without points, negative altitudes, exact duplicate altitudes within cells."""
    x0, y0, d = 435000.0, 3354000.0, 0.5
    bb = [x0, x0 + 19.5, y0, y0 + 14.5]
    n = 4400
    x = rng.uniform(bb[0] - 1.0, bb[1] + 1.0, n)
    y = rng.uniform(bb[2] - 1.0, bb[3] + 1.0, n)
    keep = ~((x > x0 + 6) & (x < x0 + 9) & (y > y0 + 4) & (y < y0 + 8))
    x, y = x[keep], y[keep]
    z = rng.uniform(-8.0, 40.0, len(x))
    q = rng.random(len(x)) < 0.5
    z[q] = np.round(z[q] * 2) / 2  # half-metre steps: duplicates within a cell
    z[z == 0] = 0.5  # no zero of either sign
    xyz = np.column_stack([x, y, z])
    return run(np.concatenate([xyz, xyz[:200]]), bb, d)  # and 200 exact duplicate points


def case_counts(rng):
    """Cells holding exactly 1, 2, 3, 4, 63, 64, 65 and 1500 points (and two empty ones) on a 2 x 5 map."""
    bb, d = [0.0, 4.0, 0.0, 1.0], 1.0
    counts = [1, 2, 3, 4, 63, 64, 65, 1500]
    pts = []
    for k, c in enumerate(counts):
        cx, cy = k % 5, k // 5
        pts.append(np.column_stack([cx + rng.uniform(-0.4, 0.4, c), cy + rng.uniform(-0.4, 0.4, c), rng.normal(30.0, 12.0, c)]))
    xyz = np.concatenate(pts)
    return run(xyz[rng.permutation(len(xyz))], bb, d)


def case_metric(rng):
    """definition 0.3 (not a power of two) at UTM magnitudes: the division and rounding at real sizes, with points on computed
    half-cell positions."""
    x0, y0, d = 435217.17, 3354108.41, 0.3
    bb = [x0, x0 + 12.0, y0, y0 + 9.0]
    n = 3000
    x = rng.uniform(bb[0] - 0.5, bb[1] + 0.5, n)
    y = rng.uniform(bb[2] - 0.5, bb[3] + 0.5, n)
    k = rng.integers(-1, 42, 300)
    x[:300] = x0 + (k + 0.5) * d
    y[300:600] = y0 + (rng.integers(-1, 32, 300) + 0.5) * d
    return run(np.column_stack([x, y, rng.uniform(-2.0, 60.0, n)]), bb, d)


CASES = {"ties": case_ties, "city": case_city, "counts": case_counts, "metric": case_metric}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", default=None, help="comma-separated fixture names (default: all): " + " ".join(CASES))
    ap.add_argument("--check", action="store_true", help="write nothing: regenerate in memory and compare with the committed fixtures, bit for bit")
    a = ap.parse_args()
    STATE["check"] = a.check
    names = list(CASES) if a.only is None else a.only.split(",")
    for name in names:
        save(name, **CASES[name](np.random.default_rng(zlib.crc32(name.encode()))))
    if os.path.isdir(OUT):
        extra = sorted(set(f[:-4] for f in os.listdir(OUT) if f.endswith(".npz")) - set(CASES))
        assert not extra, f"fixtures without a recipe: {extra}"
    if STATE["failures"]:
        print("FAILED:", STATE["failures"])
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
