"""numpy restatements of the evaluation image products (include/satrender.h), in the project's own words:
the nearest-valid-pixel fill by brute force, the byte index of the depth colouring for every combination of given / measured bounds
and both NaN policies, the three summary strips, the crop window, the solar incidence angles and the reference's strip order.  What the
reference itself computes is not restated here: tests/golden/image_products/reference.npz holds the bytes its functions returned
(tests/golden/make_image_products_golden.py), and the tests hold these restatements to them."""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


# ---- the fill -------------------------------------------------------------------------------------------------------------------------
def brute_fill(img):
    """(filled (h, w) fp32, index (h, w) int32, missing [(r, c)], sets [set of uint32 bit patterns]): every NaN pixel takes the bits
    of the valid pixel minimising ((r - r')^2 + (c - c')^2, r', c'); index = r' * w + c' (a valid pixel's own position; -1 when the
    image has no valid pixel).  ``sets[k]`` holds the bit patterns of ALL valid pixels at the least distance from ``missing[k]``."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    h, w = img.shape
    bits = img.view(np.uint32)
    valid = ~np.isnan(img)
    vr, vc = np.nonzero(valid)  # row-major: ascending (r', c')
    out = bits.copy()
    index = np.where(valid, np.arange(h * w, dtype=np.int64).reshape(h, w), -1).astype(np.int32)
    missing, sets = [], []
    for r, c in zip(*np.nonzero(~valid)):
        missing.append((int(r), int(c)))
        if vr.size == 0:
            sets.append(set())
            continue
        d2 = (vr.astype(np.int64) - r) ** 2 + (vc.astype(np.int64) - c) ** 2
        at = np.nonzero(d2 == d2.min())[0]
        k = at[0]  # the first in row-major order: the smallest row, then the smallest column
        out[r, c] = bits[vr[k], vc[k]]
        index[r, c] = vr[k] * w + vc[k]
        sets.append(set(int(b) for b in bits[vr[at], vc[at]]))
    return out.view(np.float32), index, missing, sets


def fixture_image(valid_fraction, seed, h=37, w=53):
    """The fill fixture: (h, w) fp32 of distinct normal values with `valid_fraction` of the pixels kept at random, a 9 x 14 hole, the
    three top rows and the two right columns missing."""
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((h, w)).astype(np.float32)
    assert np.unique(img).size == h * w
    img[rng.random((h, w)) >= valid_fraction] = np.nan
    img[12:21, 20:34] = np.nan
    img[:3, :] = np.nan
    img[:, -2:] = np.nan
    return img


FIXTURES = {"sparse": (0.10, 3), "dense": (0.65, 4)}  # name -> (valid fraction, seed)


def check_against_scipy(img, filled_by_scipy, filled, missing, sets):
    """The two tie-aware checks of a fill against scipy's griddata output.  Every missing pixel: scipy's value is one of the values at
    the least distance.  Every missing pixel with one such value: `filled` has exactly scipy's.  Returns the ambiguous fraction."""
    sb, fb = np.ascontiguousarray(filled_by_scipy, dtype=np.float32).view(np.uint32), np.ascontiguousarray(filled).view(np.uint32)
    valid = ~np.isnan(img)
    assert np.array_equal(sb[valid], img.view(np.uint32)[valid]) and np.array_equal(fb[valid], img.view(np.uint32)[valid])
    ambiguous = 0
    for (r, c), s in zip(missing, sets):
        assert int(sb[r, c]) in s, (r, c)
        assert int(fb[r, c]) in s, (r, c)
        if len(s) == 1:
            assert fb[r, c] == sb[r, c], (r, c)
        else:
            ambiguous += 1
    return ambiguous / max(len(missing), 1)


# ---- the colouring --------------------------------------------------------------------------------------------------------------------
def replace_nonfinite(x):
    x = np.asarray(x, dtype=np.float32)
    return np.where(np.isnan(x), F32(0), np.where(x == np.inf, FLT_MAX, np.where(x == -np.inf, -FLT_MAX, x))).astype(np.float32)


def denominator(mi, ma, vmin, vmax):
    """d of q = (x - mi) / d: both bounds given as Python floats -> the fp64 sum rounded once; else two rounded fp32 operations."""
    if vmin is not None and vmax is not None:
        return F32(float(vmax) - float(vmin) + 1e-8)
    return F32(F32(ma - mi) + F32(1e-8))


def index_image(x, nan_to_zero=False, vmin=None, vmax=None):
    """The (rows, cols) uint8 index: optional NaN / inf replacement, mi / ma given (rounded to fp32) or measured with NaN skipped,
    clipping when a bound is given, q = (x - mi) / d, y = 255 q, truncation; non-finite y -> 0."""
    x = np.asarray(x, dtype=np.float32)
    if nan_to_zero:
        x = replace_nonfinite(x)
    seen = x[~np.isnan(x)]
    with np.errstate(all="ignore"):
        mi = F32(vmin) if vmin is not None else (seen.min() if seen.size else F32(np.inf))
        ma = F32(vmax) if vmax is not None else (seen.max() if seen.size else F32(-np.inf))
        d = denominator(mi, ma, vmin, vmax)
        if vmin is not None or vmax is not None:
            x = np.where(x < mi, mi, x)
            x = np.where(x > ma, ma, x)
        q = ((x - mi) / d).astype(np.float32)
        y = (F32(255) * q).astype(np.float32)
        idx = np.where(np.isfinite(y), np.clip(np.trunc(np.where(np.isfinite(y), y, 0)), 0, 255), 0)
    return idx.astype(np.uint8)


BOUNDS = {"measured": (None, None), "vmin": (80.3, None), "vmax": (None, 120.7), "both": (80.3, 120.7)}


def recorded_bounds(name, tag):
    """The (vmin, vmax) the golden's index image ``color_{name}_{tag}`` was recorded with: BOUNDS, scaled down for the tiny image."""
    vmin, vmax = BOUNDS[tag]
    if name == "tiny":
        vmin, vmax = (None if vmin is None else 1e-9), (None if vmax is None else 1.2e-8)
    return vmin, vmax


def colors_chw(index, lut):
    """(3, rows, cols) fp32 = lut[index] / 255 in fp32 (ToTensor)."""
    return np.ascontiguousarray(np.transpose(lut[index].astype(np.float32) / F32(255), (2, 0, 1)))


# ---- the strips -----------------------------------------------------------------------------------------------------------------------
def crop_window(h, w):
    return int(h / 4), int(3 * h / 4), int(w / 4), int(3 * w / 4)


def crop(img, on=True):
    if not on:
        return img
    r0, r1, c0, c1 = crop_window(img.shape[0], img.shape[1])
    return img[r0:r1, c0:c1]


def unit_bytes(x):
    """(uint8)(x * 255) with one rounded fp32 multiply; clamped outside [0, 1], NaN -> 0."""
    y = (np.asarray(x, dtype=np.float32) * F32(255)).astype(np.float32)
    return np.where(np.isnan(y), 0, np.clip(np.trunc(np.where(np.isnan(y), 0, y)), 0, 255)).astype(np.uint8)


def unit_images():
    """Three (h, w, 3) fp32 images in [0, 1) with one cropped height and three widths; the first holds 0, 1, 1 / 255 and 254.5 / 255
    inside its crop window."""
    rng = np.random.default_rng(7)
    imgs = [rng.random((h, w, 3)).astype(np.float32) for h, w in ((37, 53), (37, 40), (36, 21))]
    imgs[0][9:21, 13:33, 0] = [[0.0, 1.0, 1 / 255, 254.5 / 255] * 5] * 12
    return imgs


def sun_strip(images, on=True):
    return unit_bytes(np.hstack([crop(i, on) for i in images])[:, :, 0])


def rgb_strip(images, on=True):
    return unit_bytes(np.hstack([crop(i, on) for i in images]))


def dsm_strip(images, lut, on=True, vmin=None, vmax=None):
    return np.hstack([lut[index_image(brute_fill(crop(i, on))[0], False, vmin, vmax)] for i in images])


# ---- the sweep ------------------------------------------------------------------------------------------------------------------------
def incidence_angle(sun_d):
    sun_d = np.asarray(sun_d, dtype=np.float64)
    return float(np.degrees(np.arccos(np.dot(sun_d / np.linalg.norm(sun_d), np.array([0., 0., 1.])))))


def sweep(upper, lower, n):
    dirs = [a * np.asarray(upper, np.float64) + (1 - a) * np.asarray(lower, np.float64) for a in np.linspace(0, 1, n)]
    return np.stack(dirs), [incidence_angle(d) for d in dirs]


def strip_order(angles):
    """Positions in the order of the sorted file names "..._solar_incidence_angle_{:.2f}deg.tif"."""
    names = ["x_epoch1_solar_incidence_angle_{:.2f}deg.tif".format(a) for a in angles]
    return [k for _, k in sorted(zip(names, range(len(names))))]
