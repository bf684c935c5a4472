"""DSM registration, host side (no GPU): a vectorised numpy restatement of dsmr.compute_shift / dsmr.apply_shift and of the metric of
sat_utils.dsm_pointwise_diff's dsmr branch, pinned to the fixtures tests/golden/make_dsmr_golden.py wrote by
running the reference.  tests/test_hip_dsmr.py uses this restatement as its yardstick on inputs no fixture covers.

Conventions: images are (H, W), i the column, j the row, a shift (dx, dy) pairs u[j, i] with v[j + dy, i + dx]; every loop spans
u's extent except apply's, which spans v's.  Non-finite values and reads outside v are skipped."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dsmr")
FIXTURES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz")) if os.path.isdir(GOLDEN) else []


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def downsample(u):
    """(ceil(H/2), ceil(W/2)) fp64: cell (J, I) averages the finite in-bounds pixels of the 2x2 window at
    (min(2J + 1, H - 1), min(2I + 1, W - 1)), summed from 0.0 in the order (j, i), (j+1, i), (j, i+1), (j+1, i+1); NaN if none."""
    u = np.asarray(u, np.float64)
    h, w = u.shape
    j0 = np.minimum(2 * np.arange((h + 1) // 2) + 1, h - 1)[:, None]
    i0 = np.minimum(2 * np.arange((w + 1) // 2) + 1, w - 1)[None, :]
    s = np.zeros((j0.shape[0], i0.shape[1]))
    n = np.zeros(s.shape, np.int64)
    for dj, di in ((0, 0), (1, 0), (0, 1), (1, 1)):
        jj, ii = np.broadcast_arrays(j0 + dj, i0 + di)
        inb = (jj < h) & (ii < w)
        t = np.full(s.shape, np.nan)
        t[inb] = u[jj[inb], ii[inb]]
        ok = np.isfinite(t)
        s = np.where(ok, s + np.where(ok, t, 0.0), s)
        n += ok
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, s / np.maximum(n, 1), np.nan)


def shifted(v, dx, dy, shape):
    """out[j, i] = v[j + dy, i + dx] over `shape`, NaN outside v."""
    v = np.asarray(v)
    h, w = shape
    out = np.full(shape, np.nan, np.float64)
    j0, j1 = max(0, -dy), min(h, v.shape[0] - dy)
    i0, i1 = max(0, -dx), min(w, v.shape[1] - dx)
    if j0 < j1 and i0 < i1:
        out[j0:j1, i0:i1] = v[j0 + dy:j1 + dy, i0 + dx:i1 + dx]
    return out


def mean_std(u, v, dx, dy):
    """(count, mu_u, mu_v, sig_u, sig_v, xcorr, ncc) of u against v shifted by (dx, dy), two-pass, fp64.  ncc is NaN where the
    reference raises (count = 0 or sig_u sig_v = 0)."""
    u = np.asarray(u, np.float64)
    vv = shifted(v, dx, dy, u.shape)
    m = np.isfinite(u) & np.isfinite(vv)
    count = int(m.sum())
    if count == 0:
        return (0,) + (np.nan,) * 6
    mu_u, mu_v = u[m].sum() / count, vv[m].sum() / count
    with np.errstate(invalid="ignore", over="ignore"):
        du, dv = u - mu_u, vv - mu_v
    m2 = np.isfinite(du) & np.isfinite(dv)
    su, sv = np.sqrt((du[m2] ** 2).sum() / count), np.sqrt((dv[m2] ** 2).sum() / count)
    xc = (du[m2] * dv[m2]).sum() / count
    ncc = xc / (su * sv) if su * sv != 0 else np.nan
    return count, mu_u, mu_v, su, sv, xc, ncc


def scan(u, v, irange, sx, sy):
    """NCC map [y][x] over (sx, sy) +- irange and the first strict maximum in y-outer, x-inner order (the start if none)."""
    n = 2 * irange + 1
    m = np.array([[mean_std(u, v, sx + x, sy + y)[6] for x in range(-irange, irange + 1)] for y in range(-irange, irange + 1)])
    flat = np.where(np.isnan(m.ravel()), -np.inf, m.ravel())
    if not np.isfinite(m).any():
        return m, sx, sy
    k = int(np.argmax(flat))  # argmax returns the first index of the maximum
    return m, sx + k % n - irange, sy + k // n - irange


def levels_of(u, v):
    lv = [(np.asarray(u, np.float64), np.asarray(v, np.float64))]
    while min(lv[-1][0].shape) > 100:
        lv.append((downsample(lv[-1][0]), downsample(lv[-1][1])))
    return lv


def compute_shift(u, v, scaling=True, irange=5):
    """dict: levels (the (u_k, v_k) pairs, k = 0 finest), ncc / start per level, shift (dx, dy), stats at the shift, a, b."""
    lv = levels_of(u, v)
    maps, starts = [None] * len(lv), [None] * len(lv)
    sx = sy = 0
    for k in range(len(lv) - 1, -1, -1):
        starts[k] = (sx, sy)
        maps[k], dx, dy = scan(lv[k][0], lv[k][1], irange, sx, sy)
        sx, sy = 2 * dx, 2 * dy
    st = mean_std(u, v, dx, dy)
    if st[0] == 0:
        raise ValueError("no valid overlap at the registered shift")
    with np.errstate(invalid="ignore", divide="ignore"):
        a = st[3] / st[4] if scaling else 1.0
    return {"levels": lv, "ncc": maps, "start": starts, "shift": (dx, dy), "stats": st, "a": a, "b": st[1] - st[2] * a}


def apply_shift(v, dx, dy, a, b):
    """a v[j + dy, i + dx] + b (+ 0.0, the reference's integer terms) in fp64 over v's extent, NaN outside v, stored fp32."""
    with np.errstate(invalid="ignore"):
        return (a * shifted(v, dx, dy, np.shape(v)) + b + 0.0).astype(np.float32)


def registered_err(pred, gt, mask=None):
    """The dsmr branch of sat_utils.dsm_pointwise_diff: water (class 9) to NaN in pred, register pred on gt, err = rdsm - gt."""
    pred = np.array(pred, np.float32)
    if mask is not None:
        pred[mask == 9] = np.nan
    r = compute_shift(gt, pred, scaling=False)
    rdsm = apply_shift(pred, *r["shift"], r["a"], r["b"])
    return rdsm - np.asarray(gt, np.float32), rdsm, r


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


# ---- pinned to the reference's fixtures ------------------------------------------------------------------------------------------
def test_fixtures_present():
    assert set(FIXTURES) >= {"dsmr_city", "dsmr_three_level", "dsmr_odd_unequal", "dsmr_scaling", "dsmr_metric"}


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_reference(name):
    g = load(name)
    r = compute_shift(g["u"], g["v"], scaling=bool(g["scaling"]), irange=int(g["irange"]))
    assert len(r["levels"]) == int(g["levels"])
    for k in range(1, len(r["levels"])):
        assert np.array_equal(bits(r["levels"][k][0]), bits(g[f"su{k}"])) and np.array_equal(bits(r["levels"][k][1]), bits(g[f"sv{k}"]))
    for k in range(len(r["levels"])):
        assert tuple(g[f"start{k}"]) == r["start"][k]
        assert np.abs(r["ncc"][k] - g[f"ncc{k}"]).max() <= 1e-12
    assert tuple(g["shift"]) == r["shift"]
    want = g["coef"]  # a, b, mu_u, mu_v, sig_u, sig_v, xcorr
    got = np.array([r["a"], r["b"], *r["stats"][1:6]])
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))
    out = apply_shift(g["v"], *(int(s) for s in g["shift"]), float(want[0]), float(want[1]))
    assert out.dtype == np.float32 and np.array_equal(bits(out), bits(g["apply"]))


def test_metric_fixture():
    g = load("dsmr_metric")
    err, _, _ = registered_err(g["v"], g["u"], g["mask"])
    assert np.isnan(g["v"][g["mask"] == 9]).all()  # the fixture's pred already carries the water NaNs
    assert np.array_equal(bits(err), bits(g["err"]))
    assert abs(float(np.nanmean(np.abs(err.astype(np.float64)))) - float(g["mae"])) <= 1e-6 * float(g["mae"])


# ---- the restatement's own rules ---------------------------------------------------------------------------------------------------
def test_downsample_edge_rule():
    u = np.arange(16, dtype=np.float64).reshape(4, 4)
    assert np.array_equal(downsample(u), [[7.5, 9.0], [13.5, 15.0]])
    odd = np.arange(15, dtype=np.float64).reshape(3, 5)  # last row / column: one-pixel-wide windows
    assert np.array_equal(downsample(odd), [[9.0, 11.0, 11.5], [11.5, 13.5, 14.0]])
    assert np.isnan(downsample(np.full((3, 3), np.nan))).all()
    assert bits(downsample(np.array([[1.0, 1.0], [1.0, -0.0]])))[0, 0] == 0  # a lone -0.0 averages to +0.0


def test_ncc_undefined_shifts_are_never_chosen():
    rng = np.random.default_rng(3)
    u = rng.normal(size=(20, 20))
    v = np.full((4, 4), np.nan)
    v[:2, :2] = rng.normal(size=(2, 2))
    m, dx, dy = scan(u, v, 3, 0, 0)
    assert np.isnan(m).any() and np.isfinite(m).any()
    assert np.isfinite(m[dy + 3, dx + 3])
    c = np.ones((12, 12))
    m, dx, dy = scan(c, c, 2, 1, -1)  # zero variance everywhere: the start stays
    assert np.isnan(m).all() and (dx, dy) == (1, -1)
    with pytest.raises(ValueError):
        compute_shift(np.full((8, 8), np.nan), np.ones((8, 8)))


def test_known_shift_recovered():
    rng = np.random.default_rng(5)
    z = np.cumsum(np.cumsum(rng.normal(size=(120, 140)), 0), 1) * 0.01
    u = z[10:90, 10:110].astype(np.float32)
    v = (z[10 + 3:90 + 3, 10 - 4:110 - 4] + 0.7).astype(np.float32)  # v[j - 3, i + 4] = u[j, i] + 0.7
    r = compute_shift(u, v, scaling=False)
    assert r["shift"] == (4, -3) and abs(r["b"] + 0.7) < 1e-5
