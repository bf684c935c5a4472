"""DSM extraction, host side (no GPU): UTM zone rules, grid geometry, and the fp64 numpy UTM restatement that tests/test_hip_dsm.py
uses as its yardstick, itself checked against independent references (a quadrature of the meridian arc, the Snyder / USGS series
off the meridian, and the inverse Krueger series)."""
import math
import os

import numpy as np
import pytest

from satnerf_amd import _lib, dsm

A_WGS84, F_WGS84, K0 = 6378137.0, 1 / 298.257223563, 0.9996
E2 = F_WGS84 * (2 - F_WGS84)
N3 = F_WGS84 / (2 - F_WGS84)


# ---- restatements (the yardsticks) ----------------------------------------------------------------------------------------------
def _alpha(n):
    return [n / 2 - 2 * n**2 / 3 + 5 * n**3 / 16 + 41 * n**4 / 180 - 127 * n**5 / 288 + 7891 * n**6 / 37800,
            13 * n**2 / 48 - 3 * n**3 / 5 + 557 * n**4 / 1440 + 281 * n**5 / 630 - 1983433 * n**6 / 1935360,
            61 * n**3 / 240 - 103 * n**4 / 140 + 15061 * n**5 / 26880 + 167603 * n**6 / 181440,
            49561 * n**4 / 161280 - 179 * n**5 / 168 + 6601661 * n**6 / 7257600,
            34729 * n**5 / 80640 - 3418889 * n**6 / 1995840,
            212378941 * n**6 / 319334400]


def _beta(n):
    return [n / 2 - 2 * n**2 / 3 + 37 * n**3 / 96 - n**4 / 360 - 81 * n**5 / 512 + 96199 * n**6 / 604800,
            n**2 / 48 + n**3 / 15 - 437 * n**4 / 1440 + 46 * n**5 / 105 - 1118711 * n**6 / 3870720,
            17 * n**3 / 480 - 37 * n**4 / 840 - 209 * n**5 / 4480 + 5569 * n**6 / 90720,
            4397 * n**4 / 161280 - 11 * n**5 / 504 - 830251 * n**6 / 7257600,
            4583 * n**5 / 161280 - 108847 * n**6 / 3991680,
            20648693 * n**6 / 638668800]


def _rect_A(n):
    return A_WGS84 / (1 + n) * (1 + n**2 / 4 + n**4 / 64 + n**6 / 256)


def central_meridian(zone):
    return 6.0 * zone - 183.0


def utm_forward_np(lat, lon, zone):
    """fp64 transverse Mercator, Krueger's series to n^6 (Karney 2011): (east, north), false northing 0 in both hemispheres."""
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    dl = lon - central_meridian(zone)
    dl = np.where(dl >= 180, dl - 360, np.where(dl < -180, dl + 360, dl))
    lam, phi = np.radians(dl), np.radians(lat)
    e = math.sqrt(E2)
    tau = np.tan(phi)
    sig = np.sinh(e * np.arctanh(e * tau / np.sqrt(1 + tau * tau)))
    taup = tau * np.sqrt(1 + sig * sig) - sig * np.sqrt(1 + tau * tau)
    xip = np.arctan2(taup, np.cos(lam))
    etap = np.arcsinh(np.sin(lam) / np.sqrt(taup * taup + np.cos(lam) ** 2))
    xi, eta = xip.copy(), etap.copy()
    for j, a in enumerate(_alpha(N3), start=1):
        xi += a * np.sin(2 * j * xip) * np.cosh(2 * j * etap)
        eta += a * np.cos(2 * j * xip) * np.sinh(2 * j * etap)
    k = K0 * _rect_A(N3)
    return 500000.0 + k * eta, k * xi


def utm_inverse_np(east, north, zone):
    """Inverse series (Karney 2011 eqs. 11, 15, 19-21): (lat, lon) degrees."""
    k = K0 * _rect_A(N3)
    xi, eta = np.asarray(north, np.float64) / k, (np.asarray(east, np.float64) - 500000.0) / k
    xip, etap = xi.copy(), eta.copy()
    for j, b in enumerate(_beta(N3), start=1):
        xip -= b * np.sin(2 * j * xi) * np.cosh(2 * j * eta)
        etap -= b * np.cos(2 * j * xi) * np.sinh(2 * j * eta)
    taup = np.sin(xip) / np.sqrt(np.sinh(etap) ** 2 + np.cos(xip) ** 2)
    lam = np.arctan2(np.sinh(etap), np.cos(xip))
    e = math.sqrt(E2)
    tau = taup.copy()
    for _ in range(6):  # Newton on tau'(tau) = taup
        sig = np.sinh(e * np.arctanh(e * tau / np.sqrt(1 + tau * tau)))
        tp = tau * np.sqrt(1 + sig * sig) - sig * np.sqrt(1 + tau * tau)
        dtau = (taup - tp) / (np.sqrt(1 + tp * tp)) * (1 + (1 - E2) * tau * tau) / ((1 - E2) * np.sqrt(1 + tau * tau))
        tau = tau + dtau
    return np.degrees(np.arctan(tau)), np.degrees(lam) + central_meridian(zone)


def grid_from_bounds_ref(cloud, resolution):
    """datasets/satellite.py:302-307 restated over an (N, 2+) numpy cloud."""
    xmin, xmax = cloud[:, 0].min(), cloud[:, 0].max()
    ymin, ymax = cloud[:, 1].min(), cloud[:, 1].max()
    xoff = np.floor(xmin / resolution) * resolution
    xsize = int(1 + np.floor((xmax - xoff) / resolution))
    yoff = np.ceil(ymax / resolution) * resolution
    ysize = int(1 - np.floor((ymin - yoff) / resolution))
    return xoff, yoff, xsize, ysize


def rasterize_np(east, north, alt, xoff, yoff, res, xsize, ysize, radius, sigma):
    """fp64 restatement of the splat convention (include/satrender.h sr_dsm_rasterize): (dsm, weight) float64."""
    sw = np.zeros((ysize, xsize))
    swa = np.zeros((ysize, xsize))
    ok = np.isfinite(east) & np.isfinite(north) & np.isfinite(alt)
    e, n, a = east[ok], north[ok], alt[ok]
    u, v = (e - xoff) / res, (yoff - n) / res
    inside = (u >= 0) & (u < xsize) & (v >= 0) & (v < ysize)
    u, v, a = u[inside], v[inside], a[inside]
    c, j = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    for dj in range(-radius, radius + 1):
        for dc in range(-radius, radius + 1):
            jj, cc = j + dj, c + dc
            m = (jj >= 0) & (jj < ysize) & (cc >= 0) & (cc < xsize)
            if math.isinf(sigma):
                w = np.ones(m.sum())
            else:
                du, dv = u[m] - (cc[m] + 0.5), v[m] - (jj[m] + 0.5)
                w = np.exp(-(du * du + dv * dv) / (2 * sigma * sigma))
            np.add.at(sw, (jj[m], cc[m]), w)
            np.add.at(swa, (jj[m], cc[m]), w * a[m])
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(sw > 0, swa / sw, np.nan)
    return out, sw


@pytest.fixture(scope="module", autouse=True)
def _library():
    """The zone rules live in the C ABI (sr_utm_zone, host code): build the library if it is missing."""
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()


# ---- zone rules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat,lon,zone,letter", [
    (30.3, -81.7, 17, "R"),            # Jacksonville (JAX)
    (0.0, 0.0, 31, "N"), (-0.0001, 0.0, 31, "M"),
    (40.0, -180.0, 1, "T"), (40.0, 180.0, 1, "T"),   # lon = +-180 normalise to [-180, 180): zone 1
    (40.0, 179.999, 60, "T"), (40.0, -174.0, 2, "T"), (40.0, -174.0000001, 1, "T"),
    (56.0, 3.0, 32, "V"), (55.9999, 3.0, 31, "U"), (63.9999, 11.9999, 32, "V"), (64.0, 3.0, 31, "W"), (60.0, 2.9999, 31, "V"),
    (60.0, 12.0, 33, "V"),
    (72.0, 0.0, 31, "X"), (71.9999, 8.0, 32, "W"), (72.0, 8.9999, 31, "X"), (72.0, 9.0, 33, "X"), (78.0, 20.9999, 33, "X"),
    (78.0, 21.0, 35, "X"), (84.0, 32.9999, 35, "X"), (84.0, 33.0, 37, "X"), (80.0, 41.9999, 37, "X"), (80.0, 42.0, 38, "X"),
    (80.0, -0.0001, 30, "X"),
    (-80.0, 10.0, 32, "C"), (-72.0, 10.0, 32, "D"), (-72.0001, 10.0, 32, "C"), (84.0, 10.0, 33, "X"), (80.0, 10.0, 33, "X"),
    (8.0, 10.0, 32, "P"), (7.9999, 10.0, 32, "N"), (-8.0, 10.0, 32, "M"), (-8.0001, 10.0, 32, "L"),
])
def test_zone_number_and_letter(lat, lon, zone, letter):
    assert dsm.utm_zone(lat, lon) == (zone, letter)


@pytest.mark.parametrize("lat", [-80.0001, 84.0001, 90.0, -90.0, float("nan")])
def test_zone_out_of_range_latitude_raises(lat):
    with pytest.raises(ValueError):
        dsm.utm_zone(lat, 10.0)


def test_zone_rules_match_restatement_on_a_sweep():
    """int((lon + 180) / 6) + 1 away from the exceptions, and the letter table, over a lat/lon sweep."""
    letters = "CDEFGHJKLMNPQRSTUVWXX"
    rng = np.random.default_rng(3)
    for lat, lon in zip(rng.uniform(-80, 84, 400), rng.uniform(-180, 180, 400)):
        zone, letter = dsm.utm_zone(lat, lon)
        assert letter == letters[int(lat + 80) >> 3]
        if not (56 <= lat < 64 and 3 <= lon < 12) and not (72 <= lat <= 84 and 0 <= lon < 42):
            assert zone == int((lon + 180) / 6) + 1


# ---- grid geometry ------------------------------------------------------------------------------------------------------------
def test_auto_grid_matches_reference_restatement():
    rng = np.random.default_rng(5)
    for res in (0.5, 0.3, 1.0):
        cloud = np.stack([rng.uniform(435000, 436000, 500), rng.uniform(-3.35e6, 3.35e6, 500) * 1e-3 + 3352000], 1)
        xmin, xmax, ymin, ymax = cloud[:, 0].min(), cloud[:, 0].max(), cloud[:, 1].min(), cloud[:, 1].max()
        assert dsm.grid_from_bounds(xmin, xmax, ymin, ymax, res) == grid_from_bounds_ref(cloud, res)
    # points exactly on cell edges: floor/ceil on exact multiples
    cloud = np.array([[10.0, 20.0], [12.5, 17.5]])
    assert dsm.grid_from_bounds(10.0, 12.5, 17.5, 20.0, 0.5) == grid_from_bounds_ref(cloud, 0.5) == (10.0, 20.0, 6, 6)
    # every point inside the grid it sizes
    xoff, yoff, xsize, ysize = dsm.grid_from_bounds(xmin, xmax, ymin, ymax, 1.0)
    assert xoff <= xmin and xmax < xoff + xsize and yoff >= ymax and ymin > yoff - ysize


def test_roi_grid_has_the_reference_yoff_quirk():
    roi = np.array([435400.0, 3354000.0, 512.0, 0.5])  # {aoi}_DSM.txt: x, y, s, r
    xoff, yoff, xsize, ysize, r = dsm.grid_from_roi(roi)
    # datasets/satellite.py:295-300
    want_yoff = roi[1] + int(roi[2]) * roi[3]
    assert (xoff, yoff, xsize, ysize, r) == (roi[0], want_yoff, 512, 512, 0.5)
    with pytest.raises(ValueError):
        dsm.grid_from_roi([1.0, 2.0, 3.0])


def test_transform_and_zone_string():
    d = dsm.DSM(None, None, 100.0, 200.0, 0.5, "17R")
    assert d.transform == (0.5, 0.0, 100.0, 0.0, -0.5, 200.0)


def test_rasterize_restatement_convention():
    """The restatement itself: a point in cell (j, c) lands there; row 0 is north; edges belong to the cell to the east / south
    (east [c r, (c+1) r), north (yoff - (j+1) r, yoff - j r])."""
    e = np.array([0.0, 0.99, 1.0, 2.5])
    n = np.array([10.0, 9.01, 9.0, 8.0])
    a = np.array([1.0, 2.0, 3.0, 4.0])
    out, w = rasterize_np(e, n, a, 0.0, 10.0, 1.0, 3, 3, 0, float("inf"))
    assert out[0, 0] == 1.5 and w[0, 0] == 2  # (0, 10) and (0.99, 9.01)
    assert out[1, 1] == 3.0                   # (1, 9): the cell to the east and south of the edge
    assert out[2, 2] == 4.0
    assert np.isnan(out[0, 1]) and w[0, 1] == 0


# ---- the UTM restatement against independent references ----------------------------------------------------------------------
def test_central_meridian_northing_is_k0_times_meridian_arc():
    from scipy.integrate import quad

    def arc(phi):
        return quad(lambda p: A_WGS84 * (1 - E2) / (1 - E2 * math.sin(p) ** 2) ** 1.5, 0.0, phi, epsabs=1e-10, epsrel=1e-13)[0]

    for lat in np.linspace(-80, 84, 83):
        east, north = utm_forward_np(lat, central_meridian(17), 17)
        assert abs(float(east) - 500000.0) < 1e-9
        assert abs(float(north) - K0 * arc(math.radians(lat))) <= 1e-6, lat


def _snyder_forward(lat, lon, zone):
    """USGS PP 1395 (Snyder 1987) eqs. 8-9, 8-10 with the series meridian arc 3-21: an independent derivation."""
    phi, lam = np.radians(lat), np.radians(lon - central_meridian(zone))
    ep2 = E2 / (1 - E2)
    Nn = A_WGS84 / np.sqrt(1 - E2 * np.sin(phi) ** 2)
    T, Cc, Aa = np.tan(phi) ** 2, ep2 * np.cos(phi) ** 2, lam * np.cos(phi)
    e4, e6 = E2 * E2, E2 * E2 * E2
    M = A_WGS84 * ((1 - E2 / 4 - 3 * e4 / 64 - 5 * e6 / 256) * phi - (3 * E2 / 8 + 3 * e4 / 32 + 45 * e6 / 1024) * np.sin(2 * phi)
                   + (15 * e4 / 256 + 45 * e6 / 1024) * np.sin(4 * phi) - (35 * e6 / 3072) * np.sin(6 * phi))
    x = K0 * Nn * (Aa + (1 - T + Cc) * Aa**3 / 6 + (5 - 18 * T + T * T + 72 * Cc - 58 * ep2) * Aa**5 / 120)
    y = K0 * (M + Nn * np.tan(phi) * (Aa**2 / 2 + (5 - T + 9 * Cc + 4 * Cc * Cc) * Aa**4 / 24
                                      + (61 - 58 * T + T * T + 600 * Cc - 330 * ep2) * Aa**6 / 720))
    return 500000.0 + x, y


def test_off_meridian_agrees_with_snyder_series():
    lat, lon = np.meshgrid(np.linspace(-60, 60, 61), central_meridian(31) + np.linspace(-3.5, 3.5, 29))
    e1, n1 = utm_forward_np(lat, lon, 31)
    e2, n2 = _snyder_forward(lat, lon, 31)
    worst = max(np.abs(e1 - e2).max(), np.abs(n1 - n2).max())
    print(f"Krueger n^6 vs Snyder, |dlon| <= 3.5 deg, |lat| <= 60: {worst * 1e3:.3f} mm")
    assert worst <= 1e-3


def test_forward_inverse_round_trip():
    rng = np.random.default_rng(11)
    lat, dlon = rng.uniform(-80, 84, 2000), rng.uniform(-6, 6, 2000)
    for zone in (1, 17, 31, 60):
        lon = central_meridian(zone) + dlon
        east, north = utm_forward_np(lat, lon, zone)
        lat2, lon2 = utm_inverse_np(east, north, zone)
        e2, n2 = utm_forward_np(lat2, lon2, zone)
        assert np.abs(e2 - east).max() <= 1e-6 and np.abs(n2 - north).max() <= 1e-6
        # 1e-11 deg ~ 1 micrometre
        assert np.abs(lat2 - lat).max() < 1e-11 and np.abs(lon2 - lon).max() < 1e-11


def test_southern_points_have_negative_northing():
    east, north = utm_forward_np(np.array([-33.9, -0.001]), np.array([18.4, 3.0]), 34)
    assert north[0] < -3.7e6 and north[1] < 0
