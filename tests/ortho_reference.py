"""fp64 numpy restatement of the nadir DSM rays (csrc/ortho.hip), the yardstick of the HIP path.

The inverse UTM projection is ``tests/test_dsm_host.utm_inverse_np`` (Karney 2011 eqs. 11, 15, 19-21): that function defines the
result.  A ray goes straight down through a cell centre: origin at ``max_alt`` normalised in fp64, direction the inward ellipsoid
normal in closed form, near = 0, far = (max_alt - min_alt) / range, the sun direction appended.
"""
import numpy as np

from oracle.rpc_oracle import latlon_to_ecef
from tests.test_dsm_host import utm_inverse_np  # noqa: F401  (re-exported: the definition of the inverse)


def cell_centres(grid):
    """(east, north), each (ysize, xsize): row 0 at the top, as ``dsm.DSM`` lays its raster out."""
    xoff, yoff, xsize, ysize, r = grid
    jj, cc = np.meshgrid(np.arange(int(ysize)), np.arange(int(xsize)), indexing="ij")
    return xoff + (cc + 0.5) * r, yoff - (jj + 0.5) * r


def ortho_rays_np(grid, zone, min_alt, max_alt, center, scene_range, sun_d):
    """(rays (ysize * xsize, 11) float64 -- not yet rounded to fp32 -- , latlon (ysize * xsize, 2) float64 degrees)."""
    east, north = cell_centres(grid)
    lat, lon = utm_inverse_np(east.ravel(), north.ravel(), zone)
    x, y, z = latlon_to_ecef(lat, lon, float(max_alt))
    phi, lam = lat * (np.pi / 180.0), lon * (np.pi / 180.0)
    rays = np.zeros((lat.size, 11))
    rays[:, 0], rays[:, 1], rays[:, 2] = (x - center[0]) / scene_range, (y - center[1]) / scene_range, (z - center[2]) / scene_range
    rays[:, 3], rays[:, 4], rays[:, 5] = -(np.cos(phi) * np.cos(lam)), -(np.cos(phi) * np.sin(lam)), -np.sin(phi)
    rays[:, 7] = (float(max_alt) - float(min_alt)) / scene_range
    rays[:, 8:11] = np.asarray(sun_d, np.float32).astype(np.float64)
    return rays, np.stack([lat, lon], 1)


def within_one_ulp(got32, want64):
    """got (fp32) is float32(want) or one of its two fp32 neighbours, element-wise."""
    want32 = np.asarray(want64, np.float64).astype(np.float32)
    return np.abs(got32.astype(np.float64) - want32.astype(np.float64)) <= np.spacing(np.abs(want32)).astype(np.float64)


# ---- the scenes the host and the GPU tests share --------------------------------------------------------------------------------------
def scene(lat0, lon0, zone, xsize, ysize, res=0.5, min_alt=-24.0, max_alt=49.0, scene_range=210.0, frac=0.25):
    """A DSM grid around (lat0, lon0) whose x offset ends in ``frac`` (cell edges off the metre), with the scene's ECEF normalisation:
    center = the ECEF point under the grid's middle at the mean altitude."""
    from tests.test_dsm_host import utm_forward_np

    e0, n0 = utm_forward_np(lat0, lon0, zone)
    xoff = float(np.floor(e0)) + frac - float(np.floor(xsize * res / 2))
    yoff = float(np.floor(n0)) + float(np.ceil(ysize * res / 2))
    grid = (xoff, yoff, xsize, ysize, res)
    center = np.array(latlon_to_ecef(lat0, lon0, 0.5 * (min_alt + max_alt)))
    sun_d = np.array([0.3213938, 0.3830222, 0.8660254], np.float32)
    return dict(grid=grid, zone=zone, min_alt=min_alt, max_alt=max_alt, center=center, scene_range=scene_range, sun_d=sun_d)


def jax(xsize, ysize, **kw):  # Jacksonville, zone 17 north
    return scene(30.3, -81.7, 17, xsize, ysize, **kw)


def cape_town(xsize, ysize, **kw):  # zone 34 south: negative northings
    return scene(-33.9, 18.4, 34, xsize, ysize, **kw)
