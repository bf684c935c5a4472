"""fp64 numpy restatement of the sun rays (csrc/sun_rays.hip) and, in fp32, of the shading: the yardstick of the
HIP path.

A sun ray starts at the surface point ``P = o + d t`` of a primary ray and runs along the (east, north, up) sun vector turned into
the tangent frame of P's geodetic position; it ends where it reaches ``max_alt`` on that tangent plane.  The geodetic position is the
oracle's ``latlonalt_from_depth`` (sat_utils.ecef_to_latlon_custom in numpy fp64).  The scenes are those of ``tests/ortho_reference.py``;
their primary rays are its restated nadir rays and the depths the CPU oracle's render of a procedural field.
"""
import functools

import numpy as np
import torch

from oracle import satnerf_oracle as O
from tests import ortho_reference as R
from tests.ortho_reference import within_one_ulp  # noqa: F401  (re-exported)

A_WGS84, E2_WGS84 = 6378137.0, 8.1819190842622e-2 ** 2


def sun_direction(elevation_deg, azimuth_deg):
    """(east, north, up) unit vector towards the sun, fp64."""
    el, az = np.radians(float(elevation_deg)), np.radians(float(azimuth_deg))
    return np.array([np.sin(az) * np.cos(el), np.cos(az) * np.cos(el), np.sin(el)])


def tangent_frame(lat_deg, lon_deg):
    """(east, north, up), each (N, 3), of geodetic positions in degrees."""
    phi, lam = np.asarray(lat_deg) * (np.pi / 180.0), np.asarray(lon_deg) * (np.pi / 180.0)
    sp, cp, sl, cl = np.sin(phi), np.cos(phi), np.sin(lam), np.cos(lam)
    return np.stack([-sl, cl, np.zeros_like(sl)], 1), np.stack([-sp * cl, -sp * sl, cp], 1), np.stack([cp * cl, cp * sl, sp], 1)


def sun_rays_np(rays, depth, center, scene_range, max_alt, sun_d=None, bias_abs=0.0, bias_rel=0.0):
    """(rows (N, 11) float64 -- not yet rounded to fp32 --, valid (N,) bool, (lat, lon, alt) of the surface points).  ``rays`` / ``depth``
    are taken as they come (fp32 arrays are widened exactly); ``sun_d`` = the call's 3 values, rounded to fp32 as the C entry takes
    them, or None for the rays' own columns 8:11."""
    r = np.asarray(rays, np.float64)
    t = np.asarray(depth, np.float64).reshape(-1)
    n = r.shape[0]
    center = np.asarray(center, np.float64)
    s = r[:, 8:11] if sun_d is None else np.broadcast_to(np.asarray(sun_d, np.float32).astype(np.float64), (n, 3))
    with np.errstate(all="ignore"):
        P = r[:, 0:3] + r[:, 3:6] * t[:, None]
        E = P * float(scene_range) + center
        lat, lon, alt = O.latlonalt_from_depth(r, t, center, scene_range)
        length = np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2])
        hat = s / length[:, None]
        valid = np.isfinite(t) & np.isfinite(E).all(1) & np.isfinite(length) & (length > 0) & (hat[:, 2] > 0)
        e, nn, u = tangent_frame(lat, lon)
        direction = hat[:, 0:1] * e + hat[:, 1:2] * nn + hat[:, 2:3] * u
        L = (float(max_alt) - alt) / (hat[:, 2] * float(scene_range))
        near = float(bias_abs) + float(bias_rel) * (r[:, 7] - r[:, 6])
        far = np.maximum(near, L)
    rows = np.zeros((n, 11))
    rows[:, 0:3], rows[:, 3:6], rows[:, 6], rows[:, 7] = P, direction, near, far
    bad = ~valid
    rows[bad, 0:6], rows[bad, 6:8] = r[bad, 0:6], 0.0
    rows[:, 8:11] = s
    return rows, valid, (lat, lon, alt)


def shade_np(albedo, sky, vis):
    """(N, 3) fp32: q = 1 - v, k = q sky, irr = v + k, x = albedo irr, clamped to [0, 1], each operation rounded to fp32; NaN stays."""
    a, k, v = np.asarray(albedo, np.float32), np.asarray(sky, np.float32), np.asarray(vis, np.float32).reshape(-1, 1)
    with np.errstate(all="ignore"):
        q = np.float32(1) - v
        x = a * (v + q * k)
        return np.where(np.isnan(x), x, np.minimum(np.maximum(x, np.float32(0)), np.float32(1))).astype(np.float32)


# ---- the scenes the host and the GPU tests share --------------------------------------------------------------------------------------
SCENES = {"jax": (R.jax, 60.0, 40.0), "cape_town": (R.cape_town, 25.0, 140.0)}  # (grid maker, sun elevation, azimuth) in degrees
DENSITY_SCALE = 64.0  # on sigma_from_xyz.0.weight: the plain random field is a haze (every visibility in 0.75-0.80)


def oracle_params(feat):
    """``procedural_satnerf_params(feat, 4, seed=1)`` with the density row scaled: a field sharp enough to cast shadows."""
    p = O.procedural_satnerf_params(feat, 4, seed=1)
    p["sigma_from_xyz.0.weight"] = p["sigma_from_xyz.0.weight"] * DENSITY_SCALE
    return p


def oracle_transparency(params, rays, n_samples):
    """(depth (N,), transparency (N, S)) of the CPU oracle in fp32 for samples at the stratum midpoints (u = 0.5), no noise."""
    rays = torch.as_tensor(rays, dtype=torch.float32)
    n = rays.shape[0]
    with torch.no_grad():
        z = O.stratified_depths(rays, n_samples, torch.full((n, n_samples), 0.5))
        xyz = O.points_along(rays[:, 0:3], rays[:, 3:6], z).reshape(-1, 3)
        sigma = O.satnerf_mlp(params, xyz, torch.repeat_interleave(rays[:, 8:11], n_samples, 0), torch.zeros(n * n_samples, 4))[:, 3].view(n, n_samples)
        weights, transparency = O.alpha_composite(z, sigma, torch.zeros_like(sigma))
        return torch.sum(weights * z, -1), transparency


@functools.lru_cache(maxsize=None)
def scene(name, xsize=37, ysize=53, feat=256, n_samples=64):
    """A scene of ``ortho_reference`` with its sun, its restated nadir rays rounded to fp32 and the oracle's depths along them:
    dict(s, sun, rays (N, 11) fp32, depth (N,) fp32, primary (N,) fp32 = the oracle's transparency[:, -1] of the primary pass).
    Computed once and shared; the arrays are read-only."""
    make, el, az = SCENES[name]
    s = make(xsize, ysize)
    sun = sun_direction(el, az)
    s["sun_d"] = sun.astype(np.float32)
    rays = R.ortho_rays_np(**s)[0].astype(np.float32)
    depth, transparency = oracle_transparency(oracle_params(feat), rays, n_samples)
    out = dict(s=s, sun=sun, elevation=el, rays=rays, depth=depth.numpy(), primary=transparency[:, -1].numpy())
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
