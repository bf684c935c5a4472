"""DSM extraction on the GPU: depth -> UTM point cloud -> rasterised DSM -> registered DSM MAE.

The reference leaves the GPU here and calls pyproj / utm (``sat_utils.utm_from_latlon``), plyflatten
(``SatelliteDataset.get_dsm_from_nerf_prediction``) and GDAL / rasterio (``sat_utils.dsm_pointwise_diff``).  This module keeps
their names and argument order; geometry is fp64, the rasteriser is the HIP kernel of csrc/dsm.hip.  No file I/O: GeoTIFF reading
and writing stay with the caller (``DSM.transform`` is the affine the reference writes).  The reference's dsmr registration
(``compute_shift`` / ``apply_shift``, numba on the CPU there) is the HIP search of csrc/dsm_register.hip.  Several clouds fuse into
one DSM by a per-cell median / mean / min / max (``eval_s2p.project_cloud_into_utm_grid``; csrc/cloud_grid.hip, section 7.6).
A nadir DSM needs neither cloud nor splat: one vertical ray per cell of a UTM grid (``render_ortho_dsm``; csrc/ortho.hip, section 7.11),
whose inverse projection is also ``eval_s2p.lonlat_from_utm``.

The rasteriser follows this project's own grid / splat convention (include/satrender.h, sr_dsm_rasterize).  plyflatten cannot be
run here, so parity with it is not claimed.
"""
from __future__ import annotations

import dataclasses
import math

import torch

from . import ops


# ---- grid geometry (host) -------------------------------------------------------------------------------------------------------
def grid_from_bounds(xmin, xmax, ymin, ymax, resolution):
    """(xoff, yoff, xsize, ysize) of the grid around a cloud's bounds, as datasets/satellite.py:302-307 sizes it."""
    r = float(resolution)
    xoff = math.floor(xmin / r) * r
    xsize = int(1 + math.floor((xmax - xoff) / r))
    yoff = math.ceil(ymax / r) * r
    ysize = int(1 - math.floor((ymin - yoff) / r))
    return xoff, yoff, xsize, ysize


def grid_from_roi(roi):
    """(xoff, yoff, xsize, ysize, resolution) of an ``{aoi}_DSM.txt`` array (x, y, s, r), with the reference's ``yoff += s * r``
    (datasets/satellite.py:295-300): (x, y) is the lower-left corner, the grid's row 0 is its top."""
    vals = [float(v) for v in (roi.tolist() if hasattr(roi, "tolist") else roi)]
    if len(vals) != 4:
        raise ValueError(f"roi must hold the 4 values (x, y, s, r) of {{aoi}}_DSM.txt, got {len(vals)}")
    xoff, yoff, size, r = vals
    size = int(size)
    return xoff, yoff + size * r, size, size, r


def zone_string(number, letter):
    return f"{number}{letter}"


def utm_zone(lat, lon):
    """(zone number, band letter) of one point: the utm package's latlon_to_zone_number / latitude_to_zone_letter (lon normalised to
    [-180, 180), Norway and Svalbard exceptions).  Raises ValueError unless -80 <= lat <= 84 and lon is finite."""
    try:
        return ops.utm_zone(lat, lon)
    except RuntimeError as exc:
        raise ValueError(str(exc)) from None


def _zone_number(zone):
    z = int(zone) if not isinstance(zone, str) else int("".join(ch for ch in zone if ch.isdigit()) or 0)
    if not 1 <= z <= 60:
        raise ValueError(f"UTM zone must be in 1..60, got {zone!r}")
    return z


# ---- public API -----------------------------------------------------------------------------------------------------------------
def utm_from_latlon(lats, lons, zone=None):
    """``sat_utils.utm_from_latlon`` (sat_utils.py:97-113) on the GPU: (easts, norths) fp64 device tensors.  The zone is the first
    point's (as in the reference) unless ``zone`` (1..60 or e.g. "17R") is given.  False northing is 0 in both hemispheres (the
    reference's "+proj=utm +zone=<n><L>" has no +south): southern points get negative northings."""
    if not (torch.is_tensor(lats) and torch.is_tensor(lons) and lats.is_cuda and lons.is_cuda):
        raise ValueError("lats / lons must be GPU tensors: satnerf_amd has no CPU path")
    lats, lons = lats.reshape(-1).double(), lons.reshape(-1).double()
    if zone is None:
        if lats.numel() == 0:
            raise ValueError("no points: the UTM zone comes from the first point")
        zone = utm_zone(lats[0].item(), lons[0].item())[0]
    return ops.utm_from_latlon(lats, lons, _zone_number(zone))


def lonlat_from_utm(easts, norths, zone):
    """``eval_s2p.lonlat_from_utm`` (eval_s2p.py:37-44) on the GPU: (lons, lats) fp64 device tensors in degrees -- the reference's
    name and return order -- of UTM eastings / northings in ``zone`` (1..60 or e.g. "17R"), the inverse of :func:`utm_from_latlon`
    (csrc/ortho.hip).  False northing is 0 in both hemispheres: southern points carry negative northings."""
    if not (torch.is_tensor(easts) and torch.is_tensor(norths) and easts.is_cuda and norths.is_cuda):
        raise ValueError("easts / norths must be GPU tensors: satnerf_amd has no CPU path")
    lats, lons = ops.utm_to_latlon(easts.reshape(-1).double(), norths.reshape(-1).double(), _zone_number(zone))
    return lons, lats


@dataclasses.dataclass
class DSM:
    """A rasterised DSM.  ``dsm`` is (ysize, xsize) fp32 on the device, NaN where no point landed (the reference's plyflatten returns
    (h, w, 1) and writes ``[:, :, 0]``); ``weight`` the per-cell sum of splat weights (the point count for sigma = inf).  Cell (j, c)
    covers east [xoff + c r, xoff + (c+1) r) and north (yoff - (j+1) r, yoff - j r]."""
    dsm: torch.Tensor
    weight: torch.Tensor
    xoff: float
    yoff: float
    resolution: float
    zone: str
    roi: tuple | None = None

    @property
    def transform(self):
        """The GeoTIFF affine (a, b, c, d, e, f) = (r, 0, xoff, 0, -r, yoff) (datasets/satellite.py:333)."""
        return (self.resolution, 0.0, self.xoff, 0.0, -self.resolution, self.yoff)


def dsm_from_depth(rays, depth, center, scene_range, roi=None, resolution=0.5, radius=1, sigma=float("inf"), zone=None):
    """``SatelliteDataset.get_dsm_from_nerf_prediction`` (datasets/satellite.py:277-338) without file I/O.

    rays (N, >=6) fp32 and depth (N,) or (N, 1) fp32 on the GPU; ``center`` (3,) / ``scene_range`` the dataset's ECEF normalisation.
    ``roi`` = the (x, y, s, r) array of ``{aoi}_DSM.txt`` (its r replaces ``resolution``); without it the grid spans the cloud.
    ``radius`` in 0..4, ``sigma`` > 0 or inf (plyflatten's arguments; the reference uses 1 and inf).  Points that are not finite, or
    outside the grid, contribute nothing.  Returns a :class:`DSM`; the raster is bitwise reproducible and independent of point order."""
    if not (torch.is_tensor(rays) and torch.is_tensor(depth) and rays.is_cuda and depth.is_cuda):
        raise ValueError("rays / depth must be GPU tensors: satnerf_amd has no CPU path")
    if rays.dim() != 2 or rays.shape[1] < 6 or depth.numel() != rays.shape[0]:
        raise ValueError(f"rays must be (N, >=6) with one depth per ray, got {tuple(rays.shape)} and {tuple(depth.shape)}")
    if not 0 <= int(radius) <= 4:
        raise ValueError(f"radius must be in 0..4, got {radius}")
    if not float(sigma) > 0:
        raise ValueError(f"sigma must be > 0 or inf, got {sigma}")
    rays = rays if rays.dtype == torch.float32 and rays.stride(-1) == 1 else rays.float().contiguous()
    depth = depth.reshape(-1).float().contiguous()
    zone_in = 0 if zone is None else _zone_number(zone)
    east, north, alt, zone_out = ops.depth_to_utm(rays, depth, center, scene_range, zone_in)
    n = rays.shape[0]
    if roi is not None:
        xoff, yoff, xsize, ysize, resolution = grid_from_roi(roi)
        meta = zone_out.cpu().tolist()  # the zone string
        if xsize < 1 or resolution <= 0:
            raise ValueError(f"zero-size DSM grid from roi {list(roi)}")
    else:
        if n == 0:
            raise ValueError("no rays: the DSM grid cannot be sized without a roi")
        # one device-to-host copy: the four bounds (fp64) and the zone (2 int32) side by side
        buf = torch.empty(5, dtype=torch.int64, device=rays.device)
        ops.dsm_bounds(east, north, alt, out=buf[:4].view(torch.float64))
        buf[4:].view(torch.int32).copy_(zone_out)
        host = buf.cpu()
        xmin, xmax, ymin, ymax = host[:4].view(torch.float64).tolist()
        meta = host[4:].view(torch.int32).tolist()
        if not all(math.isfinite(v) for v in (xmin, xmax, ymin, ymax)):
            raise ValueError("zero-size DSM grid: no usable point")
        xoff, yoff, xsize, ysize = grid_from_bounds(xmin, xmax, ymin, ymax, resolution)
    if n > 0 and meta[0] == 0:
        raise ValueError("the first ray's point is not finite or lies outside latitudes [-80, 84]: pass zone= explicitly")
    dsm, weight = ops.dsm_rasterize(east, north, alt, xoff, yoff, resolution, xsize, ysize, int(radius), float(sigma))
    number = meta[0] or zone_in
    zone_str = zone_string(number, chr(meta[1]) if meta[1] else "") if number else ""  # "" only for zero rays without zone=
    return DSM(dsm, weight, float(xoff), float(yoff), float(resolution), zone_str, None if roi is None else tuple(float(v) for v in roi))


def _raster(x, name):
    """The (H, W) device raster of a :class:`DSM` or a tensor, as fp64 (an exact widening of fp32)."""
    t = x.dsm if isinstance(x, DSM) else x
    if not (torch.is_tensor(t) and t.is_cuda):
        raise ValueError(f"{name} must be a DSM or a GPU tensor: satnerf_amd has no CPU path")
    if t.dim() != 2 or t.numel() == 0:
        raise ValueError(f"{name} must be a non-empty (H, W) raster, got shape {tuple(t.shape)}")
    if not t.dtype.is_floating_point:
        raise ValueError(f"{name} must be floating point, got {t.dtype}")
    return t.to(torch.float64).contiguous()


def _check_irange(irange):
    if not (isinstance(irange, int) and 1 <= irange <= 16):
        raise ValueError(f"irange must be an int in 1..16, got {irange!r}")


def _coefs(out):
    """(dx, dy, a, b) from sr_dsm_compute_shift's packed result, in one device-to-host copy."""
    host = out.cpu()
    coef = host[:8].view(torch.float64).tolist()
    dx, dy = host[8:].view(torch.int32).tolist()
    if coef[7] == 0:
        raise ValueError("no valid (finite) pixel pair at the registered shift: the registration is undefined")
    return dx, dy, coef[0], coef[1]


def compute_shift(ref, sec, scaling=True, irange=5):
    """``dsmr.compute_shift`` (dsmr.py:163-190) on the GPU: the integer shift (dx, dy) and the Z map z -> a z + b that register ``sec``
    on ``ref`` by a coarse-to-fine NCC search (csrc/dsm_register.hip).  ``ref`` / ``sec`` are DSMs or (H, W)
    device rasters of any float dtype; their shapes may differ.  a = sig_ref / sig_sec if ``scaling`` else 1, b = mu_ref - mu_sec a
    at the shift.  Returns (dx, dy, a, b) as Python numbers after one device-to-host copy; raises ValueError when no finite pixel
    pair exists at the chosen shift (where the reference raises ZeroDivisionError)."""
    _check_irange(irange)
    u, v = _raster(ref, "ref"), _raster(sec, "sec")
    out, _, _ = ops.dsm_compute_shift(u, v, irange=irange, scaling=scaling)
    return _coefs(out)


def apply_shift(sec, dx=0, dy=0, a=1.0, b=0.0):
    """``dsmr.apply_shift`` (dsmr.py:193-215) without file I/O: out[j, i] = a sec[j + dy, i + dx] + b over sec's extent, NaN where
    the read falls outside sec, evaluated in fp64 and returned as an fp32 device tensor (the reference's raster dtype)."""
    v = _raster(sec, "sec")
    shift = torch.tensor([int(dx), int(dy)], dtype=torch.int32).to(v.device)
    coef = torch.tensor([float(a), float(b)], dtype=torch.float64).to(v.device)
    return ops.dsm_apply_shift(v, shift, coef)


def dsm_mae(pred, gt, gt_mask=None, register="z"):
    """The DSM MAE of ``sat_utils.dsm_pointwise_diff`` + ``np.nanmean(abs(err))``.  Water cells (mask class 9) become NaN in ``pred``
    first.  ``pred`` is a :class:`DSM` built with ``roi=`` or a (H, W) device tensor already on the ground truth's grid; ``gt`` (H, W)
    and ``gt_mask`` (H, W) live on the same device.  No cropping (the reference's gdal.Translate) happens here.

    register="z" (default): the branch the reference takes without dsmr (sat_utils.py:162-171): shift = nanmean(gt - pred),
    rdsm = pred + shift, err = rdsm - gt, all fp64.  Returns (mae, err, rdsm, shift): mae / shift as floats, err / rdsm as fp64
    device tensors.

    register="xyz": the dsmr branch, i.e. the metric the reference prints (sat_utils.py:172-177): (dx, dy, a, b) =
    compute_shift(gt, pred, scaling=False), rdsm = apply_shift(pred, dx, dy, a, b) (fp32), err = rdsm - gt (fp32 for an fp32 gt),
    mae = nanmean(|err|) (summed in fp64).  Returns (mae, err, rdsm, (dx, dy, a, b)); registration runs entirely on the device and
    the result comes back in one copy."""
    if register not in ("z", "xyz"):
        raise ValueError(f"register must be 'z' or 'xyz', got {register!r}")
    if isinstance(pred, DSM):
        if pred.roi is None:
            raise ValueError("pred was not built on the ROI grid: call dsm_from_depth(..., roi=...) (cropping is not implemented)")
        pred = pred.dsm
    for name, t in (("pred", pred), ("gt", gt), ("gt_mask", gt_mask)):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise ValueError(f"{name} must be a GPU tensor: satnerf_amd has no CPU path")
    if pred.shape != gt.shape or pred.dim() != 2:
        raise ValueError(f"pred {tuple(pred.shape)} is not on the ground truth's (H, W) grid {tuple(gt.shape)}")
    if gt_mask is not None and gt_mask.shape != gt.shape:
        raise ValueError(f"gt_mask {tuple(gt_mask.shape)} does not match gt {tuple(gt.shape)}")
    if register == "xyz":
        return _dsm_mae_xyz(pred, gt, gt_mask)
    p, g = pred.double().clone(), gt.to(pred.device).double()
    if gt_mask is not None:
        p[gt_mask == 9] = float("nan")
    shift = torch.nanmean(g - p)
    rdsm = p + shift
    err = rdsm - g
    mae = torch.nanmean(err.abs())
    return mae.item(), err, rdsm, shift.item()


def _dsm_mae_xyz(pred, gt, gt_mask):
    p = _raster(pred, "pred").clone()
    g = gt.to(pred.device)
    if gt_mask is not None:
        p[gt_mask == 9] = float("nan")
    out, _, _ = ops.dsm_compute_shift(_raster(g, "gt"), p, irange=5, scaling=False)
    rdsm = ops.dsm_apply_shift(p, out[8:].view(torch.int32), out[:8].view(torch.float64))
    err = rdsm.to(torch.promote_types(torch.float32, g.dtype)) - g
    mae = torch.nanmean(err.abs().double())
    transform = _coefs(out)  # raises if the registration is undefined
    return mae.item(), err, rdsm, transform


# ---- cloud fusion ------------------------------------------------------------------------------------------
CLOUD_MODES = ("min", "max", "avg", "med")


def _check_mode(mode):
    if mode not in CLOUD_MODES:
        raise ValueError(f"mode must be one of {CLOUD_MODES}, got {mode!r}")


def project_cloud_into_utm_grid(xyz, bb, definition, mode, mask=None):
    """``eval_s2p.project_cloud_into_utm_grid`` (eval_s2p.py:175-226) on the GPU: the (map_h, map_w) fp64 device raster whose cell holds
    the ``mode`` ("min", "max", "avg" or "med") of the altitudes of the points that round to it, NaN where none did, already flipped
    so that row 0 is north.  ``xyz`` is an (N, >=3) device tensor (east, north, alt), widened to fp64; ``bb`` = [xmin, xmax, ymin,
    ymax]; map_w = int(round((xmax - xmin) / definition)) + 1 and map_h likewise.  ``mask`` is accepted and ignored: the reference
    assigns it and never reads it.  Departures: a ``mode`` outside the four raises ValueError (the reference silently takes the
    "med" branch), and a point with a non-finite coordinate or altitude contributes nothing.  min / max / med equal the reference's
    bit for bit; every mode is independent of point order."""
    _check_mode(mode)
    if not (torch.is_tensor(xyz) and xyz.is_cuda):
        raise ValueError("xyz must be a GPU tensor: satnerf_amd has no CPU path")
    if xyz.dim() != 2 or xyz.shape[1] < 3:
        raise ValueError(f"xyz must be (N, >=3), got {tuple(xyz.shape)}")
    bb = [float(v) for v in bb]
    if len(bb) != 4:
        raise ValueError(f"bb must hold [xmin, xmax, ymin, ymax], got {len(bb)} values")
    definition = float(definition)
    map_w = int(round((bb[1] - bb[0]) / definition)) + 1
    map_h = int(round((bb[3] - bb[2]) / definition)) + 1
    cols = xyz[:, :3].to(torch.float64).t().contiguous()
    out, _ = ops.cloud_grid(cols[0], cols[1], cols[2], bb[0], bb[2], definition, map_w, map_h, rule="nearest", mode=mode)
    return out


def _cat(x, name):
    parts = list(x) if isinstance(x, (list, tuple)) else [x]
    for t in parts:
        if not (torch.is_tensor(t) and t.is_cuda):
            raise ValueError(f"{name} must be a GPU tensor or a list of GPU tensors: satnerf_amd has no CPU path")
    if not parts:
        raise ValueError(f"{name} is an empty list")
    parts = [t.reshape(-1).to(torch.float64) for t in parts]
    return parts[0].contiguous() if len(parts) == 1 else torch.cat(parts)


def dsm_from_clouds(east, north, alt, roi=None, resolution=0.5, mode="med", zone=""):
    """Fuse UTM clouds into one :class:`DSM` by the per-cell ``mode`` of their altitudes (csrc/cloud_grid.hip) on the DSM grid of
    :func:`dsm_from_depth`: cell (j, c) = (floor((yoff - north) / r), floor((east - xoff) / r)).  ``east`` / ``north`` / ``alt`` are
    each a device tensor or a list of device tensors (one per cloud, concatenated); ``roi`` / ``resolution`` size the grid exactly as
    dsm_from_depth does.  ``dsm`` is fp32 (the median / mean / min / max taken in fp64), ``weight`` the points per cell as fp32.  Points
    that are not finite, or outside the grid, contribute nothing; the raster is bitwise independent of point and cloud order."""
    _check_mode(mode)
    east, north, alt = _cat(east, "east"), _cat(north, "north"), _cat(alt, "alt")
    if not east.shape == north.shape == alt.shape:
        raise ValueError(f"east / north / alt must hold one value per point each, got {east.numel()}, {north.numel()}, {alt.numel()}")
    if roi is not None:
        xoff, yoff, xsize, ysize, resolution = grid_from_roi(roi)
        if xsize < 1 or resolution <= 0:
            raise ValueError(f"zero-size DSM grid from roi {list(roi)}")
    else:
        if east.numel() == 0:
            raise ValueError("no points: the DSM grid cannot be sized without a roi")
        xmin, xmax, ymin, ymax = ops.dsm_bounds(east, north, alt).cpu().tolist()
        if not all(math.isfinite(v) for v in (xmin, xmax, ymin, ymax)):
            raise ValueError("zero-size DSM grid: no usable point")
        xoff, yoff, xsize, ysize = grid_from_bounds(xmin, xmax, ymin, ymax, resolution)
    out, count = ops.cloud_grid(east, north, alt, xoff, yoff, resolution, xsize, ysize, rule="floor", mode=mode)
    return DSM(out.float(), count.float(), float(xoff), float(yoff), float(resolution), str(zone),
               None if roi is None else tuple(float(v) for v in roi))


def _rendered_depth(models, rays, ts, args, geometry_only):
    """the per-ray depth of a whole image: from the full evaluation render, or (``geometry_only``) from the depth-only render
    (``rendering.render_depth``: trunk and density only, one launch per pass)"""
    from .rendering import render_depth, render_image_outputs

    with torch.no_grad():
        return (render_depth if geometry_only else render_image_outputs)(models, rays, ts, args)["depth"]


def render_fused_dsm(models, views, args, center, scene_range, mode="med", geometry_only=False, **dsm_kwargs):
    """Render every view and fuse the clouds into one DSM: per ``(rays, ts)`` of ``views``, ``render_image_outputs(...)["depth"]`` ->
    ``ops.depth_to_utm`` -> :func:`dsm_from_clouds` (``dsm_kwargs``: roi, resolution).  The UTM zone is the first view's first
    point's and is handed to every later view, so a scene on a zone edge never mixes projections.  With ``roi=`` the result feeds
    :func:`dsm_mae` unchanged.  ``geometry_only``: the depths come from ``rendering.render_depth`` (no colour, sun or uncertainty head)."""
    _check_mode(mode)
    views = list(views)
    if not views:
        raise ValueError("no views")
    clouds, number, zone_str = [], 0, ""
    for rays, ts in views:
        if not (torch.is_tensor(rays) and rays.is_cuda):
            raise ValueError("rays must be GPU tensors: satnerf_amd has no CPU path")
        depth = _rendered_depth(models, rays, ts, args, geometry_only)
        rays32 = rays if rays.dtype == torch.float32 and rays.stride(-1) == 1 else rays.float().contiguous()
        east, north, alt, zone_out = ops.depth_to_utm(rays32, depth.reshape(-1).float().contiguous(), center, scene_range, number)
        if not number:
            meta = zone_out.cpu().tolist()
            if meta[0] == 0:
                raise ValueError("the first view's first point is not finite or lies outside latitudes [-80, 84]")
            number, zone_str = meta[0], zone_string(meta[0], chr(meta[1]) if meta[1] else "")
        clouds.append((east, north, alt))
    return dsm_from_clouds([c[0] for c in clouds], [c[1] for c in clouds], [c[2] for c in clouds], mode=mode, zone=zone_str, **dsm_kwargs)


def render_dsm(models, rays, ts, args, center, scene_range, geometry_only=False, **dsm_kwargs):
    """The create_satnerf_dsm flow in one call: ``render_image_outputs(...)["depth"]`` -> :func:`dsm_from_depth`.  ``geometry_only``:
    the depth comes from ``rendering.render_depth`` instead (a DSM needs nothing else of the render)."""
    depth = _rendered_depth(models, rays, ts, args, geometry_only)
    return dsm_from_depth(rays, depth, center, scene_range, **dsm_kwargs)


# ---- nadir DSM -----------------------------------------------------------------------------------------------
def ortho_dsm_from_depth(depth, grid, max_alt, scene_range, zone="", roi=None):
    """The :class:`DSM` of the depths rendered along ``data.ortho_rays(grid, ...)``: one altitude per cell, no cloud and no splat.
    ``depth`` holds ysize * xsize values in grid order on the GPU; alt = max_alt - float64(depth) * scene_range, stored as fp32, NaN
    where the depth is not finite; ``weight`` is 1 where the cell is valid and 0 elsewhere.  ``grid`` = (xoff, yoff, xsize, ysize,
    resolution); ``roi`` (the ``{aoi}_DSM.txt`` array the grid came from) is recorded so that :func:`dsm_mae` takes the result."""
    from .data import _ortho_grid

    xoff, yoff, xsize, ysize, r = _ortho_grid(grid)
    if not (torch.is_tensor(depth) and depth.is_cuda):
        raise ValueError("depth must be a GPU tensor: satnerf_amd has no CPU path")
    if depth.numel() != xsize * ysize:
        raise ValueError(f"depth must hold one value per cell of the {ysize} x {xsize} grid, got {tuple(depth.shape)}")
    d = depth.reshape(ysize, xsize).to(torch.float64)
    valid = torch.isfinite(d)
    alt = torch.where(valid, float(max_alt) - d * float(scene_range), float("nan")).to(torch.float32)
    return DSM(alt, valid.to(torch.float32), xoff, yoff, r, str(zone), None if roi is None else tuple(float(v) for v in roi))


def _zone_of_center(center, device):
    """(number, letter) of the UTM zone the scene centre (ECEF) lies in, through the ECEF -> geodetic kernel (one small read-back)."""
    ray = torch.zeros(1, 6, dtype=torch.float32, device=device)
    lat, lon, _ = ops.latlonalt_from_depth(ray, torch.zeros(1, dtype=torch.float32, device=device), center, 1.0)
    return utm_zone(*torch.stack([lat[0], lon[0]]).cpu().tolist())


def render_ortho_dsm(models, ts, args, center, scene_range, min_alt, max_alt, sun_d, roi=None, grid=None, zone=None, geometry_only=False,
                     shadows=None):
    """Render a nadir DSM of a trained field: ``data.ortho_rays`` over the grid -> ``render_image_outputs`` (once, no grad) ->
    :func:`ortho_dsm_from_depth`.  Every cell gets exactly one altitude, sampled along its own vertical, so the raster has no holes
    behind leaning buildings and involves no splat convention.

    Exactly one of ``roi`` (the ``{aoi}_DSM.txt`` array (x, y, s, r), see :func:`grid_from_roi`) and ``grid`` (xoff, yoff, xsize,
    ysize, resolution) sizes the raster.  ``ts``: an int (one transient-embedding index for every ray) or an (ysize * xsize,) tensor.
    ``center`` / ``scene_range`` / ``min_alt`` / ``max_alt``: the scene's ECEF normalisation and altitude bounds; ``sun_d``: the sun
    direction of the render.  ``zone`` (1..60 or "17R") defaults to the zone of the scene centre.

    Returns (DSM, outputs).  ``outputs`` is the dict of ``render_image_outputs``; its per-ray tensors are in grid order, so
    ``outputs["rgb"].view(ysize, xsize, 3)`` is the true-ortho colour image, and likewise "albedo" (.., 3), "sun" (.., 1), "beta" (.., 1),
    "depth" / "acc" (ysize, xsize).  Cells outside the footprint the field was trained on are extrapolation: no footprint or visibility
    mask is built.  ``geometry_only``: the render is ``rendering.render_depth`` and ``outputs`` holds "depth" and "acc" only.

    ``shadows="geometry"`` answers "which cells are in shadow at this sun position?": it adds ``outputs["sun_geo"]`` (ysize * xsize,), the
    transparency of the learned density between each cell's rendered surface and the sun at ``sun_d``
    (``rendering.render_sun_visibility`` on the rendered depths; NaN where the sun ray is invalid), and with the full render also
    ``outputs["rgb_geo"]`` (.., 3) = ``ops.sun_shade`` of "albedo", "sky" and "sun_geo", a per-pixel relighting of the composited
    albedo.  The DSM and every other output are those of ``shadows=None``."""
    from .data import _ortho_grid, ortho_rays
    from .rendering import render_depth, render_image_outputs, render_sun_visibility

    if shadows not in (None, "geometry"):
        raise ValueError(f"shadows must be None or 'geometry', got {shadows!r}")
    if (roi is None) == (grid is None):
        raise ValueError("exactly one of roi= and grid= sizes the DSM")
    grid = _ortho_grid(grid_from_roi(roi) if roi is not None else grid)
    t0 = models["t"].weight if hasattr(models["t"], "weight") else models["t"]
    if not (torch.is_tensor(t0) and t0.is_cuda):
        raise ValueError("the models must live on the GPU: satnerf_amd has no CPU path")
    dev = t0.device
    with torch.cuda.device(dev):
        if zone is None:
            number, letter = _zone_of_center(center, dev)
            zone = zone_string(number, letter)
        n = grid[2] * grid[3]
        if torch.is_tensor(ts):
            if ts.numel() != n:
                raise ValueError(f"ts must be an int or hold one index per cell ({n}), got {tuple(ts.shape)}")
            ts = ts.to(dev)
        else:
            ts = torch.full((n,), int(ts), dtype=torch.int64, device=dev)
        rays = ortho_rays(grid, zone, min_alt, max_alt, center, scene_range, sun_d, device=dev)
        with torch.no_grad():
            if geometry_only:
                outputs = {k: v for k, v in render_depth(models, rays, ts, args).items() if k in ("depth", "acc")}
            else:
                outputs = render_image_outputs(models, rays, ts, args)
            if shadows == "geometry":
                outputs["sun_geo"] = render_sun_visibility(models, rays, ts, args, center, scene_range, max_alt, sun_d=sun_d,
                                                           depth=outputs["depth"])["sun_geo"]
                if not geometry_only:
                    outputs["rgb_geo"] = ops.sun_shade(outputs["albedo"], outputs["sky"], outputs["sun_geo"])
        return ortho_dsm_from_depth(outputs["depth"], grid, max_alt, scene_range, zone=str(zone), roi=roi), outputs


# ---- a DSM as geometry ---------------------------------------------------------------------------------------
def _surface(dsm, name="dsm"):
    """The (ysize, xsize) fp32 device raster of a :class:`DSM`, contiguous."""
    if not isinstance(dsm, DSM):
        raise ValueError(f"{name} must be a DSM (raster, xoff, yoff, resolution, zone), got {type(dsm).__name__}")
    t = dsm.dsm
    if not (torch.is_tensor(t) and t.is_cuda):
        raise ValueError(f"{name}.dsm must be a GPU tensor: satnerf_amd has no CPU path")
    if t.dim() != 2 or t.numel() == 0:
        raise ValueError(f"{name}.dsm must be a non-empty (ysize, xsize) raster, got shape {tuple(t.shape)}")
    if not float(dsm.resolution) > 0:
        raise ValueError(f"{name}.resolution must be > 0, got {dsm.resolution}")
    return t.float().contiguous()


def cast_rays(dsm, rays, center, scene_range, zone=None, accelerate=True):
    """Where each ray meets a DSM taken as geometry (csrc/heightfield.hip): every finite cell of ``dsm`` (a :class:`DSM`) is a solid
    column, a NaN cell is empty, and a ray is the straight chord between the UTM images of its near and far points, walked through the
    raster's cells until it enters a column.  ``rays`` (N, >=8) fp32 on the GPU in the scene frame of ``center`` / ``scene_range``;
    ``zone`` (1..60 or "17R") defaults to the DSM's.  Returns ``{"depth": (N,) fp32 in the rays' own units, NaN on a miss, "cell": (N,)
    int32 = j * xsize + c of the column that was hit, -1 on a miss, "hit": (N,) bool}``: the depth a DSM implies in a view's pixels,
    occlusion included, and the cell each pixel sees.  A ray with a non-finite end or far < near is a miss.  ``accelerate=False`` takes
    the plain walk instead of the two-level one; the results are the same bits."""
    hgt = _surface(dsm)
    if not (torch.is_tensor(rays) and rays.is_cuda):
        raise ValueError("rays must be a GPU tensor: satnerf_amd has no CPU path")
    if rays.dim() != 2 or rays.shape[1] < 8:
        raise ValueError(f"rays must be (N, >=8): origin, direction, near, far, got {tuple(rays.shape)}")
    if not float(scene_range) > 0:
        raise ValueError(f"scene_range must be > 0, got {scene_range}")
    if zone is None and not dsm.zone:
        raise ValueError("the DSM carries no UTM zone: pass zone= explicitly")
    number = _zone_number(dsm.zone if zone is None else zone)
    ctr = [float(v) for v in (center.tolist() if hasattr(center, "tolist") else center)]
    r32 = rays if rays.dtype == torch.float32 and rays.stride(1) == 1 else rays.float().contiguous()
    with torch.cuda.device(hgt.device):
        depth, cell, _, _ = ops.heightfield_cast(hgt, dsm.resolution, rays=r32, center=ctr, scene_range=scene_range, zone=number,
                                                 xoff=dsm.xoff, yoff=dsm.yoff, accelerate=accelerate)
    return {"depth": depth, "cell": cell, "hit": cell >= 0}


def shadow_mask(dsm, sun_d, bias=0.0, accelerate=True):
    """The shadows a DSM casts on itself under one sun direction: an (ysize, xsize) fp32 device raster, 1.0 lit, 0.0 shadowed, NaN where
    the cell is NaN.  From every finite cell a ray leaves the cell centre at its height + ``bias`` (metres, >= 0) along ``sun_d`` (3
    values: east, north, up, as ``data.sun_direction`` returns them; not necessarily a unit vector) and is walked through the raster up
    to its highest cell; the cell it starts in never shades itself.  The grid is taken as flat.  Raises ValueError for a sun at or below
    the horizon."""
    hgt = _surface(dsm)
    sun = [float(v) for v in (sun_d.tolist() if hasattr(sun_d, "tolist") else sun_d)]
    if len(sun) != 3 or not all(math.isfinite(v) for v in sun):
        raise ValueError(f"sun_d must hold 3 finite values (east, north, up), got {sun}")
    if not sun[2] > 0:
        raise ValueError(f"the sun is at or below the horizon (up = {sun[2]}): there is no shadow mask to cast")
    if not (math.isfinite(float(bias)) and float(bias) >= 0):
        raise ValueError(f"bias must be finite and >= 0 metres, got {bias}")
    with torch.cuda.device(hgt.device):
        return ops.heightfield_shadow(hgt, dsm.resolution, sun, bias=float(bias), accelerate=accelerate)


def sun_visibility_from_dsm(dsm, rays, depth, center, scene_range, max_alt, sun_d=None, bias=None, n_samples=None):
    """The DSM's shadows in a view's own pixels, shaped like ``rendering.render_sun_visibility``'s "sun_geo": ``data.sun_rays`` from the
    rendered surface points (``rays`` (N, >=11), ``depth`` (N,); ``sun_d``, ``bias`` and ``n_samples`` as there) followed by
    :func:`cast_rays`.  Returns (N,) fp32: 1 where the sun ray misses the DSM, 0 where it meets it, NaN for the rows ``sun_rays`` calls
    invalid.  The sun rays end at ``max_alt``: a DSM column above it cannot shade."""
    from .data import sun_rays

    sr, valid = sun_rays(rays, depth, center, scene_range, max_alt, sun_d=sun_d, bias=bias, n_samples=n_samples, return_valid=True)
    hit = cast_rays(dsm, sr, center, scene_range)["hit"]
    lit = torch.where(hit, 0.0, 1.0).to(torch.float32)
    return torch.where(valid, lit, torch.full_like(lit, float("nan")))


# ---- a view's pixels on the DSM grid ---------------------------------------------------------------------------
def _ortho_image(image, name="image"):
    """An (H, W, C) GPU image, uint8 or fp32, C in 1..4; (H, W) gains a channel."""
    if not torch.is_tensor(image) or image.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{name} must be a uint8 or float32 tensor, got {getattr(image, 'dtype', type(image).__name__)}")
    if image.dim() == 2:
        image = image.unsqueeze(-1)
    if image.dim() != 3 or image.numel() == 0 or not 1 <= image.shape[2] <= 4:
        raise ValueError(f"{name} must be a non-empty (H, W, C) or (H, W) image with C in 1..4, got {tuple(image.shape)}")
    if not image.is_cuda:
        raise ValueError(f"{name} must be a GPU tensor: satnerf_amd has no CPU path")
    return image.contiguous()


def _ortho_args(dsm, mode, bias, zone):
    """The UTM zone number of the call, after the checks that need no tensor."""
    if not isinstance(dsm, DSM):
        raise ValueError(f"dsm must be a DSM (raster, xoff, yoff, resolution, zone), got {type(dsm).__name__}")
    if mode not in ops.ORTHO_MODES:
        raise ValueError(f"mode must be one of {sorted(ops.ORTHO_MODES)}, got {mode!r}")
    if not (math.isfinite(float(bias)) and float(bias) >= 0):
        raise ValueError(f"bias must be finite and >= 0 metres, got {bias}")
    if zone is None and not dsm.zone:
        raise ValueError("the DSM carries no UTM zone: pass zone= explicitly")
    return _zone_number(dsm.zone if zone is None else zone)


def orthorectify(dsm, image, rpc, mode="bilinear", bias=0.0, accelerate=True, zone=None):
    """One view's pixels on the grid of a DSM taken as geometry (csrc/orthorectify.hip).  Every finite cell's centre at the cell's height
    is projected through ``rpc`` (an "rpcm"-format dict) into ``image`` ((H, W, C) or (H, W), uint8 -- read as value / 255 -- or fp32, on
    the GPU; pixel centres at integer (col, row)); the line of sight from the cell (lifted by ``bias`` >= 0 metres) towards the camera is
    walked through the raster up to its highest cell, the cell itself passed through; a cell that is seen takes the image's colour there
    by ``mode`` "nearest", "bilinear" or "bicubic" (Keys, a = -0.5; indices clamped to the image).  ``zone`` (1..60 or "17R") defaults
    to the DSM's.  Returns ``{"color": (ysize, xsize, C) fp32, NaN unless visible, "status": (ysize, xsize) uint8 -- 0 empty cell, 1
    visible, 2 occluded by the DSM, 3 outside the image --, "colrow": (ysize, xsize, 2) fp64 (col, row), NaN for an empty cell,
    "visible": (ysize, xsize) bool}``.  ``accelerate=False`` takes the plain walk: the same bits."""
    number = _ortho_args(dsm, mode, bias, zone)
    image = _ortho_image(image)
    hgt = _surface(dsm)
    with torch.cuda.device(hgt.device):
        color, status, colrow = ops.orthorectify(hgt, dsm.resolution, dsm.xoff, dsm.yoff, number, rpc, image, mode=mode, bias=float(bias),
                                                 accelerate=accelerate)
    return {"color": color, "status": status, "colrow": colrow, "visible": status == 1}


def ortho_mosaic(dsm, views, mode="bilinear", bias=0.0, min_views=1, accelerate=True, zone=None):
    """The mean colour of several views on a DSM's grid: :func:`orthorectify` of every ``(image, rpc)`` of ``views`` (images with the same
    channel count), accumulated per cell over the views that see it, in the order given and without atomics: bitwise repeatable.
    Returns ``{"color": (ysize, xsize, C) fp32 = fp64 sum / count rounded once, NaN where fewer than ``min_views`` views see the cell,
    "count": (ysize, xsize) int32 = the views that see each cell}``: the footprint and coverage mask of the imagery on this grid."""
    number = _ortho_args(dsm, mode, bias, zone)
    if int(min_views) < 1:
        raise ValueError(f"min_views must be >= 1, got {min_views}")
    views = list(views)
    if not views:
        raise ValueError("views is empty: a mosaic needs at least one (image, rpc)")
    views = [(_ortho_image(image, f"views[{k}] image"), rpc) for k, (image, rpc) in enumerate(views)]
    hgt = _surface(dsm)
    channels = views[0][0].shape[2]
    if any(image.shape[2] != channels for image, _ in views):
        raise ValueError(f"the views' images must have the same channel count, got {[int(image.shape[2]) for image, _ in views]}")
    ysize, xsize = hgt.shape
    with torch.cuda.device(hgt.device):
        total = torch.zeros(ysize, xsize, channels, dtype=torch.float64, device=hgt.device)
        count = torch.zeros(ysize, xsize, dtype=torch.int32, device=hgt.device)
        maxima = ops.heightfield_blockmax(hgt)
        scratch = torch.empty(ops.orthorectify_scratch(xsize, ysize), dtype=torch.uint8, device=hgt.device)
        bufs = None
        for image, rpc in views:
            bufs = ops.orthorectify(hgt, dsm.resolution, dsm.xoff, dsm.yoff, number, rpc, image, mode=mode, bias=float(bias),
                                    accelerate=accelerate, maxima=maxima, scratch=scratch, sum=total, count=count,
                                    **({} if bufs is None else dict(color=bufs[0], status=bufs[1], colrow=bufs[2])))
        mean = (total / count.unsqueeze(-1).to(torch.float64)).to(torch.float32)
        mean = torch.where((count >= int(min_views)).unsqueeze(-1), mean, torch.full_like(mean, float("nan")))
    return {"color": mean, "count": count}


def orthorectify_dataset(dsm, root_dir, img_dir, split="train", img_downscale=1.0, reader=None, **kw):
    """:func:`ortho_mosaic` of a dataset's split: the images ``data.load_rays`` and ``data.load_colors`` share (``train.txt`` /
    ``test.txt`` under ``root_dir``, pixels under ``img_dir``, ``reader`` as in ``data.load_colors``), each at its down-scaled size with
    its RPC rescaled by ``1 / img_downscale`` (``data.rescale_rpc``).  ``**kw`` goes to :func:`ortho_mosaic`."""
    from .data import _split_images, load_colors, rescale_rpc

    if not (isinstance(dsm, DSM) and torch.is_tensor(dsm.dsm)):
        raise ValueError(f"dsm must be a DSM (raster, xoff, yoff, resolution, zone), got {type(dsm).__name__}")
    metas, _ = _split_images(root_dir, split, img_downscale)
    rgbs = load_colors(root_dir, img_dir, split=split, img_downscale=img_downscale, device=dsm.dsm.device, reader=reader)
    views, off = [], 0
    for k, (d, h, w) in enumerate(metas):
        rows = rgbs[off:off + h * w] if split == "train" else rgbs[k]
        off += h * w
        if h * w:  # an image whose down-scaled grid is empty has no pixel to bring
            views.append((rows.view(h, w, 3), rescale_rpc(d["rpc"], 1.0 / img_downscale)))
    return ortho_mosaic(dsm, views, **kw)
