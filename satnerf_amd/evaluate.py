"""One image of the reference's ``eval_satnerf.eval_aoi`` (eval_satnerf.py:244-297) without file I/O: render, then the three numbers
it prints -- PSNR, SSIM and the registered DSM MAE (DESIGN.md sections 7.1 and 7.2) -- and the sun sweep of
``study_solar_interpolation.sun_interp``."""
from __future__ import annotations

import glob
import json
import os

import numpy as np
import torch

from . import metrics, ops, visualize
from .dsm import dsm_from_depth, dsm_mae
from .rendering import latlonalt_from_depth, render_image_outputs, render_sun_visibility


def evaluate_image(models, rays, ts, rgbs, h, w, args, center=None, scene_range=None, roi=None, gt=None, gt_mask=None):
    """Render one (h, w) image with ``render_image_outputs`` (once) and score it as eval_aoi does.

    rays (N, 11) and ts (N,) are the image's rays in row-major pixel order, rgbs (N, 3) its ground-truth colours, N = h * w, all on
    the GPU.  ``psnr`` = metrics.psnr(rgb, rgbs); ``ssim`` = metrics.ssim(rgb.view(1, 3, h, w), rgbs.view(1, 3, h, w)).  That
    ``.view`` keeps the reference's layout quirk (main.py:195, eval_satnerf.py:290): it reinterprets the (N, 3) pixel-major buffer, so
    "plane" c is elements [c N, (c + 1) N) of the interleaved RGB values, not colour channel c.  The SSIM is therefore the number the
    reference prints, not the SSIM of the image's true colour planes.

    With ``gt`` (the ground-truth DSM on the ``{aoi}_DSM.txt`` grid ``roi``, with the dataset's ``center`` / ``scene_range``) also
    ``mae`` = dsm_mae(dsm_from_depth(rays, depth, center, scene_range, roi=roi), gt, gt_mask, register="xyz")[0], the reference's
    registered DSM MAE; ``None`` otherwise.

    Returns {"typ", "psnr", "ssim", "mae", "outputs"}: the metrics as Python floats (psnr and ssim come back in one device-to-host
    copy), ``outputs`` the dict of ``render_image_outputs``."""
    n = rays.shape[0]
    if int(h) * int(w) != n:
        raise ValueError(f"h * w = {int(h) * int(w)} does not match the {n} rays")
    if not torch.is_tensor(rgbs) or tuple(rgbs.shape) != (n, 3):
        raise ValueError(f"rgbs must be ({n}, 3), got {tuple(rgbs.shape) if torch.is_tensor(rgbs) else type(rgbs).__name__}")
    if gt is not None and (center is None or scene_range is None or roi is None):
        raise ValueError("a DSM MAE needs center, scene_range and roi")
    with torch.no_grad():
        out = render_image_outputs(models, rays, ts, args)
        rgb = out["rgb"].contiguous()  # a column slice of the image buffer
        gt_rgb = rgbs.float().contiguous()
        psnr = metrics.psnr(rgb, gt_rgb)
        ssim = metrics.ssim(rgb.view(1, 3, h, w), gt_rgb.view(1, 3, h, w))
        mae = None
        if gt is not None:
            dsm = dsm_from_depth(rays, out["depth"], center, scene_range, roi=roi)
            mae = dsm_mae(dsm, gt, gt_mask, register="xyz")[0]
        p, s = torch.stack([psnr, ssim]).tolist()
    return {"typ": out["typ"], "psnr": p, "ssim": s, "mae": mae, "outputs": out}


def ortho_psnr(rgb, mosaic, min_views=1):
    """``metrics.psnr`` of a rendered ortho image against the imagery brought onto the same grid: ``rgb`` ((ysize, xsize, C) or
    (ysize * xsize, C), e.g. ``render_ortho_dsm``'s ``outputs["rgb"]``) against ``mosaic["color"]`` (``dsm.ortho_mosaic``'s dict) over
    the cells that at least ``min_views`` views see and where both colours are finite.  A 0-dim fp32 device tensor; NaN when no cell
    qualifies."""
    want, count = mosaic["color"], mosaic["count"]
    if not (torch.is_tensor(rgb) and rgb.is_cuda and torch.is_tensor(want) and want.is_cuda):
        raise ValueError("ortho_psnr: rgb and the mosaic must live on the GPU; satnerf_amd has no CPU path")
    if int(min_views) < 1:
        raise ValueError(f"ortho_psnr: min_views must be >= 1, got {min_views}")
    if rgb.numel() != want.numel() or rgb.shape[-1] != want.shape[-1]:
        raise ValueError(f"ortho_psnr: rgb {tuple(rgb.shape)} does not hold the mosaic's {tuple(want.shape)} colours")
    pred = rgb.reshape(want.shape).float()
    valid = (count >= int(min_views)) & torch.isfinite(want).all(-1) & torch.isfinite(pred).all(-1)
    keep = valid.unsqueeze(-1)
    return metrics.psnr(torch.where(keep, pred, 0.0), torch.where(keep, want, 0.0), valid_mask=valid)


def solar_incidence_angle(sun_d):
    """The angle in degrees between a sun direction and the vertical, in fp64: arccos of the z component of the normalised direction.
    study_solar_interpolation.py:155-159 and :193-196 take the dot product with the unit normal (0, 0, 1), which adds two exact zeros to
    that component, so the bits are the same."""
    d = np.asarray(sun_d, dtype=np.float64)
    return float(np.degrees(np.arccos((d / np.linalg.norm(d))[2])))


def _sun_direction(elevation_deg, azimuth_deg):
    """(east, north, up) fp64 unit vector towards the sun."""
    el, az = np.radians(float(elevation_deg)), np.radians(float(azimuth_deg))
    flat = np.cos(el)
    return np.array([np.sin(az) * flat, np.cos(az) * flat, np.sin(el)])


def sun_direction_bounds(root_dir):
    """(upper, lower): the sun directions (fp64, (3,)) with the smallest and the largest incidence angle among every ``*.json`` of
    ``root_dir`` (study_solar_interpolation.py:145-165), read in sorted path order (the reference takes glob's order; with two files at
    the same extreme angle the first in this order wins).  direction = (sin az cos el, cos az cos el, sin el) of "sun_azimuth" and
    "sun_elevation" in degrees."""
    paths = sorted(glob.glob(os.path.join(root_dir, "*.json")))
    if not paths:
        raise ValueError(f"no *.json under {root_dir}")
    dirs = []
    for p in paths:
        with open(p) as f:
            meta = json.load(f)
        dirs.append(_sun_direction(meta["sun_elevation"], meta["sun_azimuth"]))
    angles = [solar_incidence_angle(d) for d in dirs]
    return dirs[int(np.argmin(angles))], dirs[int(np.argmax(angles))]


def interpolated_sun_directions(upper, lower, n_interp=10):
    """(directions (n_interp, 3) fp64, incidence angles in degrees): ``alpha * upper + (1 - alpha) * lower`` for alpha in
    linspace(0, 1, n_interp) (study_solar_interpolation.py:188-196).  The directions are NOT normalised: the reference feeds them to
    the model as they are."""
    upper, lower = np.asarray(upper, dtype=np.float64), np.asarray(lower, dtype=np.float64)
    if upper.shape != (3,) or lower.shape != (3,):
        raise ValueError(f"upper and lower must be (3,), got {upper.shape} and {lower.shape}")
    if int(n_interp) < 1:
        raise ValueError(f"n_interp must be >= 1, got {n_interp}")
    dirs = np.stack([alpha * upper + (1 - alpha) * lower for alpha in np.linspace(0, 1, int(n_interp))])
    return dirs, [solar_incidence_angle(d) for d in dirs]


def reference_strip_order(angles):
    """The order in which the reference lays the sweep's images out in its summary strips: it sorts the output FILE NAMES, which carry
    the angle as ``"{:.2f}deg"`` (study_solar_interpolation.py:216,225-237) -- a string sort, so 10.20 comes before 9.50.  Returns the
    list of sweep positions in strip order; equal names keep their sweep order."""
    names = ["{:.2f}deg".format(a) for a in angles]
    return sorted(range(len(names)), key=lambda k: names[k])


def sun_interp(models, rays, ts, args, h, w, upper, lower, center, scene_range, n_interp=10, lut=None, order="reference"):
    """The sweep of ``study_solar_interpolation.sun_interp`` (:187-239) for one (h, w) view without file I/O: for each of the
    ``n_interp`` directions between ``lower`` and ``upper`` (``sun_direction_bounds``), ``float32(sun_d)`` goes into columns 8:11 of a
    copy of ``rays`` (N, 11), ``render_image_outputs`` runs once and ``latlonalt_from_depth`` gives the altitudes the reference writes
    as its depth image.

    Returns {"angles", "sun_dirs", "outputs", "alts", "order", "strips"}: the incidence angles (degrees), directions (n_interp, 3)
    fp64, per-angle output dicts and (h, w) fp32 altitude images, all in sweep order; ``order`` = the strips' layout as sweep
    positions (``order="reference"``: ``reference_strip_order``; ``"sweep"``: as rendered); ``strips`` = {"sun", "albedo", "rgb"} from
    ``visualize.sun_strip`` / ``rgb_strip`` (cropped, as the reference's summary) and, with ``lut``, "depth" = ``visualize.dsm_strip``
    over the altitude images.  Every shadow of this sweep comes from the ``sun_v`` head, a regression on the training images' sun
    directions; ``sun_interp_shadows`` is the same sweep with the shadows cast through the density as well."""
    return sun_interp_shadows(models, rays, ts, args, h, w, upper, lower, center, scene_range, n_interp=n_interp, lut=lut, order=order)


def sun_interp_shadows(models, rays, ts, args, h, w, upper, lower, center, scene_range, n_interp=10, lut=None, order="reference", shadows="head",
                       max_alt=None):
    """``sun_interp`` with a choice of where the shadows come from.  ``shadows="head"`` (the default) is
    ``sun_interp`` itself: arguments, draws and results.  ``shadows="geometry"`` (needs ``max_alt``, the scene's upper altitude bound in metres) adds to each
    direction's output dict "sun_geo" (N, 1), the transparency of the learned density between the rendered surface and the sun
    (``rendering.render_sun_visibility`` on that direction's depths), and "rgb_geo" (N, 3) = ``ops.sun_shade`` of the direction's
    "albedo", "sky" and "sun_geo": a per-pixel relighting of the composited albedo, not a per-sample re-compositing.  The strips gain
    "sun_geo" and "rgb_geo"; every other key is what ``shadows="head"`` returns.  (The keyword lives on this name, not on ``sun_interp``,
    whose parameter list is pinned as the reference's.)"""
    if shadows not in ("head", "geometry"):
        raise ValueError(f"shadows must be 'head' or 'geometry', got {shadows!r}")
    if shadows == "geometry" and max_alt is None:
        raise ValueError("shadows='geometry' needs max_alt, the scene's upper altitude bound in metres")
    n = rays.shape[0]
    if int(h) * int(w) != n:
        raise ValueError(f"h * w = {int(h) * int(w)} does not match the {n} rays")
    if rays.dim() != 2 or rays.shape[1] < 11:
        raise ValueError(f"rays must be (N, 11) with the sun direction in columns 8:11, got {tuple(rays.shape)}")
    if order not in ("reference", "sweep"):
        raise ValueError(f"order must be 'reference' or 'sweep', got {order!r}")
    h, w = int(h), int(w)
    dirs, angles = interpolated_sun_directions(upper, lower, n_interp)
    outputs, alts = [], []
    with torch.no_grad():
        swept = rays.float().clone()
        for sun_d in dirs:
            swept[:, 8:11] = torch.from_numpy(sun_d.astype(np.float32)).to(swept.device)
            out = render_image_outputs(models, swept, ts, args)
            if shadows == "geometry":
                geo = render_sun_visibility(models, swept, ts, args, center, scene_range, max_alt, sun_d=sun_d, depth=out["depth"])["sun_geo"]
                out["sun_geo"] = geo.view(n, 1)
                out["rgb_geo"] = ops.sun_shade(out["albedo"], out["sky"], geo)
            outputs.append(out)
            alts.append(latlonalt_from_depth(swept, out["depth"], center, scene_range)[2].float().view(h, w))
        layout = reference_strip_order(angles) if order == "reference" else list(range(len(angles)))
        strips = {"sun": visualize.sun_strip([outputs[k]["sun"].view(h, w, 1) for k in layout]),
                  "albedo": visualize.rgb_strip([outputs[k]["albedo"].view(h, w, 3) for k in layout]),
                  "rgb": visualize.rgb_strip([outputs[k]["rgb"].view(h, w, 3) for k in layout])}
        if shadows == "geometry":
            strips["sun_geo"] = visualize.sun_strip([outputs[k]["sun_geo"].view(h, w, 1) for k in layout])
            strips["rgb_geo"] = visualize.rgb_strip([outputs[k]["rgb_geo"].view(h, w, 3) for k in layout])
        if lut is not None:
            strips["depth"] = visualize.dsm_strip([alts[k] for k in layout], lut)
    return {"angles": angles, "sun_dirs": dirs, "outputs": outputs, "alts": alts, "order": layout, "strips": strips}
