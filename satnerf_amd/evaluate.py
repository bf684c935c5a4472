"""One image of the reference's ``eval_satnerf.eval_aoi`` (eval_satnerf.py:244-297) without file I/O: render, then the three numbers
it prints -- PSNR, SSIM and the registered DSM MAE (DESIGN.md sections 7.1 and 7.2)."""
from __future__ import annotations

import torch

from . import metrics
from .dsm import dsm_from_depth, dsm_mae
from .rendering import render_image_outputs


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
