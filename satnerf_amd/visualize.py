"""The reference's image products after the render, on the GPU: the nearest-valid-pixel hole fill, the
colour-mapped depth image of ``train_utils.visualize_depth`` and the summary strips of ``study_solar_interpolation.py``.

Everything takes and returns GPU tensors and reads its inputs in place through their strides, so a column of
``render_image_outputs``'s image buffer (e.g. ``out["sun"].view(h, w, 1)``) or a DSM raster goes in without a copy.

The colour table is the one part of these images that is not held to the reference: the reference colours with OpenCV's
``COLORMAP_JET`` / ``COLORMAP_VIRIDIS``, whose tables are not reproduced here.  Every function takes the table as a (256, 3) uint8
device tensor in the channel order wanted out; ``lut_from_matplotlib`` builds one from matplotlib's colormaps, which are
matplotlib's tables, not OpenCV's.  The byte index that goes into the table is the reference's, bit for bit."""
from __future__ import annotations

import torch

from . import ops


def crop_window(h, w):
    """(row_start, row_end, col_start, col_end) of the strips' crop: int(h / 4), int(3 h / 4), int(w / 4), int(3 w / 4)
    (study_solar_interpolation.py:31-32)."""
    h, w = int(h), int(w)
    return int(h / 4), int(3 * h / 4), int(w / 4), int(3 * w / 4)


def lut_from_matplotlib(name, device=None):
    """A (256, 3) uint8 RGB table from matplotlib's colormap ``name`` sampled at its 256 byte levels (``cmap(i, bytes=True)``), on
    ``device`` (default: the current GPU).  matplotlib's table -- its "jet" and "viridis" are not OpenCV's COLORMAP_JET /
    COLORMAP_VIRIDIS byte for byte.  matplotlib is imported here, so the package does not need it otherwise."""
    import matplotlib
    import numpy as np

    table = np.ascontiguousarray(matplotlib.colormaps[name](np.arange(256), bytes=True)[:, :3].astype(np.uint8))
    return torch.from_numpy(table).to(torch.device("cuda", torch.cuda.current_device()) if device is None else device)


def _image2d(image, name="image"):
    """(h, w) view of an (h, w) or (h, w, 1) GPU tensor."""
    if not torch.is_tensor(image) or not image.is_cuda:
        raise ValueError(f"{name} must be a GPU tensor: satnerf_amd has no CPU path")
    if image.dim() == 3 and image.shape[2] == 1:
        image = image[:, :, 0]
    if image.dim() != 2:
        raise ValueError(f"{name} must be (h, w) or (h, w, 1), got {tuple(image.shape)}")
    return image if image.dtype == torch.float32 else image.float()


def _windows(images, channels, crop):
    """The images' (cropped) views, checked to share one height: [(view (rows, cols[, C]))], rows, total columns."""
    images = list(images)
    if not images:
        raise ValueError("a strip needs at least one image")
    views = []
    for k, img in enumerate(images):
        if channels is None:
            v = _image2d(img, f"images[{k}]")
        else:
            if not torch.is_tensor(img) or not img.is_cuda:
                raise ValueError(f"images[{k}] must be a GPU tensor: satnerf_amd has no CPU path")
            v = img[:, :, None] if img.dim() == 2 else img
            if v.dim() != 3 or v.shape[2] < channels:
                raise ValueError(f"images[{k}] must be (h, w, >={channels}), got {tuple(img.shape)}")
            v = (v if v.dtype == torch.float32 else v.float())[:, :, :channels]
        if crop:
            r0, r1, c0, c1 = crop_window(v.shape[0], v.shape[1])
            v = v[r0:r1, c0:c1]
        views.append(v)
    rows = views[0].shape[0]
    if any(v.shape[0] != rows for v in views):
        raise ValueError(f"the images of one strip must share their height after the crop, got {[v.shape[0] for v in views]}")
    return views, rows, sum(v.shape[1] for v in views)


def fill_nans_nearest(image, return_index=False):
    """``quickly_interpolate_nans_from_singlechannel_img`` (study_solar_interpolation.py:53-68), scipy's griddata(method="nearest"):
    the (h, w) fp32 image with each NaN replaced by the nearest non-NaN pixel (Euclidean distance between pixel centres).  Of several
    pixels at the same distance the one in the smallest row, then the smallest column, is taken; scipy's choice among them is an
    implementation detail of its KD-tree.  An image of NaN only comes back unchanged (scipy raises).  Sides up to 8192.  With
    ``return_index`` also the (h, w) int32 index r' * w + c' of each pixel's source (-1 where there is none), from which a caller gets
    the distance."""
    return ops.nearest_fill(_image2d(image), want_index=bool(return_index))


def visualize_depth(depth, lut):
    """``train_utils.visualize_depth`` (train_utils.py:59-72): NaN -> 0, the image's own range, ``(uint8)(255 (x - mi) / (ma - mi +
    1e-8))``, the colour table, ``ToTensor``.  depth (H, W) fp32; returns (3, H, W) fp32 in the table's channel order."""
    return ops.colorize(_image2d(depth, "depth"), lut, nan_to_zero=True, want_chw=True)["chw"]


def dsm_strip(images, lut, crop=True, vmin=None, vmax=None):
    """``hstack_dsm_tifs_v1`` (study_solar_interpolation.py:70-95): each (h, w) image is cropped, its NaNs filled from the nearest valid
    pixel of the crop, normalised over its own range (or ``vmin`` / ``vmax``, Python floats, with clipping) and coloured; the results
    stand side by side.  Returns (rows, total_cols, 3) uint8 in the table's channel order."""
    views, rows, total = _windows(images, None, crop)
    strip = torch.empty(rows, total, 3, dtype=torch.uint8, device=views[0].device)
    col = 0
    for v in views:
        ops.colorize(ops.nearest_fill(v), lut, vmin=vmin, vmax=vmax, strip=strip, strip_col0=col)
        col += v.shape[1]
    return strip


def sun_strip(images, crop=True):
    """``hstack_sun_tifs`` (study_solar_interpolation.py:23-36): the first channel of each (h, w) or (h, w, C) image, cropped, side by
    side, as ``(uint8)(x * 255)``.  Returns (rows, total_cols) uint8."""
    views, rows, total = _windows(images, 1, crop)
    strip = torch.empty(rows, total, 1, dtype=torch.uint8, device=views[0].device)
    col = 0
    for v in views:
        ops.unit_to_u8(v, strip, col)
        col += v.shape[1]
    return strip[:, :, 0]


def rgb_strip(images, crop=True):
    """``hstack_rgb_tifs`` (study_solar_interpolation.py:38-51): the (h, w, 3) images, cropped, side by side, as ``(uint8)(x * 255)``.
    Returns (rows, total_cols, 3) uint8."""
    views, rows, total = _windows(images, 3, crop)
    strip = torch.empty(rows, total, 3, dtype=torch.uint8, device=views[0].device)
    col = 0
    for v in views:
        ops.unit_to_u8(v, strip, col)
        col += v.shape[1]
    return strip
