"""Image metrics on the GPU: the reference's ``metrics.mse`` / ``metrics.psnr`` / ``metrics.ssim``
(metrics.py:105-121) with the same names and signatures, over the HIP reductions of csrc/image_metrics.hip.

The reference's ``ssim`` calls kornia 0.5.3's ``losses.ssim`` with window 3; kornia is not needed here.  Both reductions accumulate
in fp64 and are bitwise repeatable; a metric is returned as a 0-dim fp32 device tensor, rounded once from fp64.  Nothing is read back
to the host, so the calls can be captured into a graph.  There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

import torch

from . import ops


def _pair(a, b, fn):
    for name, t in (("image_pred", a), ("image_gt", b)):
        if not torch.is_tensor(t):
            raise TypeError(f"{fn}: {name} must be a tensor")
        if not t.is_cuda:
            raise ValueError(f"{fn}: {name} must live on the GPU (got {t.device}); satnerf_amd has no CPU path")
        if not t.dtype.is_floating_point:
            raise ValueError(f"{fn}: {name} must be floating point (got {t.dtype})")
    if a.shape != b.shape:
        raise ValueError(f"{fn}: image_pred {tuple(a.shape)} and image_gt {tuple(b.shape)} differ in shape")
    if a.device != b.device:
        raise ValueError(f"{fn}: image_pred is on {a.device}, image_gt on {b.device}")
    return a.float().contiguous(), b.float().contiguous()


def _mask_div(valid_mask, shape, fn):
    """mask_div of a boolean mask over the leading dimensions of ``shape`` (torch boolean indexing): the trailing size."""
    if not torch.is_tensor(valid_mask) or valid_mask.dtype != torch.bool:
        raise ValueError(f"{fn}: valid_mask must be a boolean tensor")
    if not valid_mask.is_cuda:
        raise ValueError(f"{fn}: valid_mask must live on the GPU (got {valid_mask.device})")
    k = valid_mask.dim()
    if k < 1 or tuple(valid_mask.shape) != tuple(shape[:k]):
        raise ValueError(f"{fn}: valid_mask {tuple(valid_mask.shape)} must match the leading dimensions of the images {tuple(shape)}")
    div = 1
    for s in shape[k:]:
        div *= int(s)
    return div


def _sse(image_pred, image_gt, valid_mask, reduction, fn):
    """(pred, gt, {sum, count}) for reduction 'mean', (pred, gt, None) for 'none'."""
    if reduction not in ("mean", "none"):
        raise ValueError(f"{fn}: reduction must be 'mean' or 'none', got {reduction!r}")
    a, b = _pair(image_pred, image_gt, fn)
    div = None if valid_mask is None else _mask_div(valid_mask, a.shape, fn)
    if reduction == "none":
        return a, b, None
    if div is None or a.numel() == 0:  # no mask, or nothing a mask could select
        return a, b, ops.image_sse(a, b)
    return a, b, ops.image_sse(a, b, valid_mask.contiguous(), div)


def mse(image_pred, image_gt, valid_mask=None, reduction="mean"):
    """``metrics.mse`` (metrics.py:105-112): the mean of (pred - gt)^2 over the elements ``valid_mask`` selects (a boolean mask of the
    images' shape or of their leading dimensions), a 0-dim fp32 device tensor summed in fp64 on the GPU; NaN when the mask selects
    nothing.  ``reduction='none'`` returns the per-element values as the reference does (elementwise torch, fp32)."""
    a, b, sse = _sse(image_pred, image_gt, valid_mask, reduction, "mse")
    if sse is None:
        value = (a - b) ** 2
        return value[valid_mask] if valid_mask is not None else value
    return (sse[0] / sse[1]).float()


def psnr(image_pred, image_gt, valid_mask=None, reduction="mean"):
    """``metrics.psnr`` (metrics.py:114-115): -10 log10(mse), evaluated in fp64 from the fp64 sum and rounded once to a 0-dim fp32 device
    tensor.  Identical images give inf, an empty mask NaN, as in torch.  ``reduction='none'`` is the reference's elementwise form."""
    a, b, sse = _sse(image_pred, image_gt, valid_mask, reduction, "psnr")
    if sse is None:
        return -10 * torch.log10(mse(a, b, valid_mask, reduction))
    return (-10.0 * torch.log10(sse[0] / sse[1])).float()


def ssim(image_pred, image_gt):
    """``metrics.ssim`` (metrics.py:117-121): the mean of kornia 0.5.3's ``losses.ssim`` map with window 3 (3x3 Gaussian, sigma 1.5,
    reflect borders, C1 = 0.01^2, C2 = 0.03^2) over every pixel of every plane of (B, C, H, W) images, a 0-dim fp32 device tensor
    (the map and its sum in fp64 on the GPU).  H and W must be >= 2 (torch's reflect padding raises below that).

    The reference passes ``results["rgb_*"].view(1, 3, H, W)`` of an (H*W, 3) pixel-major tensor: a reinterpretation, not a permute.
    This function takes NCHW as given; to score the true image of such a tensor, ``.t().reshape(1, 3, H, W)`` it first."""
    a, b = _pair(image_pred, image_gt, "ssim")
    if a.dim() != 4:
        raise ValueError(f"ssim: the images must be (B, C, H, W), got shape {tuple(a.shape)}")
    if a.shape[2] < 2 or a.shape[3] < 2:
        raise ValueError(f"ssim: H and W must be >= 2 for reflect padding, got {tuple(a.shape)}")
    out = ops.ssim_sum(a, b)
    return (out[0] / out[1]).float()
