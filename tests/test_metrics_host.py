"""fp64 restatements of the reference's image metrics (metrics.py:105-121) and the checks on them (CPU only).

``ssim_np`` restates kornia 0.5.3's ``losses.ssim`` (window 3) in numpy with explicit reflect indexing; ``ssim_torch`` restates it a
second, independent way, line for line as kornia 0.5.3's ``filter2D`` / ``ssim`` (torch ``F.pad(mode='reflect')`` + grouped
``F.conv2d``), in any dtype: fp64 to check the first, fp32 for what the reference itself computes.  kornia is not installed here, so
no kornia output could be produced; both restatements follow the written semantics of DESIGN.md section 7.2.  ``mse_np`` /
``psnr_np`` restate ``metrics.mse`` / ``metrics.psnr``.  tests/test_hip_metrics.py checks the GPU kernels against these.
"""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kornia.filters.get_gaussian_kernel1d(3, 1.5), evaluated in fp64
GAUSS_TAPS = (0.30780132912346997, 0.38439734175306, 0.30780132912346997)
C1, C2, EPS = 0.01 ** 2, 0.03 ** 2, 1e-12


# ---- numpy restatement ------------------------------------------------------------------------------------------------------------
def reflect_index(n):
    """Source index of padded positions -1 .. n of torch's reflect padding: -1 -> 1, n -> n - 2."""
    idx = np.arange(-1, n + 1)
    idx[0], idx[-1] = 1, n - 2
    return idx


def ssim_moments_np(x, y):
    """(mu1, mu2, sigma1^2, sigma2^2, sigma12) of two (..., H, W) arrays in fp64: the 3x3 Gaussian over reflect-padded images."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    h, w = x.shape[-2:]
    assert h >= 2 and w >= 2
    ri, ci = reflect_index(h), reflect_index(w)
    g = np.asarray(GAUSS_TAPS)

    def filt(z):
        zp = z[..., ri, :][..., :, ci]
        out = np.zeros_like(z)
        for dy in range(3):
            for dx in range(3):
                out += g[dy] * g[dx] * zp[..., dy:dy + h, dx:dx + w]
        return out

    mu1, mu2 = filt(x), filt(y)
    return mu1, mu2, filt(x * x) - mu1 ** 2, filt(y * y) - mu2 ** 2, filt(x * y) - mu1 * mu2


def ssim_map_np(x, y):
    mu1, mu2, s1, s2, s12 = ssim_moments_np(x, y)
    num = (2 * mu1 * mu2 + C1) * (2 * s12 + C2)
    den = (mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2)
    return num / (den + EPS)


def ssim_np(x, y):
    """metrics.ssim: the mean of the map over every pixel of every plane (fp64)."""
    return float(ssim_map_np(x, y).mean())


# ---- torch restatement, line for line as kornia 0.5.3 -------------------------------------------------------------------------------
def _gaussian(window_size, sigma, dtype):
    x = torch.arange(window_size, dtype=dtype) - window_size // 2
    gauss = torch.exp(-x.pow(2.0) / float(2 * sigma ** 2))
    return gauss / gauss.sum()


def _filter2d(inp, kernel):
    b, c, h, w = inp.shape
    tmp_kernel = kernel.unsqueeze(1).to(inp).expand(-1, c, -1, -1)
    height, width = tmp_kernel.shape[-2:]
    input_pad = F.pad(inp, [width // 2, width // 2, height // 2, height // 2], mode="reflect")
    tmp_kernel = tmp_kernel.reshape(-1, 1, height, width)
    input_pad = input_pad.view(-1, tmp_kernel.size(0), input_pad.size(-2), input_pad.size(-1))
    return F.conv2d(input_pad, tmp_kernel, groups=tmp_kernel.size(0), padding=0, stride=1).view(b, c, h, w)


def ssim_map_torch(img1, img2, window_size=3, max_val=1.0, eps=1e-12):
    k1 = _gaussian(window_size, 1.5, img1.dtype)
    kernel = torch.matmul(k1.unsqueeze(-1), k1.unsqueeze(-1).t()).unsqueeze(0)
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    mu1, mu2 = _filter2d(img1, kernel), _filter2d(img2, kernel)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    sigma1_sq = _filter2d(img1 ** 2, kernel) - mu1_sq
    sigma2_sq = _filter2d(img2 ** 2, kernel) - mu2_sq
    sigma12 = _filter2d(img1 * img2, kernel) - mu1_mu2
    num = (2.0 * mu1_mu2 + c1) * (2.0 * sigma12 + c2)
    den = (mu1_sq + mu2_sq + c1) * (sigma1_sq + sigma2_sq + c2)
    return num / (den + eps)


def ssim_torch(img1, img2):
    """metrics.ssim as the reference computes it, in img1's dtype and on its device: torch.mean(ssim_(img1, img2, 3))."""
    return torch.mean(ssim_map_torch(img1, img2, 3))


# ---- mse / psnr --------------------------------------------------------------------------------------------------------------------
def mse_np(pred, gt, valid_mask=None, reduction="mean"):
    """metrics.mse in fp64: the mask selects like torch boolean indexing (the images' shape or their leading dimensions)."""
    value = (np.asarray(pred, np.float64) - np.asarray(gt, np.float64)) ** 2
    if valid_mask is not None:
        value = value[np.asarray(valid_mask, bool)]
    if reduction == "mean":
        with np.errstate(invalid="ignore"):
            return value.sum() / value.size if value.size else float("nan")
    return value


def psnr_np(pred, gt, valid_mask=None, reduction="mean"):
    with np.errstate(divide="ignore"):
        return -10 * np.log10(mse_np(pred, gt, valid_mask, reduction))


def random_pair(rng, shape):
    x = rng.random(shape)
    return x, np.clip(x + 0.1 * rng.standard_normal(shape), 0, 1)


# ---- tests -------------------------------------------------------------------------------------------------------------------------
def test_gaussian_taps_closed_form():
    e = math.exp(-1 / (2 * 1.5 ** 2))
    assert GAUSS_TAPS[0] == GAUSS_TAPS[2]
    assert abs(GAUSS_TAPS[0] - e / (1 + 2 * e)) <= 1e-16 and abs(GAUSS_TAPS[1] - 1 / (1 + 2 * e)) <= 1e-16
    assert np.abs(_gaussian(3, 1.5, torch.float64).numpy() - np.asarray(GAUSS_TAPS)).max() <= 1e-16
    # the HIP kernel carries the same two constants
    src = open(os.path.join(REPO, "satnerf_amd", "csrc", "image_metrics.hip")).read()
    g0 = float(re.search(r"constexpr double kG0 = ([0-9.e+-]+);", src).group(1))
    g1 = float(re.search(r"constexpr double kG1 = ([0-9.e+-]+);", src).group(1))
    assert (g0, g1) == (GAUSS_TAPS[0], GAUSS_TAPS[1])


@pytest.mark.parametrize("shape", [(1, 3, 2, 2), (1, 3, 2, 7), (1, 3, 3, 3), (2, 5, 7, 9), (1, 3, 17, 64), (1, 1, 40, 33)])
def test_numpy_and_torch_restatements_agree(shape):
    rng = np.random.default_rng(sum(shape))
    x, y = random_pair(rng, shape)
    a = ssim_map_np(x, y)
    b = ssim_map_torch(torch.from_numpy(x), torch.from_numpy(y)).numpy()
    assert np.abs(a - b).max() <= 1e-12
    assert abs(ssim_np(x, y) - ssim_torch(torch.from_numpy(x), torch.from_numpy(y)).item()) <= 1e-12


def test_reflect_is_not_edge_repeat():
    assert reflect_index(5).tolist() == [1, 0, 1, 2, 3, 4, 3]
    assert reflect_index(2).tolist() == [1, 0, 1, 0]
    x = torch.arange(6, dtype=torch.float64).view(1, 1, 2, 3)
    pad = F.pad(x, [1, 1, 1, 1], mode="reflect")[0, 0]
    ri, ci = reflect_index(2), reflect_index(3)
    assert torch.equal(pad, x[0, 0][ri][:, ci])


def test_identical_images():
    rng = np.random.default_rng(1)
    x = rng.random((1, 3, 12, 10))
    mu1, _, s1, _, _ = ssim_moments_np(x, x)
    num = (2 * mu1 ** 2 + C1) * (2 * s1 + C2)
    assert np.abs(ssim_map_np(x, x) - num / (num + EPS)).max() <= 1e-15
    assert abs(ssim_np(x, x) - 1.0) <= 1e-6


@pytest.mark.parametrize("a,b", [(0.2, 0.7), (0.0, 1.0), (0.5, 0.5), (0.9, 0.1)])
def test_constant_images_closed_form(a, b):
    x, y = np.full((1, 3, 6, 5), a), np.full((1, 3, 6, 5), b)
    want = (2 * a * b + C1) * C2 / ((a * a + b * b + C1) * C2 + EPS)
    assert np.abs(ssim_map_np(x, y) - want).max() <= 1e-12
    assert abs(ssim_np(x, y) - want) <= 1e-12


def test_symmetric_in_its_arguments():
    rng = np.random.default_rng(2)
    x, y = random_pair(rng, (2, 3, 9, 11))
    assert np.abs(ssim_map_np(x, y) - ssim_map_np(y, x)).max() <= 1e-15


def test_two_by_two_by_hand():
    x = np.array([[0.1, 0.8], [0.4, 0.3]])
    y = np.array([[0.2, 0.6], [0.5, 0.9]])
    g = GAUSS_TAPS
    # a 2 x 2 image reflect-pads to rows / columns (1, 0, 1, 0): pixel i's neighbourhood is (1, 0, 1) for i = 0 and (0, 1, 0) for i = 1
    nb = {0: (1, 0, 1), 1: (0, 1, 0)}
    total = 0.0
    for i in range(2):
        for j in range(2):
            m = [0.0] * 5
            for a in range(3):
                for b in range(3):
                    wgt = g[a] * g[b]
                    u, v = x[nb[i][a], nb[j][b]], y[nb[i][a], nb[j][b]]
                    for k, val in enumerate((u, v, u * u, v * v, u * v)):
                        m[k] += wgt * val
            s1, s2, s12 = m[2] - m[0] ** 2, m[3] - m[1] ** 2, m[4] - m[0] * m[1]
            total += (2 * m[0] * m[1] + C1) * (2 * s12 + C2) / ((m[0] ** 2 + m[1] ** 2 + C1) * (s1 + s2 + C2) + EPS)
    assert abs(ssim_np(x[None, None], y[None, None]) - total / 4) <= 1e-15


def test_psnr_restatement():
    rng = np.random.default_rng(3)
    p, g = random_pair(rng, (50, 3))
    tp, tg = torch.from_numpy(p), torch.from_numpy(g)
    # the reference's own formulas (metrics.py:105-115) in torch fp64 on the CPU
    ref_mse = lambda v, m=None: torch.mean(((tp - tg) ** 2)[m] if m is not None else (tp - tg) ** 2)  # noqa: E731
    assert abs(mse_np(p, g) - ref_mse(None).item()) <= 1e-15
    assert abs(psnr_np(p, g) - (-10 * torch.log10(ref_mse(None))).item()) <= 1e-12
    row = rng.random(50) < 0.6
    elem = rng.random((50, 3)) < 0.5
    for m in (row, elem):
        tm = torch.from_numpy(m)
        assert abs(mse_np(p, g, m) - ref_mse(None, tm).item()) <= 1e-15
        assert np.array_equal(mse_np(p, g, m, "none"), (((tp - tg) ** 2)[tm]).numpy())
        assert np.allclose(psnr_np(p, g, m, "none"), -10 * np.log10(mse_np(p, g, m, "none")))
    assert mse_np(p, g, row, "none").shape == (int(row.sum()), 3) and mse_np(p, g, elem, "none").shape == (int(elem.sum()),)
    assert psnr_np(p, p) == float("inf")
    assert math.isnan(psnr_np(p, g, np.zeros(50, bool)))
