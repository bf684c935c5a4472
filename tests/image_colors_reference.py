"""fp64 restatement of the colours ``load_tensor_from_rgb_geotiff`` (datasets/satellite.py:67-80) makes from an 8-bit image: ``u8 / 255``
rounded to float32, then ATen's ``upsample_bicubic2d`` (align_corners=False, no antialias, A = -0.75, border taps clamped, no clamp of the
result).  The source coordinate, its floor and the fraction t are computed in float32 exactly as sr_image_colors defines them (DESIGN.md
section 7.7) and then widened; the weights and the 16-tap sum are in float64.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np
import torch

A = -0.75
# (H, W, img_downscale) of the resize tests: sizes that are no multiple of anything, an exact factor, a large factor, sources barely larger
# than the stencil, a single output pixel, and a strip wide enough for the last bit of the fp32 coordinate to matter
SHAPES = [(37, 53, 1.5), (64, 96, 2), (50, 70, 4), (5, 7, 2), (3, 3, 3), (4, 2048, 1.7)]


def out_size(h, w, down):
    return int(h // down), int(w // down)


def random_image(h, w, seed=None):
    """Seeded uint8 (h, w, 3) noise: every tap matters and neighbouring pixels differ by up to the full range."""
    rng = np.random.default_rng(1000 * h + w if seed is None else seed)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def convert(u8):
    """float32(float64(u8) / 255.), the reference's conversion."""
    return (np.asarray(u8).astype(np.float64) / 255.).astype(np.float32)


def cubic1(x):
    return ((A + 2) * x - (A + 3)) * x * x + 1


def cubic2(x):
    return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A


def axis_taps(n_in, n_out, fp64_coords=False):
    """(indices (n_out, 4) clamped to the source, weights (n_out, 4) float64) of one axis."""
    dst = np.arange(n_out)
    if fp64_coords:
        src = (n_in / n_out) * (dst + 0.5) - 0.5
        i0 = np.floor(src)
        t = src - i0
    else:
        f = np.float32
        scale = f(n_in) / f(n_out)
        src = scale * (dst.astype(f) + f(0.5)) - f(0.5)  # numpy rounds the product and the difference separately: no fma
        assert src.dtype == np.float32
        i0 = np.floor(src)
        t = (src - i0).astype(np.float64)
    idx = np.clip(i0.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
    return idx, np.stack([cubic2(t + 1), cubic1(t), cubic1(1 - t), cubic2(2 - t)], 1)


def resize_rows(taps, wy, out_w, fp64_coords=False):
    """(k, out_w, 3) float64: k output rows from their source rows ``taps`` (k, 4, W, 3) float32 and row weights ``wy`` (k, 4)."""
    taps = np.asarray(taps)
    assert taps.dtype == np.float32 and taps.ndim == 4 and taps.shape[1] == 4 and taps.shape[3] == 3
    ix, wx = axis_taps(taps.shape[2], out_w, fp64_coords)
    rows = np.einsum("rj,rjwk->rwk", wy, taps.astype(np.float64))  # (k, W, 3)
    return np.einsum("cj,rcjk->rck", wx, rows[:, ix])              # (k, out_w, 3)


def resize(values, out_h, out_w, fp64_coords=False):
    """(out_h * out_w, 3) float64 from (H, W, 3) float32 values."""
    v = np.asarray(values)
    assert v.dtype == np.float32 and v.ndim == 3 and v.shape[2] == 3
    iy, wy = axis_taps(v.shape[0], out_h, fp64_coords)
    return resize_rows(v[iy], wy, out_w, fp64_coords).reshape(out_h * out_w, 3)


def colors(u8_hwc, out_h, out_w, fp64_coords=False):
    """(out_h * out_w, 3) float64: what sr_image_colors is to produce from a uint8 (H, W, 3) image."""
    u8 = np.asarray(u8_hwc)
    assert u8.dtype == np.uint8 and u8.ndim == 3 and u8.shape[2] == 3
    v = convert(u8)
    if out_h * out_w == 0:
        return np.zeros((0, 3))
    if (out_h, out_w) == u8.shape[:2]:
        return v.reshape(-1, 3).astype(np.float64)
    return resize(v, out_h, out_w, fp64_coords)


@functools.lru_cache(maxsize=None)
def case(h, w, down):
    """(uint8 image (h, w, 3), out_h, out_w, oracle colours (out_h * out_w, 3) float64) of one resize case; computed once, read-only."""
    img = random_image(h, w)
    oh, ow = out_size(h, w, down)
    want = colors(img, oh, ow)
    img.setflags(write=False)
    want.setflags(write=False)
    return img, oh, ow, want


def image_colors_stub(calls):
    """``ops.image_colors`` on the CPU through the oracle, rounded to float32; appends (H, W, out_h, out_w, layout) to ``calls``."""
    def stub(image_u8, out_h, out_w, out=None, layout=None):
        assert image_u8.dtype == torch.uint8 and image_u8.dim() == 3 and layout in ("hwc", "chw")
        assert out_h * out_w > 0, "an empty grid must not reach the kernel"
        a = image_u8.numpy()
        a = np.transpose(a, (1, 2, 0)) if layout == "chw" else a
        calls.append((a.shape[0], a.shape[1], out_h, out_w, layout))
        res = torch.from_numpy(colors(np.ascontiguousarray(a), out_h, out_w).astype(np.float32))
        if out is None:
            return res
        assert tuple(out.shape) == (out_h * out_w, 3) and out.dtype == torch.float32
        out.copy_(res)
        return out

    return stub
