"""Image metrics on the GPU (csrc/image_metrics.hip through satnerf_amd.metrics / satnerf_amd.evaluate): PSNR and SSIM against the
fp64 restatements of tests/test_metrics_host.py and an fp32 restatement of kornia 0.5.3's op sequence, determinism, graph capture,
errors, and one image of eval_aoi end to end."""
import math

import numpy as np
import pytest
import torch

from oracle import satnerf_oracle as O
from tests.test_metrics_host import mse_np, psnr_np, random_pair, ssim_np, ssim_torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _m():
    from satnerf_amd import metrics

    return metrics


def _t(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(DEV)


def structured_pair(rng, shape):
    """Smooth gradients and edges with noise: the kind of image SSIM is for."""
    *lead, h, w = shape
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    base = 0.5 + 0.3 * np.sin(6 * xx + 3 * yy) * ((xx + yy) > 0.7) + 0.2 * (yy > 0.4)
    x = np.broadcast_to(base, shape) * rng.uniform(0.6, 1.0, tuple(lead) + (1, 1))
    y = x + 0.05 * rng.standard_normal(shape)
    return np.clip(x, 0, 1), np.clip(y, 0, 1)


def check_ssim(x, y, tol=1e-6):
    """The GPU SSIM of fp32 images x, y against the fp64 restatement and against the reference's fp32 op sequence."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)  # both restatements see the fp32 values the kernel reads
    got = _m().ssim(_t(x), _t(y))
    assert got.dtype == torch.float32 and got.dim() == 0 and got.is_cuda
    want = ssim_np(x, y)
    assert abs(got.item() - want) <= tol, (got.item(), want)
    ref32 = ssim_torch(torch.from_numpy(x), torch.from_numpy(y)).item()  # on the CPU
    assert abs(got.item() - ref32) <= 1e-4, (got.item(), ref32)
    return got.item(), want


@pytest.mark.parametrize("h", [2, 3, 17, 64, 513])
@pytest.mark.parametrize("w", [2, 3, 17, 64, 513])
def test_ssim_against_restatement(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    check_ssim(*random_pair(rng, (1, 3, h, w)))


@pytest.mark.parametrize("shape", [(1, 3, 100, 70), (2, 5, 40, 33), (1, 3, 33, 65), (3, 1, 257, 130)])
def test_ssim_structured_and_batched(shape):
    rng = np.random.default_rng(sum(shape))
    check_ssim(*structured_pair(rng, shape))
    check_ssim(*random_pair(rng, shape))


def test_ssim_identical_and_extreme_images():
    rng = np.random.default_rng(5)
    x = rng.random((1, 3, 31, 47)).astype(np.float32)
    check_ssim(x, x)
    check_ssim(np.zeros_like(x), np.ones_like(x))
    check_ssim(np.full_like(x, 0.25), np.full_like(x, 0.75))


def test_ssim_2048():
    # the fp64 reference here is the torch restatement (tests/test_metrics_host.py pins it to the numpy one at 1e-12), on the CPU
    rng = np.random.default_rng(2048)
    x, y = (torch.from_numpy(a.astype(np.float32)) for a in structured_pair(rng, (1, 3, 2048, 2048)))
    got = _m().ssim(x.to(DEV), y.to(DEV)).item()
    assert abs(got - ssim_torch(x.double(), y.double()).item()) <= 1e-6
    assert abs(got - ssim_torch(x, y).item()) <= 1e-4


def test_psnr_and_mse():
    metrics = _m()
    rng = np.random.default_rng(7)
    p, g = (a.astype(np.float32) for a in random_pair(rng, (4097, 3)))
    tp, tg = _t(p), _t(g)
    for fn, ref in ((metrics.mse, mse_np), (metrics.psnr, psnr_np)):
        got = fn(tp, tg)
        assert got.dtype == torch.float32 and got.dim() == 0 and got.is_cuda
        want = ref(p, g)
        assert abs(got.item() - want) <= 2e-7 * abs(want), (fn.__name__, got.item(), want)
        row = rng.random(4097) < 0.7
        elem = rng.random((4097, 3)) < 0.3
        for m in (row, elem):
            tm = torch.from_numpy(m).to(DEV)
            got, want = fn(tp, tg, tm).item(), ref(p, g, m)
            assert abs(got - want) <= 2e-7 * abs(want), (fn.__name__, m.shape, got, want)
            none = fn(tp, tg, tm, reduction="none")
            assert none.is_cuda and none.shape == ref(p, g, m, "none").shape
            assert np.allclose(none.cpu().numpy(), ref(p, g, m, "none"), rtol=1e-5, atol=1e-9)
        none = fn(tp, tg, reduction="none")
        assert none.shape == (4097, 3) and np.allclose(none.cpu().numpy(), ref(p, g, None, "none"), rtol=1e-5, atol=1e-9)
    # odd sizes, an unaligned view (the scalar path), a 4-D image, a mask over the first two dimensions
    for n in (1, 2, 3, 5, 1023):
        a, b = rng.random(n).astype(np.float32), rng.random(n).astype(np.float32)
        assert abs(metrics.mse(_t(a), _t(b)).item() - mse_np(a, b)) <= 2e-7 * mse_np(a, b)
    big_p, big_g = _t(np.concatenate([[0.0], p.ravel()])), _t(np.concatenate([[0.0], g.ravel()]))
    aligned = metrics.mse(tp.view(-1), tg.view(-1))
    assert torch.equal(metrics.mse(big_p[1:], big_g[1:]), aligned)  # the same elements in the same order, bit for bit
    x, y = (a.astype(np.float32) for a in random_pair(rng, (2, 3, 9, 8)))
    m = rng.random((2, 3)) < 0.5
    m[0, 0] = True
    got = metrics.psnr(_t(x), _t(y), torch.from_numpy(m).to(DEV)).item()
    assert abs(got - psnr_np(x, y, m)) <= 2e-7 * abs(psnr_np(x, y, m))


def test_psnr_special_values():
    metrics = _m()
    x = torch.rand(100, 3, device=DEV)
    assert metrics.psnr(x, x).item() == float("inf") and metrics.mse(x, x).item() == 0.0
    empty = torch.zeros(100, dtype=torch.bool, device=DEV)
    assert math.isnan(metrics.psnr(x, torch.rand_like(x), empty).item())
    assert math.isnan(metrics.mse(x, torch.rand_like(x), empty).item())
    assert math.isnan(metrics.mse(x[:0], x[:0]).item())  # torch.mean of nothing


def test_deterministic_and_capturable():
    metrics = _m()
    rng = np.random.default_rng(11)
    x, y = (_t(a) for a in structured_pair(rng, (1, 3, 700, 900)))
    mask = torch.from_numpy(rng.random(700 * 900) < 0.8).to(DEV)
    px, py = x.view(-1, 3), y.view(-1, 3)  # the reference's (N, 3) view

    def step():
        return metrics.psnr(px, py), metrics.psnr(px, py, mask), metrics.ssim(x, y)

    first = [t.clone() for t in step()]
    for _ in range(3):
        again = step()
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, again))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, captured))


def test_errors():
    metrics = _m()
    x = torch.rand(1, 3, 8, 8, device=DEV)
    for fn in (metrics.mse, metrics.psnr, metrics.ssim):
        with pytest.raises(ValueError):
            fn(x.cpu(), x.cpu())
        with pytest.raises(ValueError):
            fn(x, x[:, :2])
    with pytest.raises(ValueError):
        metrics.ssim(x[0], x[0])  # not 4-D
    for bad in (x[:, :, :1], x[:, :, :, :1]):  # H or W = 1
        with pytest.raises(ValueError):
            metrics.ssim(bad, bad)
    with pytest.raises(ValueError):
        metrics.psnr(x, x, torch.ones(3, dtype=torch.bool, device=DEV))  # not the leading dimensions
    with pytest.raises(ValueError):
        metrics.psnr(x, x, torch.ones(1, dtype=torch.bool))  # CPU mask
    with pytest.raises(ValueError):
        metrics.psnr(x, x, reduction="sum")


# ---- evaluate_image ------------------------------------------------------------------------------------------------------------
def _model_and_rays(n):
    from satnerf_amd.models import load_model

    args = O.default_args(n_samples=64, mlp_mode="bf16x3")
    m = load_model(args)
    m.load_state_dict(O.procedural_satnerf_params(args.fc_units, args.t_embbeding_tau, seed=1))
    emb = torch.nn.Embedding(args.t_embbeding_vocab, args.t_embbeding_tau)
    emb.load_state_dict({"weight": O.procedural_uniform((args.t_embbeding_vocab, args.t_embbeding_tau), 1.0, 7)})
    models = {"coarse": m.to(DEV).eval(), "t": emb.to(DEV)}
    rays, ts = O.synthetic_rays(n, seed=31)
    g = torch.Generator().manual_seed(32)
    draws = [torch.rand(n, 64, generator=g).to(DEV), torch.randn(n, 64, generator=g).to(DEV)]
    return models, args, rays.to(DEV), ts.to(DEV), draws


def _ecef(lat, lon, alt):
    a, e2 = 6378137.0, 6.69437999014e-3
    phi, lam = math.radians(lat), math.radians(lon)
    n = a / math.sqrt(1 - e2 * math.sin(phi) ** 2)
    return np.array([(n + alt) * math.cos(phi) * math.cos(lam), (n + alt) * math.cos(phi) * math.sin(lam), (n * (1 - e2) + alt) * math.sin(phi)])


def test_evaluate_image_matches_restatements_and_keeps_the_view_quirk():
    from satnerf_amd import rendering
    from satnerf_amd.evaluate import evaluate_image

    h, w = 20, 25
    models, args, rays, ts, draws = _model_and_rays(h * w)
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    img = np.stack([xx, yy, 0.5 + 0.5 * np.sin(8 * xx * yy)], -1).reshape(-1, 3)  # (N, 3) pixel-major, distinct channels
    rgbs = _t(img)
    with rendering.replay_rng(draws):
        res = evaluate_image(models, rays, ts, rgbs, h, w, args)
    with torch.no_grad(), rendering.replay_rng(draws):
        rgb = rendering.render_image_outputs(models, rays, ts, args)["rgb"]
    assert res["typ"] == "coarse" and res["mae"] is None and isinstance(res["psnr"], float) and isinstance(res["ssim"], float)
    assert torch.equal(res["outputs"]["rgb"], rgb)
    r, gt = rgb.cpu().numpy(), img.astype(np.float32)
    assert abs(res["psnr"] - psnr_np(r, gt)) <= 2e-7 * abs(psnr_np(r, gt))
    quirk = ssim_np(r.reshape(1, 3, h, w), gt.reshape(1, 3, h, w))  # the reference's .view(1, 3, H, W) of the (N, 3) buffer
    assert abs(res["ssim"] - quirk) <= 1e-6
    true_planes = ssim_np(r.T.reshape(1, 3, h, w), gt.T.reshape(1, 3, h, w))
    assert abs(res["ssim"] - true_planes) > 1e-3, (res["ssim"], true_planes)
    with pytest.raises(ValueError):
        evaluate_image(models, rays, ts, rgbs, h + 1, w, args)
    with pytest.raises(ValueError):
        evaluate_image(models, rays, ts, rgbs[:, :2], h, w, args)


def test_evaluate_image_dsm_mae():
    from satnerf_amd import dsm, rendering
    from satnerf_amd.evaluate import evaluate_image

    h, w = 20, 25
    models, args, rays, ts, draws = _model_and_rays(h * w)
    center, scene_range = _ecef(30.3, -81.7, 0.0), 300.0
    rgbs = torch.rand(h * w, 3, generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad(), rendering.replay_rng(draws):
        depth = rendering.render_image_outputs(models, rays, ts, args)["depth"]
    auto = dsm.dsm_from_depth(rays, depth, center, scene_range, resolution=2.0)
    side = max(auto.dsm.shape)
    roi = np.array([auto.xoff, auto.yoff - side * 2.0, side, 2.0])  # an {aoi}_DSM.txt grid around the cloud
    on_roi = dsm.dsm_from_depth(rays, depth, center, scene_range, roi=roi).dsm
    assert int(torch.isfinite(on_roi).sum()) > 0
    gt = torch.nan_to_num(on_roi, nan=float(torch.nanmean(on_roi))) + 0.25
    gt = gt + 0.1 * torch.rand(gt.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    want = dsm.dsm_mae(dsm.dsm_from_depth(rays, depth, center, scene_range, roi=roi), gt, register="xyz")[0]
    with rendering.replay_rng(draws):
        res = evaluate_image(models, rays, ts, rgbs, h, w, args, center=center, scene_range=scene_range, roi=roi, gt=gt)
    assert res["mae"] == want and math.isfinite(want)
    with pytest.raises(ValueError):
        evaluate_image(models, rays, ts, rgbs, h, w, args, gt=gt)  # no grid to put the DSM on
