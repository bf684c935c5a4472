"""The fused classic-NeRF forward (csrc/nerf_fwd.inc: sr_nerf_mlp_fwd, sr_nerf_render_fwd) on the GPU.

1. per point against the bf16-operand float64 chain of tests/nerf_reference.py on lively weights (the golden's weights give an almost
   constant network: tests/test_nerf_reference_host.py);
2. the render entry against the point entry between the stand-alone sampling / compositing kernels;
3. the reference's golden through render_rays in bf16 (a sanity check: the chain alone stays below 8.8e-4 on it);
4. the plumbing up to render_rays / batched_inference.
"""
import ctypes as C

import pytest
import torch

from oracle import satnerf_oracle as O
from tests import nerf_reference as R
from tests.helpers import golden_cfg, golden_draws, load_golden, maxnorm_rel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# Kernel against chain, max-norm relative, the largest over seeds 1-3 and both layouts, measured on the MI355X: rgb 3.22e-3, sigma
# 1.85e-3 (per case: rgb 1.86e-3 .. 3.22e-3, sigma 6.3e-4 .. 1.85e-3).  What separates the two is accumulation order and the bf16
# roundings it flips, which varies by about a factor of two from seed to seed (2.6e-3 .. 5.0e-3 between fp32 and fp64 accumulation on
# the CPU), so the gate is twice the measured value: rgb 6.44e-3, sigma 3.7e-3.  It may not exceed 1.5e-2, half the smallest planted
# fault (3e-2).
MEASURED_RGB, MEASURED_SIGMA = 3.22e-3, 1.85e-3
GATE_RGB, GATE_SIGMA = 2 * MEASURED_RGB, 2 * MEASURED_SIGMA
assert max(GATE_RGB, GATE_SIGMA) <= 1.5e-2


def _lazy():
    from satnerf_amd import ops, rendering
    from satnerf_amd.models import NeRF

    return ops, rendering, NeRF


def _model(params, feat=256):
    _, _, NeRF = _lazy()
    m = NeRF(feat=feat)
    m.load_state_dict(params)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def lively():
    return {seed: _model(R.lively_nerf_params(256, seed)) for seed in (1, 2, 3)}


_CHAIN = {}


def _chain(seed, p, row_div):
    key = (seed, p, row_div)
    if key not in _CHAIN:
        xyz, d = R.points(p, 100 + seed)
        d = d if row_div == 1 else d[:(p + row_div - 1) // row_div].contiguous()
        _CHAIN[key] = (xyz, d, R.chain(R.lively_nerf_params(256, seed), xyz, d, row_div))
    return _CHAIN[key]


# ---- 1. per point against the chain --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("p,row_div", [(261, 1), (250, 50)])  # 8 full waves + 5 points: ragged for a wave and for a workgroup | a direction per ray
def test_points_against_the_bf16_chain(lively, seed, p, row_div):
    ops, _, _ = _lazy()
    xyz, d, (rgb_ref, sigma_ref) = _chain(seed, p, row_div)
    model = lively[seed]
    rgb, sigma = ops.nerf_mlp(xyz.to(DEV), d.to(DEV), row_div, model.packed("bf16"))
    e_rgb, e_sigma = maxnorm_rel(rgb, rgb_ref), maxnorm_rel(sigma, sigma_ref)
    print(f"seed {seed} P {p} row_div {row_div}: rgb {e_rgb:.2e} sigma {e_sigma:.2e}")
    assert rgb.shape == (p, 3) and sigma.shape == (p,)
    assert e_rgb < GATE_RGB and e_sigma < GATE_SIGMA
    if row_div == 1:  # NeRF.forward is the same launch in the reference's (P, 4) layout
        out = model(xyz.to(DEV), input_dir=d.to(DEV), mlp_mode="bf16")
        assert out.shape == (p, 4) and torch.equal(out[:, :3], rgb) and torch.equal(out[:, 3], sigma)
        assert torch.equal(model(xyz.to(DEV), sigma_only=True, mlp_mode="bf16")[:, 0], sigma)


# ---- 2. the render entry equals the point entry ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise_std", [0.0, 0.3])
@pytest.mark.parametrize("n,s,i", [(33, 50, 7), (1, 2, 1)])
def test_render_entry_equals_point_entry(lively, n, s, i, noise_std):
    ops, _, _ = _lazy()
    stream = lively[1].packed("bf16")
    rays, _ = O.synthetic_rays(n, seed=11, classic=True)
    rays[:, :3] *= 2  # points out to ~[-8, 8]
    rays = rays.to(DEV)
    g = torch.Generator().manual_seed(5)
    u = torch.rand(n, s, generator=g).to(DEV)
    u2 = torch.rand(n, i, generator=g).to(DEV)
    noise = (torch.randn(n, s, generator=g).to(DEV), torch.randn(n, s + i, generator=g).to(DEV)) if noise_std else (None, None)

    def composed(z, nz):
        k = z.shape[1]
        rgbs, sigma = ops.nerf_mlp(ops.points_along(rays, 3, z), rays[:, 3:6], k, stream)
        w, t, depth, rgb = ops.composite(z, sigma.view(n, k), nz, noise_std, rgbs.view(n, k, 3), None, None, clamp_rgb=False)
        return {"rgb": rgb, "depth": depth, "weights": w, "transparency": t}

    def compare(got, want, what):
        for key, v in want.items():
            assert got[key].shape == v.shape
            e = maxnorm_rel(got[key], v)
            assert e < 1e-5, (what, key, e)

    coarse = ops.nerf_render_fwd(rays, s, stream, u=u, noise=noise[0], noise_std=noise_std, want_z=True)
    z = ops.ray_sample(rays, u, s)
    assert torch.equal(coarse["z"], z)
    compare(coarse, composed(z, noise[0]), "coarse")
    z_fine = torch.sort(torch.cat([z, rays[:, 6:7] + (rays[:, 7:8] - rays[:, 6:7]) * u2], 1), 1)[0].contiguous()
    fine = ops.nerf_render_fwd(rays, s + i, stream, z=z_fine, noise=noise[1], noise_std=noise_std)
    assert fine["z"] is z_fine
    compare(fine, composed(z_fine, noise[1]), "fine")
    assert ops.nerf_render_fwd(rays, s, stream, u=u)["z"] is None


# ---- 3. the reference's golden --------------------------------------------------------------------------------------------------------
def test_golden_coarse_and_fine_in_bf16():
    _, rendering, _ = _lazy()
    g = load_golden("nerf_coarse_fine")
    args = golden_cfg(g)
    assert args.model == "nerf" and args.n_importance > 0
    args.mlp_mode = "bf16"
    models = {typ: _model(O.procedural_nerf_params(args.fc_units, seed=seed)) for typ, seed in (("coarse", 1), ("fine", 2))}
    assert all(m.fused_forward("bf16") for m in models.values())
    draws = [d.to(DEV) for d in golden_draws(g)]
    with torch.no_grad(), rendering.replay_rng(draws) as rng:
        res = rendering.render_rays(models, args, g["rays"].to(DEV), None)
    assert rng.i == len(draws) == 4  # rand (N,S), randn (N,S), rand (N,I), randn (N,S+I): shapes are checked by the replay
    expected = {k[4:]: v for k, v in g.items() if k.startswith("out_")}
    assert set(res) == set(expected)
    worst = {k: maxnorm_rel(res[k].cpu(), v) for k, v in expected.items()}
    print({k: f"{e:.1e}" for k, e in worst.items()})
    assert all(res[k].shape == v.shape for k, v in expected.items())
    assert max(worst.values()) < 3e-3, worst


# ---- 4. plumbing ----------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    return O.default_args(model="nerf", **kw)


def _draws(n, s, i, seed=3):
    g = torch.Generator().manual_seed(seed)
    d = [torch.rand(n, s, generator=g), torch.randn(n, s, generator=g)]
    if i:
        d += [torch.rand(n, i, generator=g), torch.randn(n, s + i, generator=g)]
    return [t.to(DEV) for t in d]


def _render(models, args, rays, draws):
    _, rendering, _ = _lazy()
    with rendering.replay_rng(draws):
        return rendering.render_rays(models, args, rays, None)


def test_fused_forward_flags(lively):
    m = lively[1]
    assert m.fused_forward("bf16") and not m.fused_forward("bf16x3") and not m.fused_forward("f16")
    assert type(m).fused is False
    small = _model(O.procedural_nerf_params(128, seed=1), feat=128)
    assert not small.fused_forward("bf16")
    with pytest.raises(ValueError):
        small.packed("bf16")


def test_other_widths_and_grad_keep_the_layer_path(lively):
    rays = O.synthetic_rays(16, seed=2, classic=True)[0].to(DEV)
    small = {"coarse": _model(O.procedural_nerf_params(128, seed=1), feat=128), "fine": _model(O.procedural_nerf_params(128, seed=2), feat=128)}
    with torch.no_grad():
        a = _render(small, _args(fc_units=128, n_samples=8, n_importance=4, mlp_mode="bf16"), rays, _draws(16, 8, 4))
        b = _render(small, _args(fc_units=128, n_samples=8, n_importance=4), rays, _draws(16, 8, 4))
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    # grad enabled at the fused shape: the layer path + autograd, whatever the mode
    models = {"coarse": lively[1]}
    a = _render(models, _args(n_samples=8, n_importance=0, mlp_mode="bf16"), rays, _draws(16, 8, 0))
    b = _render(models, _args(n_samples=8, n_importance=0), rays, _draws(16, 8, 0))
    assert a["rgb_coarse"].grad_fn is not None and all(torch.equal(a[k], b[k]) for k in a)
    with torch.no_grad():
        c = _render(models, _args(n_samples=8, n_importance=0, mlp_mode="bf16"), rays, _draws(16, 8, 0))
    assert c["rgb_coarse"].grad_fn is None and not torch.equal(c["rgb_coarse"], a["rgb_coarse"])  # single-pass bf16 now


def test_weight_change_repacks():
    params = R.lively_nerf_params(256, 2)
    model = _model(params)
    rays = O.synthetic_rays(16, seed=4, classic=True)[0].to(DEV)
    args = _args(n_samples=8, n_importance=0, mlp_mode="bf16")
    with torch.no_grad():
        before = _render({"coarse": model}, args, rays, _draws(16, 8, 0))
        stream = model.packed("bf16")
        assert model.packed("bf16") is stream  # cached while the weights stand
        model.fc_net[6].weight.mul_(1.25)
        model.mark_weights_changed()
        after = _render({"coarse": model}, args, rays, _draws(16, 8, 0))
        params["fc_net.6.weight"] = params["fc_net.6.weight"] * 1.25
        fresh = _render({"coarse": _model(params)}, args, rays, _draws(16, 8, 0))
    assert not torch.equal(before["rgb_coarse"], after["rgb_coarse"])
    assert all(torch.equal(after[k], fresh[k]) for k in after)


def test_batched_inference_chunks(lively):
    _, rendering, _ = _lazy()
    n, s, i = 250, 8, 4
    rays = O.synthetic_rays(n, seed=6, classic=True)[0].to(DEV)
    models = {"coarse": lively[1], "fine": lively[2]}
    args = _args(n_samples=s, n_importance=i, mlp_mode="bf16", chunk=100)
    per_chunk = [_draws(k, s, i, seed=20 + c) for c, k in enumerate((100, 100, 50))]
    with rendering.replay_rng([d for ds in per_chunk for d in ds]):
        whole = rendering.batched_inference(models, rays, None, args)
    with torch.no_grad():
        parts = [_render(models, args, rays[100 * c:100 * c + 100], ds) for c, ds in enumerate(per_chunk)]
    assert set(whole) == set(parts[0])
    for k, v in whole.items():
        assert v.shape[0] == n and torch.equal(v, torch.cat([p[k] for p in parts], 0))


def test_empty_cpu_and_bad_arguments(lively):
    from satnerf_amd import _lib

    ops, rendering, _ = _lazy()
    stream = lively[1].packed("bf16")
    with torch.no_grad():
        res = rendering.render_rays({"coarse": lively[1], "fine": lively[2]}, _args(n_samples=8, n_importance=4, mlp_mode="bf16"),
                                    torch.empty(0, 8, device=DEV), None)
    assert res["rgb_coarse"].shape == (0, 3) and res["depth_fine"].shape == (0,) and res["weights_coarse"].shape == (0, 8)
    assert res["transparency_fine"].shape == (0, 12)
    rgb, sigma = ops.nerf_mlp(torch.empty(0, 3, device=DEV), torch.empty(0, 3, device=DEV), 1, stream)
    assert rgb.shape == (0, 3) and sigma.shape == (0,)
    rays = O.synthetic_rays(4, seed=1, classic=True)[0]
    with pytest.raises(ValueError):
        ops.nerf_mlp(torch.rand(4, 3), torch.rand(4, 3), 1, stream)
    with pytest.raises(ValueError):
        ops.nerf_render_fwd(rays, 8, stream, u=torch.rand(4, 8))
    with pytest.raises(RuntimeError):
        rendering.render_rays({"coarse": lively[1]}, _args(n_samples=8, n_importance=0, mlp_mode="bf16"), rays, None)
    with pytest.raises(ValueError):  # a ray's samples must fit a workgroup's points
        ops.nerf_render_fwd(rays.to(DEV), 300, stream, u=torch.rand(4, 300, device=DEV))
    with pytest.raises(ValueError):
        ops.nerf_mlp(torch.rand(100, 3, device=DEV), torch.rand(1, 3, device=DEV), 50, stream)  # too few direction rows
    # the C ABI refuses what it does not serve: a null pointer, another width
    lib = _lib.lib()
    r, u = rays.to(DEV), torch.rand(4, 8, device=DEV)
    w, t = torch.empty(4, 8, device=DEV), torch.empty(4, 8, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.sr_nerf_render_fwd(p(r), 8, 4, 8, p(u), None, None, 0.0, 256, None, None, None, None, p(w), p(t), st) != 0
    assert b"null" in lib.sr_last_error()
    assert lib.sr_nerf_render_fwd(p(r), 8, 4, 8, p(u), None, None, 0.0, 384, p(stream), None, None, None, p(w), p(t), st) != 0
    assert b"384" in lib.sr_last_error()
    assert lib.sr_nerf_render_fwd(p(r), 8, 4, 8, p(u), p(u), None, 0.0, 256, p(stream), None, None, None, p(w), p(t), st) != 0
    assert lib.sr_nerf_mlp_fwd(p(r), 8, p(r), 8, 1, 4, 384, p(stream), p(w), p(t), st) != 0
    torch.cuda.synchronize()
