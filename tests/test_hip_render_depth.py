"""Depth-only ("geometry") rendering on the GPU: the trunk-and-sigma cores (csrc/gen/fwd_core*.py heads=False) behind
sr_satnerf_render_depth / sr_satnerf_mlp_sigma, ops.render_depth / ops.satnerf_sigma, rendering.render_depth and the geometry_only
switch of the DSM entry points.

The tolerance against the full render is ZERO (torch.equal): the geometry stream feeds the sigma tile the same pieces in the same
k order as the full stream (tests/test_fwd_core_geometry.py holds the two SIG registers bit-equal on the lane model), softplus and
composite_ray are the full kernel's functions on the same LDS rows, and the reduction order of a ray does not depend on the colour
terms it leaves out.  Against the reference's goldens the bound is the gate tests/test_hip_parity.py applies to the same golden
in the same arithmetic, imported (BF16_RENDER_GATES) or read off the parity test that states it."""
import functools
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import satnerf_oracle as O
from tests import ortho_reference as R
from tests import test_hip_parity as P
from tests.helpers import golden_cfg, golden_draws, load_golden, maxnorm_rel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (width, samples, rays): the smallest shapes that reach every edge -- a workgroup owns 256 points at width 256 and 128 at width 512,
# so each case has more than one workgroup and a ragged last one (256 / 64 / 5: the second workgroup holds one live ray)
SHAPES = [(256, 64, 5), (256, 128, 3), (256, 32, 9), (512, 64, 3), (512, 128, 2)]


@functools.lru_cache(maxsize=None)
def _models(feat, tau, variant="sat-nerf", seed=21):
    """seeded random weights from the models' own init"""
    from satnerf_amd.models import load_model

    args = O.default_args(model=variant, fc_units=feat, t_embbeding_tau=tau)
    torch.manual_seed(seed + feat + tau)
    m = load_model(args).to(DEV).eval()
    if variant != "sat-nerf":
        return {"coarse": m}
    fine = load_model(args).to(DEV).eval()
    emb = torch.nn.Embedding(args.t_embbeding_vocab, tau).to(DEV)
    return {"coarse": m, "fine": fine, "t": emb}


def _sky(m):
    sk = m.sky_color
    return [sk[0].weight.data, sk[0].bias.data, sk[2].weight.data, sk[2].bias.data]


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("tau", [4, 16])
@pytest.mark.parametrize("feat,s,n", SHAPES)
def test_render_depth_is_bit_equal_to_the_full_render(feat, s, n, tau, mode):
    from satnerf_amd import ops

    models = _models(feat, tau)
    m, emb = models["coarse"], models["t"].weight.data
    hi, lo, l0 = m.packed(mode)
    rays, ts = O.synthetic_rays(n, seed=100 + n)
    rays, ts = rays.to(DEV), ts.to(DEV)
    g = torch.Generator().manual_seed(7 * s + n)
    u, noise = torch.rand(n, s, generator=g).to(DEV), torch.randn(n, s, generator=g).to(DEV)
    ctr = torch.tensor([3, 0, 0, 0], dtype=torch.float32, device=DEV)
    ways = [dict(u=u), dict(seed=5, step_counter=ctr)]
    if (feat, s) == (256, 128):  # the fine pass: given depths (sorted, inside the rays' bounds: another pass's merged depths)
        z = ops.render_depth(rays, ts, emb, s, feat, tau, mode, hi, lo, l0, u=torch.rand(n, s, generator=g).to(DEV))["z"]
        ways.append(dict(z=z.clone()))
    for noise_std in (0.0, 0.3):
        for way in ways:
            kw = dict(way, noise=noise if noise_std else None, noise_std=noise_std)
            full = ops.render_fwd(rays, ts, emb, s, feat, tau, mode, hi, lo, l0, *_sky(m), want_sigma=True, **kw)
            got = ops.render_depth(rays, ts, emb, s, feat, tau, mode, hi, lo, l0, want_sigma=True, **kw)  # (no sky weights: none are read)
            assert set(got) == {"z", "sigma", "weights", "transparency", "depth"}
            for k in got:
                assert got[k].shape == full[k].shape, k
                assert torch.equal(got[k], full[k]), (k, sorted(way), noise_std, float((got[k] - full[k]).abs().max()))
            assert torch.isfinite(got["depth"]).all() and float(got["weights"].sum()) > 0
            assert int(ctr[0].item()) == 3  # no tick asked for


@pytest.mark.parametrize("mode", ["bf16", "f16", "bf16x3"])
@pytest.mark.parametrize("feat,tau", [(256, 4), (256, 16), (512, 4), (512, 16)])
def test_sigma_launch_is_bit_equal_to_the_full_point_launch(feat, tau, mode):
    """P = 70: two full tiles and a partial one.  Also through SatNeRF.forward(sigma_only=True), whose bits must be what they were."""
    from satnerf_amd import ops

    m = _models(feat, tau)["coarse"]
    if not m.fused_forward(mode):
        assert (feat, mode) == (512, "bf16x3")
        return
    hi, lo, l0 = m.packed(mode)
    g = torch.Generator().manual_seed(70 + tau)
    x, t = (torch.rand(70, 3, generator=g) * 2 - 1).to(DEV), torch.rand(70, tau, generator=g).to(DEV)
    sun = torch.nn.functional.normalize(torch.randn(70, 3, generator=g), dim=1).to(DEV)
    want = ops.satnerf_mlp(x, None, sun, None, t, None, 70, 1, feat, tau, mode, hi, lo, l0)[1]
    got = ops.satnerf_sigma(x, None, sun, None, t, None, 70, 1, feat, tau, mode, hi, lo, l0)
    assert got.shape == want.shape == (70,) and torch.equal(got, want), float((got - want).abs().max())
    with torch.no_grad():
        only = m(x, input_sun_dir=sun, input_t=t, sigma_only=True, mlp_mode=mode)
        every = m(x, input_sun_dir=sun, input_t=t, mlp_mode=mode)
    assert only.shape == (70, 1) and torch.equal(only[:, 0], want) and torch.equal(every[:, 3], want)
    assert ops.satnerf_sigma(x[:0], None, sun[:0], None, t[:0], None, 0, 1, feat, tau, mode, hi, lo, l0).shape == (0,)


@pytest.mark.parametrize("tau", [4, 16])
def test_parity_mode_serves_a_depth_only_request_with_its_full_kernel(tau):
    """SR_MODE_BF16X3 has no geometry core: the C entry runs the parity kernel under the render pass with rgb, sky, albedo, sun_v and beta
    null (and asks for the sky weights, which that kernel evaluates).  The full render's bits; 5 rays x 64: a ragged second workgroup."""
    from satnerf_amd import _lib, ops

    models = _models(256, tau)
    m, emb = models["coarse"], models["t"].weight.data
    hi, lo, l0 = m.packed("bf16x3")
    rays, ts = O.synthetic_rays(5, seed=105)
    rays, ts = rays.to(DEV), ts.to(DEV)
    g = torch.Generator().manual_seed(8)
    u, noise = torch.rand(5, 64, generator=g).to(DEV), torch.randn(5, 64, generator=g).to(DEV)
    for kw in (dict(u=u), dict(u=u, noise=noise, noise_std=0.3)):
        full = ops.render_fwd(rays, ts, emb, 64, 256, tau, "bf16x3", hi, lo, l0, *_sky(m), want_sigma=True, **kw)
        got = ops.render_depth(rays, ts, emb, 64, 256, tau, "bf16x3", hi, lo, l0, sky=_sky(m), want_sigma=True, **kw)
        for k in got:
            assert torch.equal(got[k], full[k]), (k, sorted(kw))
    with pytest.raises(_lib.SatRenderError, match="sky head"):
        ops.render_depth(rays, ts, emb, 64, 256, tau, "bf16x3", hi, lo, l0, u=u)


def test_shadow_nerf_sigma_only_keeps_its_bits():
    m = _models(256, 4, "s-nerf")["coarse"]
    x = torch.rand(70, 3, device=DEV) * 2 - 1
    sun = torch.nn.functional.normalize(torch.randn(70, 3, device=DEV), dim=1)
    with torch.no_grad():
        only, every = m(x, input_sun_dir=sun, sigma_only=True, mlp_mode="bf16"), m(x, input_sun_dir=sun, mlp_mode="bf16")
    assert only.shape == (70, 1) and every.shape == (70, 8) and torch.equal(only[:, 0], every[:, 3])


# ---- against the reference's own depths ----------------------------------------------------------------------------------------
def _stated(test, pattern, which=0):
    """the bound a parity test states in its source.  tests/test_hip_parity.py names only BF16_RENDER_GATES; its f16 and width-512 gates
    are literals inside assert lines, and existing test files are not edited, so they are read from the source text here rather than
    copied.  This is brittle on purpose: it depends on the spelling of those lines (and, at width 512, on bf16 coming before f16) and
    fails at import when they change -- the day they get names in a shared helper, import those instead."""
    found = re.findall(pattern, inspect.getsource(test))
    assert found, (test.__name__, pattern)
    return float(found[which])


F16_GATE = _stated(P.test_f16_mode_matches_reference_goldens_eight_times_closer_than_bf16, r'\("rgb", "depth", "weights"\)\) < ([0-9.e-]+)')
W512_GATES = {"bf16": _stated(P.test_width_512_fused_forward_kernel, r'"depth_coarse", "weights_coarse"\)\) < ([0-9.e-]+)', 0),
              "f16": _stated(P.test_width_512_fused_forward_kernel, r'"depth_coarse", "weights_coarse"\)\) < ([0-9.e-]+)', 1)}
GOLDEN_CASES = [(name, mode) for name in ("satnerf_coarse", "satnerf_sc", "satnerf_fine", "satnerf_noise", "satnerf_s128", "satnerf_feat512")
                for mode in ("bf16", "f16")]


def _golden_gate(name, mode):
    if name == "satnerf_feat512":
        return W512_GATES[mode]
    return P.BF16_RENDER_GATES["depth"] if mode == "bf16" else F16_GATE


@pytest.mark.parametrize("name,mode", GOLDEN_CASES)
def test_render_depth_reproduces_the_reference_depth(name, mode):
    """every sat-nerf golden with a depth at a fused width; satnerf_fine runs coarse -> resample -> fine, satnerf_sc has the draw of a
    pass that is skipped here, satnerf_noise the density noise"""
    from satnerf_amd import rendering

    g = load_golden(name)
    args = golden_cfg(g)
    args.mlp_mode = mode
    models = P.build_models(args)
    typ = "fine" if args.n_importance > 0 else "coarse"
    with rendering.replay_rng([d.to(DEV) for d in golden_draws(g)]) as rng:
        got = rendering.render_depth(models, g["rays"].to(DEV), g["ts"].to(DEV), args, return_weights=True)
    assert rng.i == len(rng.draws) and got["typ"] == typ
    err = maxnorm_rel(got["depth"].cpu(), g[f"out_depth_{typ}"])
    werr = maxnorm_rel(got["weights"].cpu(), g[f"out_weights_{typ}"])
    print(f"{name} {mode}: depth {err:.2e} (gate {_golden_gate(name, mode):g}), weights {werr:.2e}")
    assert err < _golden_gate(name, mode), err
    assert got["depth"].shape == (g["rays"].shape[0],) and got["weights"].shape == g[f"out_weights_{typ}"].shape == got["z"].shape
    assert torch.allclose(got["acc"], got["weights"].sum(-1))
    with torch.no_grad(), rendering.replay_rng([d.to(DEV) for d in golden_draws(g)]):
        full = rendering.render_rays(models, args, g["rays"].to(DEV), g["ts"].to(DEV))
    for k in ("depth", "weights", "transparency"):  # the same seed gives the depths of the full render
        assert torch.equal(got[k], full[f"{k}_{typ}"]), k


# ---- public paths ----------------------------------------------------------------------------------------------------------------
def _scene_models(mode="bf16", **kw):
    args = O.default_args(n_samples=64, fc_units=256, mlp_mode=mode, **kw)
    models = _models(256, 4)
    return args, ({k: models[k] for k in ("coarse", "t")} if args.n_importance == 0 else models)


def test_render_dsm_geometry_only():
    from satnerf_amd import dsm, rendering
    from tests.test_hip_dsm import ecef_from_geodetic

    args, models = _scene_models(chunk=200)  # three chunks, the last ragged
    rays, ts = O.synthetic_rays(500, seed=31)
    rays, ts = rays.to(DEV), ts.to(DEV)
    center = ecef_from_geodetic(np.array(30.3), np.array(-81.7), np.array(0.0))
    torch.manual_seed(4)
    got = dsm.render_dsm(models, rays, ts, args, center, 300.0, geometry_only=True, resolution=2.0)
    torch.manual_seed(4)
    depth = rendering.render_depth(models, rays, ts, args)["depth"]
    want = dsm.dsm_from_depth(rays, depth, center, 300.0, resolution=2.0)
    assert torch.equal(got.dsm.view(torch.int32), want.dsm.view(torch.int32)) and torch.equal(got.weight, want.weight)
    assert int(torch.isfinite(got.dsm).sum()) > 0
    torch.manual_seed(4)
    fused = dsm.render_fused_dsm(models, [(rays, ts)], args, center, 300.0, geometry_only=True, resolution=2.0)
    assert fused.dsm.shape == got.dsm.shape and int(torch.isfinite(fused.dsm).sum()) > 0
    # the default is the full render, and it gives the same depth on the same draws
    torch.manual_seed(4)
    full = rendering.render_image_outputs(models, rays, ts, args)["depth"]
    assert torch.equal(full, depth)


def test_render_ortho_dsm_geometry_only():
    from satnerf_amd import data, dsm, rendering

    args, models = _scene_models()
    s = R.jax(6, 5)
    n = s["grid"][2] * s["grid"][3]
    common = (s["center"], s["scene_range"], s["min_alt"], s["max_alt"], s["sun_d"])
    torch.manual_seed(0)
    got, outputs = dsm.render_ortho_dsm(models, 3, args, *common, grid=s["grid"], zone=17, geometry_only=True)
    torch.manual_seed(0)
    by_hand = rendering.render_depth(models, data.ortho_rays(device=DEV, **s), torch.full((n,), 3, dtype=torch.int64, device=DEV), args)
    want = dsm.ortho_dsm_from_depth(by_hand["depth"], s["grid"], s["max_alt"], s["scene_range"], zone="17")
    assert n == 30 and set(outputs) == {"depth", "acc"}
    assert torch.equal(got.dsm.view(torch.int32), want.dsm.view(torch.int32)) and torch.equal(got.weight, want.weight)
    assert torch.equal(outputs["depth"], by_hand["depth"]) and torch.isfinite(got.dsm).all()


def test_no_rays_give_empty_results():
    from satnerf_amd import ops, rendering

    args, models = _scene_models(n_importance=64)
    m, emb = models["coarse"], models["t"].weight.data
    hi, lo, l0 = m.packed("bf16")
    rays, ts = torch.empty(0, 11, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV)
    o = ops.render_depth(rays, ts, emb, 64, 256, 4, "bf16", hi, lo, l0, u=torch.empty(0, 64, device=DEV))
    assert o["depth"].shape == (0,) and o["weights"].shape == (0, 64) and o["z"].shape == (0, 64)
    out = rendering.render_depth(models, rays, ts, args, return_weights=True)
    assert out["typ"] == "fine" and out["depth"].shape == out["acc"].shape == (0,) and out["weights"].shape == out["z"].shape == (0, 128)
    torch.cuda.synchronize()


# ---- fallbacks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,kw", [("layer path", dict(fc_units=128, mlp_mode="bf16")), ("parity mode", dict(mlp_mode="bf16x3")),
                                     ("samples that do not divide the workgroup", dict(n_samples=50, mlp_mode="bf16")),
                                     ("classic nerf", dict(model="nerf", mlp_mode="bf16x3")), ("s-nerf", dict(model="s-nerf", mlp_mode="bf16"))])
def test_render_depth_never_fails_for_lack_of_the_geometry_kernel(what, kw):
    """what the depth-only kernel does not cover renders through render_rays (s-nerf rides on the Sat-NeRF kernels and does get the
    geometry core): same keys, and the depth of render_rays under the same draws, bit for bit.  n_samples = 50 is served by the fallback
    here; through ops.render_depth it raises the C entry's message (below)."""
    from satnerf_amd import rendering
    from satnerf_amd.models import load_model

    args = O.default_args(**kw)
    torch.manual_seed(9)
    models = {"coarse": load_model(args).to(DEV).eval()}
    if args.model == "sat-nerf":
        models["t"] = torch.nn.Embedding(args.t_embbeding_vocab, args.t_embbeding_tau).to(DEV)
    n, s = 37, args.n_samples
    rays, ts = O.synthetic_rays(n, seed=12)
    rays, ts = (rays[:, :8] if args.model == "nerf" else rays).to(DEV), (ts.to(DEV) if args.model == "sat-nerf" else None)
    g = torch.Generator().manual_seed(13)
    draws = [torch.rand(n, s, generator=g).to(DEV), torch.randn(n, s, generator=g).to(DEV)]
    with rendering.replay_rng(draws):
        got = rendering.render_depth(models, rays, ts, args, return_weights=True)
    with torch.no_grad(), rendering.replay_rng(draws):
        want = rendering.render_rays(models, args, rays, ts)
    assert set(got) == {"typ", "depth", "acc", "weights", "transparency", "z"} and got["typ"] == "coarse"
    assert torch.equal(got["depth"], want["depth_coarse"]) and torch.equal(got["weights"], want["weights_coarse"])
    assert got["z"].shape == (n, s) and bool((got["z"][:, 1:] >= got["z"][:, :-1]).all())
    assert torch.allclose(got["depth"], (got["weights"] * got["z"]).sum(-1), rtol=1e-5, atol=1e-6)
    # under kernel_rng too (the depths cannot be kept from a kernel's own draw: these chunks draw on the host), and never a bank
    with rendering.kernel_rng(5, torch.zeros(4, device=DEV)):
        k = rendering.render_depth(models, rays, ts, args, return_weights=True)
    assert torch.allclose(k["depth"], (k["weights"] * k["z"]).sum(-1), rtol=1e-5, atol=1e-6) and bool((k["z"][:, 1:] >= k["z"][:, :-1]).all())
    with rendering.kernel_rng(5, torch.zeros(4, device=DEV), bank_chunks=2), pytest.raises(NotImplementedError):
        rendering.render_depth(models, rays, ts, args)


V1_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import torch
from oracle import satnerf_oracle as O
from satnerf_amd import ops
from satnerf_amd.models import load_model
for feat, tau, s, n in ((256, 4, 64, 5), (512, 16, 64, 3)):
    args = O.default_args(fc_units=feat, t_embbeding_tau=tau)
    torch.manual_seed(3)
    m = load_model(args).cuda().eval()
    emb = torch.rand(30, tau, device="cuda")
    hi, lo, l0 = m.packed("bf16")
    sk = m.sky_color
    sky = [sk[0].weight.data, sk[0].bias.data, sk[2].weight.data, sk[2].bias.data]
    rays, ts = O.synthetic_rays(n, seed=2)
    rays, ts, u = rays.cuda(), ts.cuda(), torch.rand(n, s, device="cuda")
    full = ops.render_fwd(rays, ts, emb, s, feat, tau, "bf16", hi, lo, l0, *sky, u=u, want_sigma=True)
    got = ops.render_depth(rays, ts, emb, s, feat, tau, "bf16", hi, lo, l0, sky=sky, u=u, want_sigma=True)
    for k in got:
        assert torch.equal(got[k], full[k]), (feat, k)
    x = torch.rand(70, 3, device="cuda")
    a = ops.satnerf_mlp(x, None, x, None, torch.rand(70, tau, device="cuda").mul_(0).add_(0.5), None, 70, 1, feat, tau, "bf16", hi, lo, l0)[1]
    b = ops.satnerf_sigma(x, None, x, None, torch.full((70, tau), 0.5, device="cuda"), None, 70, 1, feat, tau, "bf16", hi, lo, l0)
    assert torch.equal(a, b), feat
    try:
        ops.render_depth(rays, ts, emb, s, feat, tau, "bf16", hi, lo, l0, u=u)
    except Exception as e:
        assert "sky head" in str(e), e
    else:
        raise AssertionError("the full kernel was handed no sky weights")
torch.cuda.synchronize()
print("v1 ok")
"""


def test_scheduled_route_serves_a_depth_only_request():
    """SATNERF_FWD_V1=1 is read once per process: a fresh child, under its own time limit.  There a depth-only request runs the
    compiler-scheduled full kernel with the unused outputs null -- the full render's bits -- and needs the sky weights."""
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", V1_CHILD, ROOT], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, SATNERF_FWD_V1="1"))
    assert r.returncode == 0 and "v1 ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from satnerf_amd import _lib, ops, rendering

    args, models = _scene_models()
    rays, ts = O.synthetic_rays(5, seed=1)
    rays, ts = rays.to(DEV), ts.to(DEV)
    bad = ts.clone()
    bad[2] = args.t_embbeding_vocab
    with pytest.raises(IndexError):
        rendering.render_depth(models, rays, bad, args)
    with pytest.raises(TypeError):
        rendering.render_depth(models, rays, None, args)
    with pytest.raises(ValueError):
        rendering.render_depth(models, rays, ts, O.default_args(model="bogus"))
    m, emb = models["coarse"], models["t"].weight.data
    hi, lo, l0 = m.packed("bf16")
    with pytest.raises(_lib.SatRenderError, match="n_samples=50 must be >= 2 and divide 256"):
        ops.render_depth(rays, ts, emb, 50, 256, 4, "bf16", hi, lo, l0, u=torch.rand(5, 50, device=DEV))
    with pytest.raises(ValueError):
        ops.render_depth(rays, ts, emb, 64, 256, 4, "bf16", hi, lo, l0, u=torch.rand(5, 32, device=DEV))
