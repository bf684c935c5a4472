"""Geometric sun visibility on the GPU: sr_sun_rays and sr_sun_shade against the restatements of
tests/sun_rays_reference.py, rendering.render_sun_visibility against the chain of launches it stands for (tolerance zero) and against
the CPU oracle, and the ``shadows=`` keyword of evaluate.sun_interp_shadows and dsm.render_ortho_dsm.

The gates against the oracle are measured, not derived (BF16_RENDER_GATES has no transparency entry and a field this sharp is not the
goldens' field): max |GPU - oracle| of the visibility on cape_town(37, 53), sun elevation 25 deg, azimuth 140 deg, S = 64, u = 0.5,
default bias, procedural weights (seed 1) with the density row times 64.  Beside each figure stands the same error of the PRIMARY pass's
transparency[:, -1] -- the same kernel on the camera rays, from the same run and the same oracle.  Each gate is twice the measured
sun-pass error (the factor covers the differences between machines; a sign or frame error moves visibilities by tenths).

    width  mode     sun pass    primary pass   gate        (sun pass from the oracle's depths, depth error: context, not gated)
    256    bf16     4.067e-02   3.571e-03      8.134e-02   1.378e-02   3.403e-03
    256    f16      5.214e-03   5.593e-04      1.043e-02   3.155e-03   4.722e-04
    256    bf16x3   5.549e-05   3.099e-06      1.110e-04   1.997e-05   4.426e-06
    512    bf16     5.177e-02   1.899e-02      1.035e-01   1.240e-02   1.721e-03
    512    f16      6.855e-03   2.183e-03      1.371e-02   2.762e-03   2.531e-04

At width 256 the sun pass stands 9 to 18 times above its primary companion, beyond the factor of ten that asks for an explanation.  It
has two parts, both measured.  (1) The companion is a saturated number on this field: at width 256 the primary
rays' transparency[:, -1] lies below 0.12 on every ray (median 0.003), while the visibilities spread over 0 .. 1.  A relative error of
a ray's optical depth tau moves its transmittance T by T tau: mean 0.047 over the primary rays against 0.19 over the sun rays, which
is the factor of 4 to 6 between the primary pass and the sun pass started from the oracle's own depths; at width 512, where the primary
transparencies spread as widely as the visibilities (mean T tau 0.23 against 0.18), that factor is 0.7 to 1.3.  (2) The rest is the
primary pass's depth error carried into the start of the sun ray: on the oracle alone, moving the depths by 1e-3 moves a visibility by
up to 0.035 (width 256) and 0.038 (width 512), so the depth errors in the last column account for up to 0.12 (bf16), 1.7e-2 (f16) and
1.6e-4 (bf16x3), above what is seen.  Neither is arithmetic of the sun pass: its rays are within one fp32 ulp of the restatement.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import satnerf_oracle as O
from tests import sun_rays_reference as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ORACLE_GATES = {(256, "bf16"): 8.134e-2, (256, "f16"): 1.043e-2, (256, "bf16x3"): 1.110e-4, (512, "bf16"): 1.035e-1, (512, "f16"): 1.371e-2}
BIAS_REL = 1 / 64  # the default bias at S = 64: one interval of the primary ray


def _t(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _scene_args(sc):
    s = sc["s"]
    return s["center"], s["scene_range"], s["max_alt"]


@functools.lru_cache(maxsize=None)
def _per_ray(name):
    """The scene's rays with a sun vector of their own each: the scene's direction at lengths from 0.5 to 1.5 (s need not be a unit
    vector).  Read-only."""
    sc = S.scene(name)
    rays = sc["rays"].copy()
    rays[:, 8:11] *= np.linspace(0.5, 1.5, rays.shape[0], dtype=np.float32)[:, None]
    rays.setflags(write=False)
    return rays


# ---- sr_sun_rays ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call_sun", [False, True])
@pytest.mark.parametrize("n", [0, 1, 257, 37 * 53])  # 257: the one-lane tail of a second 256-thread block
@pytest.mark.parametrize("name", ["jax", "cape_town"])
def test_sun_rays_match_restatement(name, n, call_sun):
    from satnerf_amd import data, ops

    sc = S.scene(name)
    scene = _scene_args(sc)
    rays_np, depth_np = _per_ray(name)[:n], sc["depth"][:n]
    sun = tuple(2.0 * sc["sun"]) if call_sun else None
    rays, depth = _t(rays_np).view(n, 11), _t(depth_np)
    got, valid, lla = data.sun_rays(rays, depth, *scene, sun_d=sun, n_samples=64, return_valid=True, return_latlonalt=True)
    assert got.shape == (n, 11) and got.dtype == torch.float32 and valid.shape == (n,) and valid.dtype == torch.bool
    assert lla.shape == (3, n) and lla.dtype == torch.float64
    if n == 0:
        return
    want, want_valid, _ = S.sun_rays_np(rays_np, depth_np, *scene, sun_d=sun, bias_rel=BIAS_REL)
    g = got.cpu().numpy()
    ok = S.within_one_ulp(g[:, :8], want[:, :8])
    assert ok.all(), (np.argwhere(~ok)[:5], g[:, :8][~ok][:5], want[:, :8][~ok][:5])
    assert want_valid.all() and bool(valid.all())
    near = (BIAS_REL * (rays_np[:, 7].astype(np.float64) - rays_np[:, 6].astype(np.float64))).astype(np.float32)
    assert (g[:, 6].view(np.uint32) == near.view(np.uint32)).all()  # exactly float32 of its formula
    assert (g[:, 7] > g[:, 6]).all()
    sun32 = want[:, 8:11].astype(np.float32)  # the primary row's columns, or the call's vector as given (not normalised)
    assert (g[:, 8:11].view(np.uint32) == sun32.view(np.uint32)).all()
    assert torch.equal(lla, torch.stack(ops.latlonalt_from_depth(rays, depth, scene[0], scene[1])))  # bit for bit
    # a 13-column buffer (the image buffer's width): columns 11:13 keep their sentinel, the rest is the same bytes as before
    buf = torch.full((n, 13), -7.25, dtype=torch.float32, device=DEV)
    view = data.sun_rays(rays, depth, *scene, sun_d=sun, n_samples=64, out=buf)
    assert view.shape == (n, 11) and view.data_ptr() == buf.data_ptr()
    assert torch.equal(_bits(buf[:, :11]), _bits(got)) and bool((buf[:, 11:] == -7.25).all())
    with pytest.raises(ValueError, match="storage"):
        data.sun_rays(rays, depth, *scene, sun_d=sun, n_samples=64, out=rays)
    again = data.sun_rays(rays, depth, *scene, sun_d=sun, n_samples=64)
    assert torch.equal(_bits(again), _bits(got))
    # an absolute bias
    fixed = data.sun_rays(rays, depth, *scene, sun_d=sun, bias=0.003)
    assert bool((fixed[:, 6] == np.float32(0.003)).all()) and torch.equal(_bits(fixed[:, :6]), _bits(got[:, :6]))


def test_invalid_sun_rays_are_finite_zero_length_rays():
    """sr_sun_rays only: no planted value is ever fed to an MLP kernel."""
    from satnerf_amd import data

    sc = S.scene("cape_town")
    scene = _scene_args(sc)
    n = 300
    clean_rays, clean_depth = _per_ray("cape_town")[:n], sc["depth"][:n]
    rays, depth = clean_rays.copy(), clean_depth.copy()
    depth[1], depth[2], depth[255] = np.nan, np.inf, -np.inf
    rays[4, 8:11] = 0.0
    rays[256, 8:11] = (0.3, 0.4, -0.1)  # below the horizon
    rays[6, 8:11] = (0.3, 0.4, 0.0)  # on it
    rays[7, 8:11] = (np.nan, 0.4, 0.5)
    rays[299, 8:11] = (np.inf, 0.4, 0.5)
    depth[9], depth[10] = -0.01, 0.0  # above max_alt, and at the ray's origin on it: valid, far == near
    bad = np.zeros(n, bool)
    bad[[1, 2, 255, 4, 256, 6, 7, 299]] = True
    got, valid = data.sun_rays(_t(rays), _t(depth), *scene, n_samples=64, return_valid=True)
    g = got.cpu().numpy()
    want, want_valid, _ = S.sun_rays_np(rays, depth, *scene, bias_rel=BIAS_REL)
    assert (want_valid == ~bad).all() and (valid.cpu().numpy() == ~bad).all()
    assert np.isfinite(g[bad, 0:8]).all() and (g[bad, 0:6].view(np.uint32) == rays[bad, 0:6].view(np.uint32)).all()
    assert (g[bad, 6:8].view(np.uint32) == 0).all()  # near = far = +0
    assert (g[:, 8:11].view(np.uint32) == rays[:, 8:11].view(np.uint32)).all()  # the sun columns, NaN included, unchanged
    assert g[9, 7] == g[9, 6] > 0 and g[10, 7] == g[10, 6] > 0
    assert S.within_one_ulp(g[~bad, :8], want[~bad, :8]).all()
    # every valid row is what it is without the planted neighbours
    clean = data.sun_rays(_t(clean_rays), _t(clean_depth), *scene, n_samples=64).cpu().numpy()
    same = ~bad
    same[[9, 10]] = False
    assert (g[same].view(np.uint32) == clean[same].view(np.uint32)).all()
    # a call-level sun overrides the planted sun columns: only the depths stay invalid
    _, valid2 = data.sun_rays(_t(rays), _t(depth), *scene, sun_d=sc["sun"], n_samples=64, return_valid=True)
    assert (~valid2).nonzero().flatten().tolist() == [1, 2, 255]


# ---- sr_sun_shade --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 257])
def test_sun_shade_is_bit_equal_to_the_restatement(n):
    from satnerf_amd import ops

    rng = np.random.default_rng(50 + n)
    image = rng.uniform(0, 1, (n, 13)).astype(np.float32)  # the image buffer's layout: albedo in columns 6:9, sky in 10:13
    image[:, 6:9] = rng.uniform(-0.3, 1.6, (n, 3))
    vis = rng.uniform(0, 1, n).astype(np.float32)
    if n > 1:
        vis[5], vis[6], vis[7], vis[256] = np.nan, 1.0, 0.0, 0.5
        image[6, 6:9], image[256, 6:9] = (1.5, -0.2, 0.5), (2.5, -1.0, 1.0)
    dev = _t(image).view(n, 13) if n else torch.empty(0, 13, device=DEV)
    a0, a1 = ops.IMAGE_COLUMNS["albedo"]
    s0, s1 = ops.IMAGE_COLUMNS["sky"]
    got = ops.sun_shade(dev[:, a0:a1], dev[:, s0:s1], _t(vis))
    assert got.shape == (n, 3) and got.dtype == torch.float32
    want = S.shade_np(image[:, a0:a1], image[:, s0:s1], vis)
    g = got.cpu().numpy()
    nan = np.isnan(want)
    assert (np.isnan(g) == nan).all() and (g[~nan].view(np.uint32) == want[~nan].view(np.uint32)).all()
    if n > 1:
        assert np.isnan(g[5]).all() and nan.sum() == 3  # NaN in gives NaN out, and nowhere else
        assert (g[6] == [1.0, 0.0, 0.5]).all() and g[~nan].min() == 0.0 and g[~nan].max() == 1.0  # both clamps are reached
        col = ops.sun_shade(dev[:, a0:a1], dev[:, s0:s1], _t(vis).view(n, 1), out=torch.full((n, 5), -7.25, device=DEV))
        assert col.shape == (n, 3) and (np.isnan(col.cpu().numpy()) == nan).all() and torch.equal(_bits(col)[~_t(nan, torch.bool)], _bits(got)[~_t(nan, torch.bool)])


# ---- render_sun_visibility against the chain it stands for, tolerance zero -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _models(feat, seed=21):
    """seeded random weights from the models' own init"""
    from satnerf_amd.models import load_model

    args = O.default_args(fc_units=feat)
    torch.manual_seed(seed + feat)
    return {"coarse": load_model(args).to(DEV).eval(), "fine": load_model(args).to(DEV).eval(),
            "t": torch.nn.Embedding(args.t_embbeding_vocab, 4).to(DEV)}


@functools.lru_cache(maxsize=None)
def _view(xsize=32, ysize=16):
    """(scene, rays (N, 11) on the GPU, ts): a nadir view over cape_town with the low sun of the oracle test."""
    sc = S.scene("cape_town", xsize, ysize)
    n = xsize * ysize
    return sc, _t(sc["rays"]), (torch.arange(n, device=DEV) % 7).long()


def _midpoint_draws(n_total, chunk, s, n_imp=0):
    """what a ``replay_rng`` feeds a render without perturbation, chunk by chunk: 0.5 for the stratified jitter, (i + 0.5) / n_imp for
    the importance draws, 0 for the noise"""
    draws = []
    for i in range(0, n_total, chunk):
        n = min(chunk, n_total - i)
        draws += [torch.full((n, s), 0.5), torch.zeros(n, s)]
        if n_imp:
            draws += [((torch.arange(n_imp, dtype=torch.float64) + 0.5) / n_imp).float().expand(n, n_imp), torch.zeros(n, s + n_imp)]
    return draws


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("feat", [256, 512])
def test_sun_visibility_is_the_chain_of_its_launches(feat, mode):
    """512 rays in chunks of 200: two full chunks and a ragged tail."""
    from satnerf_amd import data, ops, rendering

    sc, rays, ts = _view()
    scene = _scene_args(sc)
    n, s, chunk = rays.shape[0], 64, 200
    args = O.default_args(n_samples=s, fc_units=feat, mlp_mode=mode, chunk=chunk)
    models = {k: v for k, v in _models(feat).items() if k != "fine"}
    assert ops.render_fused_ok(feat, mode, s)
    cpu_state, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    got = rendering.render_sun_visibility(models, rays, ts, args, *scene)
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(DEV), gpu_state)  # no draw
    assert set(got) == {"typ", "depth", "sun_geo", "valid"} and got["typ"] == "coarse"
    assert got["sun_geo"].shape == got["depth"].shape == got["valid"].shape == (n,) and got["valid"].dtype == torch.bool
    # by hand: render_depth, then data.sun_rays, then the geometry launch at u = 0.5 chunk by chunk
    with rendering.replay_rng(_midpoint_draws(n, chunk, s)):
        depth = rendering.render_depth(models, rays, ts, args)["depth"]
    srays, valid = data.sun_rays(rays, depth, *scene, n_samples=s, return_valid=True)
    m, emb = models["coarse"], models["t"].weight.data
    hi, lo, l0 = m.packed(mode)
    want = torch.cat([ops.render_depth(srays[i:i + chunk].contiguous(), ts[i:i + chunk], emb, s, feat, 4, mode, hi, lo, l0,
                                       u=torch.full((min(chunk, n - i), s), 0.5, device=DEV))["transparency"][:, -1] for i in range(0, n, chunk)])
    assert bool(valid.all()) and torch.equal(got["valid"], valid) and torch.equal(got["depth"], depth)
    assert torch.equal(got["sun_geo"], want), float((got["sun_geo"] - want).abs().max())
    assert bool(((want >= 0) & (want <= 1)).all())
    again = rendering.render_sun_visibility(models, rays, ts, args, *scene)
    assert torch.equal(again["sun_geo"], got["sun_geo"]) and torch.equal(again["depth"], got["depth"])
    given = rendering.render_sun_visibility(models, rays, ts, args, *scene, depth=depth)
    assert torch.equal(given["sun_geo"], got["sun_geo"])
    # a call-level sun is the per-ray sun it replaces
    call = rendering.render_sun_visibility(models, rays, ts, args, *scene, depth=depth, sun_d=sc["s"]["sun_d"])
    assert torch.equal(call["sun_geo"], got["sun_geo"])
    if (feat, mode) == (256, "bf16"):  # perturb=True draws as render_depth does: primary pass, then sun pass
        torch.manual_seed(5)
        drawn = rendering.render_sun_visibility(models, rays, ts, args, *scene, perturb=True)
        torch.manual_seed(5)
        d2 = rendering.render_depth(models, rays, ts, args)["depth"]
        v2 = rendering.render_depth(models, data.sun_rays(rays, d2, *scene, n_samples=s), ts, args, return_weights=True)["transparency"][:, -1]
        assert torch.equal(drawn["depth"], d2) and torch.equal(drawn["sun_geo"], v2) and not torch.equal(drawn["sun_geo"], got["sun_geo"])


@pytest.mark.parametrize("what,kw", [("layer path", dict(fc_units=128, mlp_mode="bf16")), ("parity mode", dict(fc_units=256, mlp_mode="bf16x3")),
                                     ("fine pass", dict(fc_units=256, mlp_mode="bf16", n_importance=64)),
                                     ("s-nerf", dict(fc_units=256, mlp_mode="bf16", model="s-nerf"))])
def test_sun_visibility_on_every_route_of_render_depth(what, kw):
    from satnerf_amd import data, rendering
    from satnerf_amd.models import load_model

    sc, rays, ts = _view()
    scene = _scene_args(sc)
    n, s, chunk = rays.shape[0], 64, 200
    args = O.default_args(n_samples=s, chunk=chunk, **kw)
    if what == "fine pass":
        models = _models(256)
    else:
        torch.manual_seed(9)
        models = {"coarse": load_model(args).to(DEV).eval()}
        if args.model == "sat-nerf":
            models["t"] = torch.nn.Embedding(args.t_embbeding_vocab, args.t_embbeding_tau).to(DEV)
    ts = ts if args.model == "sat-nerf" else None
    draws = _midpoint_draws(n, chunk, s, args.n_importance)
    got = rendering.render_sun_visibility(models, rays, ts, args, *scene)
    with rendering.replay_rng(draws):
        depth = rendering.render_depth(models, rays, ts, args)["depth"]
    srays = data.sun_rays(rays, depth, *scene, n_samples=s)
    with rendering.replay_rng(draws) as rng:
        want = rendering.render_depth(models, srays, ts, args, return_weights=True)["transparency"][:, -1]
    assert rng.i == len(draws) and got["typ"] == ("fine" if args.n_importance else "coarse")
    assert torch.equal(got["depth"], depth) and torch.equal(got["sun_geo"], want), what
    assert torch.equal(rendering.render_sun_visibility(models, rays, ts, args, *scene)["sun_geo"], got["sun_geo"])


# ---- against the CPU oracle ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_visibility(feat):
    """(visibility, primary transparency[:, -1]) of the CPU oracle in fp32 on cape_town(37, 53): fp64 restated sun rays from the
    oracle's own depth, its MLP, its compositing.  Nothing of satnerf_amd takes part."""
    sc = S.scene("cape_town", 37, 53, feat)
    rows, valid, _ = S.sun_rays_np(sc["rays"], sc["depth"], *_scene_args(sc), bias_rel=BIAS_REL)
    assert valid.all()
    vis = S.oracle_transparency(S.oracle_params(feat), rows.astype(np.float32), 64)[1][:, -1].numpy()
    return vis, sc["primary"]


@pytest.mark.parametrize("feat,mode", sorted(ORACLE_GATES))
def test_sun_visibility_against_the_cpu_oracle(feat, mode):
    from satnerf_amd import rendering
    from satnerf_amd.models import load_model

    sc = S.scene("cape_town", 37, 53, feat)
    want, want_primary = _oracle_visibility(feat)
    low, high = float((want < 0.2).mean()), float((want > 0.8).mean())
    assert low >= 0.10 and high >= 0.10, (low, high)  # the field casts shadows and leaves light: a flat field cannot pass
    args = O.default_args(n_samples=64, fc_units=feat, mlp_mode=mode, chunk=1024)
    model = load_model(args)
    model.load_state_dict(S.oracle_params(feat))
    models = {"coarse": model.to(DEV).eval(), "t": torch.nn.Embedding(args.t_embbeding_vocab, 4).to(DEV)}
    rays = _t(sc["rays"])
    ts = torch.zeros(rays.shape[0], dtype=torch.int64, device=DEV)
    got = rendering.render_sun_visibility(models, rays, ts, args, *_scene_args(sc))
    with rendering.replay_rng(_midpoint_draws(rays.shape[0], 1024, 64)):
        primary = rendering.render_depth(models, rays, ts, args, return_weights=True)
    assert bool(got["valid"].all()) and torch.equal(primary["depth"], got["depth"])
    err = float(np.abs(got["sun_geo"].cpu().numpy() - want).max())
    err_primary = float(np.abs(primary["transparency"][:, -1].cpu().numpy() - want_primary).max())
    err_depth = float(np.abs(got["depth"].cpu().numpy() - sc["depth"]).max())
    # context, not gated: the sun pass alone, started from the oracle's depths instead of the GPU's own
    given = rendering.render_sun_visibility(models, rays, ts, args, *_scene_args(sc), depth=_t(sc["depth"]))
    err_given = float(np.abs(given["sun_geo"].cpu().numpy() - want).max())
    print(f"width {feat} {mode}: sun pass {err:.3e}, primary pass {err_primary:.3e}, gate {ORACLE_GATES[(feat, mode)]:.3e}; "
          f"depth {err_depth:.3e}, sun pass from the oracle's depths {err_given:.3e}; oracle visibilities {100 * low:.0f} % below 0.2, {100 * high:.0f} % above 0.8")
    assert err <= ORACLE_GATES[(feat, mode)]


# ---- the shadows= keyword ---------------------------------------------------------------------------------------------------------------
def test_sun_interp_with_geometric_shadows():
    from satnerf_amd import evaluate, ops, rendering

    sc, rays, ts = _view(16, 16)
    center, scene_range, max_alt = _scene_args(sc)
    args = O.default_args(n_samples=64, fc_units=256, mlp_mode="bf16", chunk=100)
    models = {k: v for k, v in _models(256).items() if k != "fine"}
    upper, lower = S.sun_direction(70, 120), S.sun_direction(25, 140)
    sweep = (models, rays, ts, args, 16, 16, upper, lower, center, scene_range)

    def run(**kw):
        torch.manual_seed(3)
        return (evaluate.sun_interp_shadows if kw else evaluate.sun_interp)(*sweep, n_interp=3, **kw)

    base, head, geo = run(), run(shadows="head"), run(shadows="geometry", max_alt=max_alt)
    for res in (head, geo):
        assert res["angles"] == base["angles"] and res["order"] == base["order"] and (res["sun_dirs"] == base["sun_dirs"]).all()
        for k, strip in base["strips"].items():
            assert torch.equal(res["strips"][k], strip), k
        for a, b, x, y in zip(res["outputs"], base["outputs"], res["alts"], base["alts"]):
            assert torch.equal(x, y) and all(torch.equal(a[k], b[k]) if torch.is_tensor(b[k]) else a[k] == b[k] for k in b)
    assert set(head["strips"]) == set(base["strips"]) and all(set(o) == set(b) for o, b in zip(head["outputs"], base["outputs"]))
    assert set(geo["strips"]) == set(base["strips"]) | {"sun_geo", "rgb_geo"}
    assert geo["strips"]["sun_geo"].shape == base["strips"]["sun"].shape and geo["strips"]["sun_geo"].dtype == torch.uint8
    assert geo["strips"]["rgb_geo"].shape == base["strips"]["rgb"].shape and geo["strips"]["rgb_geo"].dtype == torch.uint8
    swept = rays.clone()
    seen = []
    for sun_d, out, b in zip(geo["sun_dirs"], geo["outputs"], base["outputs"]):
        assert set(out) == set(b) | {"sun_geo", "rgb_geo"} and out["sun_geo"].shape == (256, 1) and out["rgb_geo"].shape == (256, 3)
        swept[:, 8:11] = _t(sun_d.astype(np.float32))
        want = rendering.render_sun_visibility(models, swept, ts, args, center, scene_range, max_alt, sun_d=sun_d, depth=out["depth"])
        assert bool(want["valid"].all()) and torch.equal(out["sun_geo"][:, 0], want["sun_geo"])
        assert torch.equal(out["rgb_geo"], ops.sun_shade(out["albedo"], out["sky"], out["sun_geo"]))
        seen.append(out["sun_geo"])
    assert not torch.equal(seen[0], seen[2])  # the visibility follows the sun


def test_render_ortho_dsm_with_geometric_shadows():
    from satnerf_amd import data, dsm, ops, rendering

    sc = S.scene("cape_town", 16, 16)
    s = sc["s"]
    args = O.default_args(n_samples=64, fc_units=256, mlp_mode="bf16")
    models = {k: v for k, v in _models(256).items() if k != "fine"}
    common = (s["center"], s["scene_range"], s["min_alt"], s["max_alt"], s["sun_d"])

    def run(**kw):
        torch.manual_seed(0)
        return dsm.render_ortho_dsm(models, 3, args, *common, grid=s["grid"], zone=34, **kw)

    rays = data.ortho_rays(device=DEV, **s)
    ts = torch.full((256,), 3, dtype=torch.int64, device=DEV)
    for geometry_only in (True, False):
        plain, outputs0 = run(geometry_only=geometry_only)
        got, outputs = run(geometry_only=geometry_only, shadows="geometry")
        assert torch.equal(_bits(got.dsm), _bits(plain.dsm)) and torch.equal(got.weight, plain.weight)
        assert set(outputs) == set(outputs0) | ({"sun_geo"} if geometry_only else {"sun_geo", "rgb_geo"})
        assert not geometry_only or set(outputs) == {"depth", "acc", "sun_geo"}
        assert all(torch.equal(outputs[k], v) if torch.is_tensor(v) else outputs[k] == v for k, v in outputs0.items())
        want = rendering.render_sun_visibility(models, rays, ts, args, s["center"], s["scene_range"], s["max_alt"], sun_d=s["sun_d"],
                                               depth=outputs["depth"])["sun_geo"]
        assert outputs["sun_geo"].shape == (256,) and torch.equal(outputs["sun_geo"], want) and bool(torch.isfinite(want).all())
        if not geometry_only:
            assert torch.equal(outputs["rgb_geo"], ops.sun_shade(outputs["albedo"], outputs["sky"], outputs["sun_geo"]))


# ---- empty inputs ----------------------------------------------------------------------------------------------------------------------
def test_no_rays_give_empty_results():
    from satnerf_amd import data, ops, rendering

    sc = S.scene("cape_town", 16, 16)
    scene = _scene_args(sc)
    rays, ts, depth = torch.empty(0, 11, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV), torch.empty(0, device=DEV)
    r, valid, lla = ops.sun_rays(rays, depth, *scene, want_latlonalt=True)
    assert r.shape == (0, 11) and r.dtype == torch.float32 and valid.shape == (0,) and valid.dtype == torch.uint8
    assert lla.shape == (3, 0) and lla.dtype == torch.float64
    r, valid = data.sun_rays(rays, depth, *scene, sun_d=(0.3, 0.4, 0.8), bias=0.0, return_valid=True)
    assert r.shape == (0, 11) and valid.shape == (0,) and valid.dtype == torch.bool
    rgb = ops.sun_shade(torch.empty(0, 3, device=DEV), torch.empty(0, 3, device=DEV), depth)
    assert rgb.shape == (0, 3) and rgb.dtype == torch.float32
    models = {k: v for k, v in _models(256).items() if k != "fine"}
    for kw in (dict(), dict(depth=depth)):
        out = rendering.render_sun_visibility(models, rays, ts, O.default_args(mlp_mode="bf16"), *scene, **kw)
        assert out["typ"] == "coarse" and out["sun_geo"].shape == out["depth"].shape == out["valid"].shape == (0,)
        assert out["sun_geo"].dtype == torch.float32 and out["valid"].dtype == torch.bool
    torch.cuda.synchronize()
