"""tests/ray_reference.py checked on the CPU, before any kernel is held to it.

1. The formulas are the oracle's: in float64 ("exact" mode: nothing rounded) on smooth inputs every value equals
   oracle/satnerf_oracle.py's and every gradient torch.autograd's through the oracle's own functions, to 1e-12 of the output's largest
   magnitude.
2. A float32 evaluation of the same formulas (sequential cumprod / cumsum where the kernels scan across lanes) lies inside every gate on
   every input set the GPU module runs.  Worst |error| / gate over all cases, per output (this is a record, nothing is derived from it):
     render_loss      rgb 0.13   d_sigma 0.08   d_albedo 0.33   d_sun 0.33   g_beta 0.33   d_sky 0.11   loss 0.10
     composite        weights 0.41   transp 0.39   depth 0.06   rgb 0.16
     composite_bwd    d_sigma 0.19   d_albedo 0.99   d_sun 0.57   d_sky 0.18
                      (d_albedo = w * g_rgb without a sun head is ONE rounding of a product of data: the gate of one rounding is sharp)
     satnerf_loss     g_rgb 0.33   g_weights 0.14   g_beta 0.13   loss 0.07
     sc_loss          d_sun 0.52   loss 0.02
     depth_loss       g_depth 0.56   loss 0.06
     composite_image  0.08
3. Every planted fault (ray_reference.FAULTS) puts the emulation outside a gate by a factor of 4 or more on some element.
4. The input sets reach the edges the issue names, with no ray left out."""
import pytest
import torch

from oracle import satnerf_oracle as O

from . import ray_reference as R

ALL = [(kind, case) for kind, cases in R.CASES.items() for case in cases]
PIN = 1e-12


def _close(got, want, what):
    got, want = (got.v if isinstance(got, R.V) else got).detach().double(), want.detach().double()
    assert got.shape == want.shape, what
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert err <= PIN * max(float(want.abs().max()), 1.0), (what, err)


def _smooth(n, s, noise=True):
    inp = R.make_inputs(n, s, 5, noise=noise, smooth=True)
    return {k: (v.double() if torch.is_tensor(v) else v) for k, v in inp.items()}


def _oracle_render(inp, leaves, clamp=True):
    for t in leaves:
        inp[t].requires_grad_(True)
    noise = torch.zeros_like(inp["sigma"]) if inp["noise"] is None else inp["noise"] * inp["noise_std"]
    w, t = O.alpha_composite(inp["z"], inp["sigma"], noise)
    depth = torch.sum(w * inp["z"], -1)
    sun, sky = inp["sun_v"].unsqueeze(-1), inp["sky"].unsqueeze(1)
    c = torch.sum(w.unsqueeze(-1) * inp["albedo"] * (sun + (1 - sun) * sky), -2)      # models/satnerf.py:68-69, as satnerf_inference
    return w, t, depth, (torch.clamp(c, 0.0, 1.0) if clamp else c)


@pytest.mark.parametrize("s", [7, 64, 130])
@pytest.mark.parametrize("noise", [True, False])
def test_composite_is_the_oracle(s, noise):
    inp = _smooth(6, s, noise)
    a = [inp[k] for k in ("z", "sigma", "noise", "noise_std")]
    leaves = ("sigma", "albedo", "sun_v", "sky")
    w, t, depth, rgb = _oracle_render(inp, leaves)
    ref = R.composite(*a, inp["albedo"], inp["sun_v"], inp["sky"], mode="exact")
    for k, v in (("weights", w), ("transp", t), ("depth", depth), ("rgb", rgb)):
        _close(ref[k], v, k)
    g = torch.Generator().manual_seed(3)
    gs = [torch.randn(x.shape, generator=g, dtype=torch.float64) for x in (rgb, depth, w, t)]
    grads = torch.autograd.grad(sum((x * y).sum() for x, y in zip((rgb, depth, w, t), gs)), [inp[k] for k in leaves], retain_graph=True)
    got = R.composite_grads(*a, inp["albedo"], inp["sun_v"], inp["sky"], True, *gs, mode="exact")
    for k, v in zip(("d_sigma", "d_albedo", "d_sun", "d_sky"), grads):
        _close(got[k], v, k)
    # each arriving gradient alone, and the sigma-only / no-sun-head forms
    for i, name in enumerate(("g_rgb", "g_depth", "g_w", "g_T")):
        grads = torch.autograd.grad(((rgb, depth, w, t)[i] * gs[i]).sum(), [inp[k] for k in leaves], retain_graph=True, allow_unused=True)
        got = R.composite_grads(*a, inp["albedo"], inp["sun_v"], inp["sky"], True, **{name: gs[i]}, mode="exact")
        for k, v in zip(("d_sigma", "d_albedo", "d_sun", "d_sky"), grads):
            _close(got[k], torch.zeros_like(got[k].v) if v is None else v, (name, k))
    plain = torch.sum(w.unsqueeze(-1) * inp["albedo"], -2)
    grads = torch.autograd.grad((plain * gs[0]).sum(), [inp["sigma"], inp["albedo"]], retain_graph=True)
    got = R.composite_grads(*a, inp["albedo"], None, None, False, g_rgb=gs[0], mode="exact")
    _close(R.composite(*a, inp["albedo"], None, None, False, mode="exact")["rgb"], plain, "rgb without a sun head")
    _close(got["d_sigma"], grads[0], "d_sigma without a sun head")
    _close(got["d_albedo"], grads[1], "d_albedo without a sun head")
    got = R.composite_grads(*a, None, None, None, True, g_rgb=gs[0], g_w=gs[2], mode="exact")
    _close(got["d_sigma"], torch.autograd.grad((w * gs[2]).sum(), inp["sigma"])[0], "d_sigma, sigma only")


@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("s", [1, 7, 64])
def test_render_loss_is_the_oracle(s, warm):
    inp = _smooth(6, s)
    leaves = ("sigma", "albedo", "sun_v", "sky", "beta")
    w, _, _, rgb = _oracle_render(inp, leaves)
    res = {"weights_coarse": w, "beta_coarse": inp["beta"].unsqueeze(-1), "rgb_coarse": rgb}
    loss = O.snerf_loss(res, inp["target"], lambda_sc=0.0) if warm else O.satnerf_loss(res, inp["target"], beta_min=0.05)
    grads = torch.autograd.grad(loss, [inp[k] for k in leaves], allow_unused=True)
    got = R.render_loss(*[inp[k] for k in ("z", "sigma", "noise", "noise_std", "albedo", "sun_v", "beta", "sky", "target")], warm=warm, mode="exact")
    _close(got["loss"], loss, "loss")
    _close(got["rgb"], rgb, "rgb")
    for k, v in zip(("d_sigma", "d_albedo", "d_sun", "d_sky", "g_beta"), grads):
        _close(got[k], torch.zeros_like(got[k].v) if v is None else v, k)


@pytest.mark.parametrize("warm,grad_scale", [(False, 1.0), (False, 0.5), (True, 0.5)])
def test_satnerf_loss_is_the_oracle(warm, grad_scale):
    inp = _smooth(6, 70)
    w, _, _, rgb = _oracle_render(inp, ())
    w, rgb, beta = (t.detach().requires_grad_(True) for t in (w, rgb, inp["beta"]))
    res = {"weights_coarse": w, "beta_coarse": beta.unsqueeze(-1), "rgb_coarse": rgb}
    loss = O.snerf_loss(res, inp["target"], lambda_sc=0.0) if warm else O.satnerf_loss(res, inp["target"], beta_min=0.05)
    grads = torch.autograd.grad(loss * grad_scale, [rgb, w, beta], allow_unused=True)
    got = R.satnerf_loss(rgb, w, beta, inp["target"], grad_scale=grad_scale, warm=warm, mode="exact")
    _close(got["loss"], loss, "loss")          # the value is not scaled
    for k, v in zip(("g_rgb", "g_weights", "g_beta"), grads):
        _close(got[k], torch.zeros_like(got[k].v) if v is None else v, k)


def test_sc_depth_and_image_are_the_oracle():
    inp = _smooth(6, 70)
    a = [inp[k] for k in ("z", "sigma", "noise", "noise_std")]
    w, t, depth, rgb = _oracle_render(inp, ())
    sun = inp["sun_v"].clone().requires_grad_(True)
    loss = O.solar_correction_loss({"sun_sc_coarse": sun.unsqueeze(-1), "transparency_sc_coarse": t, "weights_sc_coarse": w}, 0.05)
    got = R.sc_loss(*a, inp["sun_v"], 0.05, mode="exact")
    _close(got["loss"], loss, "sc loss")
    _close(got["d_sun"], torch.autograd.grad(loss, sun)[0], "sc d_sun")

    g = torch.Generator().manual_seed(1)
    d = torch.rand(33, generator=g, dtype=torch.float64).requires_grad_(True)
    depths = torch.rand(33, 3, generator=g, dtype=torch.float64)
    for uw in (True, False):
        loss = O.depth_loss({"depth_coarse": d}, depths[:, 0], depths[:, 1] if uw else 1.0, lambda_ds=1000.0)
        got = R.depth_loss(d, depths, 1000.0, uw, mode="exact")
        _close(got["loss"], loss, "depth loss")
        _close(got["g_depth"], torch.autograd.grad(loss, d)[0], "g_depth")

    n, s = inp["z"].shape
    res = {"rgb_coarse": rgb, "depth_coarse": depth, "weights_coarse": w, "sun_coarse": inp["sun_v"].unsqueeze(-1), "albedo_coarse": inp["albedo"],
           "beta_coarse": inp["beta"].unsqueeze(-1), "sky_coarse": inp["sky"].unsqueeze(1).expand(n, s, 3)}
    want = O.image_outputs(res, "coarse")
    want = torch.cat([want[k].reshape(n, -1) for k in ("rgb", "depth", "acc", "sun", "albedo", "beta", "sky")], -1)
    _close(R.composite_image(*a, inp["albedo"], inp["sun_v"], inp["beta"], inp["sky"], mode="exact")["image"], want, "image")


def test_reference_leaves_its_inputs_alone():
    kind, case = "render_loss", R.CASES["render_loss"][0]
    inp = R.case_inputs(kind, case)
    before = {k: v.clone() for k, v in inp.items() if torch.is_tensor(v)}
    R.compare(kind, case, R.emulate(kind, case))
    assert all(torch.equal(v, inp[k]) for k, v in before.items())


@pytest.mark.parametrize("kind,case", ALL, ids=[f"{k}-{R.case_id(c)}" for k, c in ALL])
def test_float32_emulation_is_inside_every_gate(kind, case):
    res = R.compare(kind, case, R.emulate(kind, case))
    print(kind, R.case_id(case), {k: round(v, 3) for k, v in res.items()})
    assert res and all(v <= 1.0 for v in res.values()), res


def _case(kind, **want):
    hits = [c for c in R.CASES[kind] if all(c[k] == v for k, v in want.items())]
    assert hits, (kind, want)
    return kind, hits[0]


_C64, _C128 = _case("composite", s=64, variant="full"), _case("composite", s=128, variant="full")
_RL = _case("render_loss", n=37, s=64, noise=True, warm=False)
PLANTED = {   # fault -> the cases it is planted in and the outputs one of which must leave its gate
    "last_delta": [(_C64, ("weights", "depth"))],
    "no_floor": [(_C64, ("transp",)), (_RL, ("d_sigma",))],
    "inclusive_T": [(_C64, ("transp",)), (_RL, ("rgb",))],
    "suffix_incl": [(_C64, ("d_sigma",)), (_RL, ("d_sigma",))],
    "carry_fwd": [(_C128, ("transp",))],
    "carry_rev": [(_C128, ("d_sigma",))],
    "gate_sigma": [(_case("composite", s=64, variant="noise"), ("d_sigma",)), (_RL, ("d_sigma",))],
    "no_clamp_gate": [(_C64, ("d_albedo",)), (_RL, ("d_albedo",))],
    "no_1m_sun": [(_C64, ("d_sky",)), (_RL, ("d_sky",))],
    "no_1m_sky": [(_C64, ("d_sun",)), (_RL, ("d_sun",))],
    "db_missing": [(_RL, ("g_beta",))],
    "db_sign": [(_RL, ("g_beta",))],
    "warm_log": [(_case("render_loss", n=37, s=64, noise=True, warm=True), ("loss",))],
    "mean_3n": [(_RL, ("d_albedo",)), (_case("satnerf_loss", grad_scale=0.5, warm=False), ("g_rgb",))],
    "depth_no_w": [(_case("depth_loss", n=257, stride=3, use_weights=True), ("g_depth",))],
    "sc_no_w": [(_case("sc_loss", s=64, noise=True), ("d_sun",))],
}


def test_every_fault_is_planted():
    assert set(PLANTED) == set(R.FAULTS)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_fault_leaves_its_gate(fault):
    for (kind, case), outputs in PLANTED[fault]:
        res = R.compare(kind, case, R.emulate(kind, case, fault))
        print(fault, kind, R.case_id(case), {k: round(res[k], 1) for k in outputs})
        assert max(res[k] for k in outputs) >= 4.0, (fault, kind, case, res)


def test_carry_faults_act_behind_a_segment_boundary():
    """The two carry faults must be seen where the carry is used: at samples >= 64 (forward) and < 64 (reverse) of S = 128."""
    kind, case = _C128
    ref_ok = R.emulate(kind, case)
    fwd, rev = R.emulate(kind, case, "carry_fwd"), R.emulate(kind, case, "carry_rev")
    assert torch.equal(fwd["transp"][:, :64], ref_ok["transp"][:, :64]) and not torch.equal(fwd["transp"][:, 64:], ref_ok["transp"][:, 64:])
    assert torch.equal(rev["d_sigma"][:, 64:], ref_ok["d_sigma"][:, 64:]) and not torch.equal(rev["d_sigma"][:, :64], ref_ok["d_sigma"][:, :64])


COVERED = [(k, c) for k, c in ALL if k in ("render_loss", "composite", "sc_loss", "composite_image", "satnerf_loss")]


@pytest.mark.parametrize("kind,case", COVERED, ids=[f"{k}-{R.case_id(c)}" for k, c in COVERED])
def test_inputs_reach_the_edges(kind, case):
    """Shares and special rays on every set large enough to hold them (n >= 9 rays of >= 50 samples); on the small shapes -- (5, 7),
    (1, 2), (3, 1), S = 1 -- what must hold everywhere: nothing undecidable, so no ray is left out anywhere."""
    inp = dict(R.case_inputs(kind, case))
    if inp["albedo"] is None or inp["sun_v"] is None:      # the coverage is a property of the rays; variants only drop inputs
        inp.update(R.case_inputs(kind, dict(case, variant="full", noise=False)))
    cov = R.coverage(inp)
    print(kind, R.case_id(case), cov)
    assert cov["undecided_clamp"] == 0 and cov["undecided_f"] == 0
    if case["n"] >= 9 and case["s"] >= 50:
        assert cov["saturated"] >= 0.10 and cov["dens_le_0"] >= 0.20 and cov["tiny_x"] >= 0.10
        assert cov["all_off_rays"] >= 1 and cov["opaque_first_rays"] >= 1 and cov["clamped_rays"] >= 3
        out = R.composite(*[inp[k] for k in ("z", "sigma", "noise", "noise_std")])
        assert float(out["weights"].v.detach()[0].abs().max()) == 0.0            # the all-off ray: weights zero, beta_r = beta_min
        if case["s"] > 64:   # some ray is still alive (transmittance a normal float32) behind every segment boundary
            assert all(int((out["transp"].v.detach()[1:, b] > 2.0 ** -100).sum()) >= 1 for b in range(64, case["s"], 64))
