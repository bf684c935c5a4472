"""tests/dx_reference.py pinned on the CPU: its float64 chain is autograd's gradient of every pre-activation, its operand model stays close
to it, and its MX8 restatement round-trips within the half step the GPU test uses as its quantisation bound."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import satnerf_oracle as O
from satnerf_amd import packing

from . import dx_reference as X

N = 40
CASES = [(256, 4), (256, 16), (512, 4)]


def forward_recorded(p, xyz, sun, t_emb):
    """oracle.satnerf_oracle.satnerf_mlp with every pre-activation kept: -> (outputs (albedo, sigma, sun_v, beta), {key: pre-activation})."""
    pre = {}
    h = xyz
    for i in range(8):
        if i == 4:
            h = torch.cat([xyz, h], -1)
        pre[f"a{i}"] = F.linear(h, p[f"fc_net.{2 * i}.weight"], p[f"fc_net.{2 * i}.bias"])
        h = torch.sin((30.0 if i == 0 else 1.0) * pre[f"a{i}"])
    pre["sigma"] = F.linear(h, p["sigma_from_xyz.0.weight"], p["sigma_from_xyz.0.bias"])
    pre["feats"] = F.linear(h, p["feats_from_xyz.weight"], p["feats_from_xyz.bias"])
    pre["rgbh"] = F.linear(pre["feats"], p["rgb_from_xyzdir.0.weight"], p["rgb_from_xyzdir.0.bias"])
    logits = F.linear(torch.sin(pre["rgbh"]), p["rgb_from_xyzdir.2.weight"], p["rgb_from_xyzdir.2.bias"])
    s = torch.cat([pre["feats"], sun], -1)
    for j, k in ((0, "s1"), (2, "s2"), (4, "s3")):
        pre[k] = F.linear(s, p[f"sun_v_net.{j}.weight"], p[f"sun_v_net.{j}.bias"])
        s = torch.sin(pre[k])
    sun_logit = F.linear(s, p["sun_v_net.6.weight"], p["sun_v_net.6.bias"])
    pre["e1"] = F.linear(torch.cat([pre["feats"], t_emb], -1), p["beta_from_xyz.0.weight"], p["beta_from_xyz.0.bias"])
    beta_pre = F.linear(torch.sin(pre["e1"]), p["beta_from_xyz.2.weight"], p["beta_from_xyz.2.bias"])
    pre["head"] = torch.cat([logits, sun_logit, beta_pre], 1)
    pre["dt"] = t_emb
    albedo = torch.sigmoid(pre["head"][:, 0:3]) * 1.002 - 0.001
    return (albedo, F.softplus(pre["sigma"][:, 0]), torch.sigmoid(pre["head"][:, 3]), F.softplus(pre["head"][:, 4])), pre


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"w{c[0]}-tau{c[1]}")
def case(request):
    feat, tau = request.param
    p = {k: v.double().requires_grad_(True) for k, v in O.procedural_satnerf_params(feat, tau, seed=11).items()}   # (every pre-activation in the graph)
    g = torch.Generator().manual_seed(feat + tau)
    xyz = torch.rand(N, 3, generator=g, dtype=torch.float64) * 2 - 1
    sun = F.normalize(torch.randn(N, 3, generator=g, dtype=torch.float64), dim=1)
    t_emb = (torch.rand(N, tau, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_(True)
    outs, pre = forward_recorded(p, xyz, sun, t_emb)
    want = O.satnerf_mlp(p, xyz, sun, t_emb.detach())
    for got, cols in zip(outs, (slice(0, 3), 3, 4, 8)):
        assert torch.allclose(got.detach(), want[:, cols], rtol=0, atol=1e-13)
    grads = (torch.randn(N, 3, generator=g, dtype=torch.float64), torch.randn(N, generator=g, dtype=torch.float64),
             torch.randn(N, generator=g, dtype=torch.float64), torch.randn(N, generator=g, dtype=torch.float64))
    # phases exactly as the forward would save them with unlimited resolution: frac(argument of the sine / 2 pi)
    phases = {k: torch.frac((30.0 if k == "a0" else 1.0) * v.detach() / (2 * math.pi)) for k, v in pre.items() if k not in ("sigma", "feats", "head", "dt")}
    return dict(feat=feat, tau=tau, p=p, outs=outs, pre=pre, grads=grads, phases=phases)


def autograd_dpre(c, grads):
    """d sum(g out) / d every pre-activation and d t_emb, keyed like the reference's vectors (fc_net.0's row divided by 30: the reference's
    ``pre0`` is with respect to the sine's argument)."""
    loss = sum((g * o).sum() for g, o in zip(grads, c["outs"]) if g is not None)
    keys = list(c["pre"])
    got = torch.autograd.grad(loss, [c["pre"][k] for k in keys], retain_graph=True, allow_unused=True)
    out = {}
    for k, v in zip(keys, got):
        v = torch.zeros_like(c["pre"][k]) if v is None else v
        out["pre" + k[1:] if k[0] == "a" else k] = v / 30.0 if k == "a0" else v
    return out


@pytest.mark.parametrize("drop", [None, 0, 1, 2, 3], ids=["all", "no_albedo", "no_sigma", "no_sun", "no_beta"])
def test_exact_chain_is_autograd(case, drop):
    c = case
    grads = tuple(None if i == drop else g for i, g in enumerate(c["grads"]))
    want = autograd_dpre(c, grads)
    got = X.chain(c["p"], c["phases"], [o.detach() for o in c["outs"]], grads, c["feat"], c["tau"], rounded=False)
    assert set(got) == set(want) == set(X.geometry(c["feat"], c["tau"])["dp"]) | {"dt"}
    for k in want:
        assert got[k].shape == want[k].shape, k
        for f in range(0, want[k].shape[1], 16):   # per fragment of 16 features
            a, b = got[k][:, f:f + 16], want[k][:, f:f + 16]
            assert float((a - b).abs().max()) <= 1e-10 * float(b.abs().max()), (k, f, float((a - b).abs().max()), float(b.abs().max()))
    if drop is not None:   # a missing gradient is a zero gradient: the rows it alone feeds are exactly zero
        dead = {0: ("rgbh",), 1: ("sigma",), 2: ("s1", "s2", "s3"), 3: ("e1", "dt")}[drop]
        assert all(float(got[k].abs().max()) == 0.0 for k in dead)


def test_one_stage_mode_rebuilds_the_chain(case):
    """Feeding every stage the chain's own (unrounded) output of the stage above gives the chain's output again, and A bounds |M|."""
    c = case
    outs = [o.detach() for o in c["outs"]]
    M = X.chain(c["p"], c["phases"], outs, c["grads"], c["feat"], c["tau"], rounded=False)
    wts = X.weights(c["p"], rounded=False)
    for st in X.steps(c["feat"], c["tau"]):
        m, a = X.stage(st, M, wts, c["phases"])
        assert torch.equal(m, M[st[1]]) and bool((m.abs() <= a * (1 + 1e-12)).all()), st[0]
    assert [s[0] for s in X.steps(c["feat"], c["tau"])][3:] == X.STAGES[1:] and X.STAGES[0] == "bH"


def test_rounded_chain_stays_near_the_exact_one(case):
    """The operand model (bf16 weights, bf16 hand-off) is not the exact chain, and is within 2^-6 of it in every column's 2-norm.

    The column norm of the difference is taken relative to the column norm of the stage's magnitude sum A = (|W|^T |d_in|) |cos|, the scale
    the rounding error of a dot product is proportional to -- not to the column norm of the result: the sun chain's gradient is rank one
    in the features (one head row times sun_v_net.6.weight), so single columns of d s2 / d s1 cancel to 1 / 200 of their neighbours and
    their relative error says nothing about the model.  Measured (40 points): <= 0.5 % of |A| in every column; relative to the result's
    own norm the median column is at 0.2 - 0.8 %, the cancelled columns of s2 / s1 at 17 - 105 %, single columns of feats / dt at 4 %."""
    c = case
    outs = [o.detach() for o in c["outs"]]
    exact, mag = X.chain(c["p"], c["phases"], outs, c["grads"], c["feat"], c["tau"], rounded=False, want_abs=True)
    rounded = X.chain(c["p"], c["phases"], outs, c["grads"], c["feat"], c["tau"], rounded=True)
    worst = 0.0
    for k in exact:
        d, n = (rounded[k] - exact[k]).norm(dim=0), mag[k].norm(dim=0)
        assert float(d.min()) > 0.0, k
        assert bool((d < 2.0 ** -6 * n).all()), (k, float((d / n).max()))
        worst = max(worst, float((d / n).max()))
    print(f"w{c['feat']} tau{c['tau']}: worst |rounded - exact| / |A| per column = {worst:.2e}")


def test_scaling_the_gradients_by_a_power_of_two_is_exact(case):
    """What the GPU test's linearity check rests on: every operation of the chain commutes with 2^k, in both evaluations."""
    c = case
    outs = [o.detach() for o in c["outs"]]
    g32 = tuple(g.float() * 1e-3 for g in c["grads"])
    for rounded in (False, True):
        base = X.chain(c["p"], c["phases"], outs, g32, c["feat"], c["tau"], rounded)
        for k in (-20, 20):
            scaled = X.chain(c["p"], c["phases"], outs, tuple(g * 2.0 ** k for g in g32), c["feat"], c["tau"], rounded)
            assert all(torch.equal(scaled[key], base[key] * 2.0 ** k) for key in base), (rounded, k)


def test_geometry_is_the_packers():
    for feat, tau in CASES:
        geo, bm, g8 = X.geometry(feat, tau), packing.backward_maps(feat, tau), packing.fmt8_geometry(feat)
        frags = lambda d: sorted(f0 + i for f0, n in d.values() for i in range(n // 16))  # noqa: E731
        assert frags(geo["dp"]) == sorted({f for r in bm["block_rows"] for f in r}) == list(range(g8["DP_HEAD"] + 1))
        assert set(frags(geo["act"])) | set(range(g8["ACT_FEATS"] + geo["auxs"], g8["ACT_FEATS"] + geo["auxs"] + g8["KS"])) \
            == {f for cols in bm["block_cols"] for f in cols}
        assert [geo["dp"][k][0] for k in ("feats", "sigma", "rgbh", "head")] == [g8[k] for k in ("DP_FEATS", "DP_SIGMA", "DP_RGBH", "DP_HEAD")]


def test_mx8_restatement_round_trips_within_the_half_step():
    g = torch.Generator().manual_seed(8)
    v = torch.randn(4096, 16, generator=g) * torch.exp2(torch.randint(-60, 20, (4096, 1), generator=g).float())
    v[0] = 0.0                                             # an all-zero lane: the clamp E = 6, code 128
    v[1] = torch.tensor([1.0] + [0.25] * 15)               # a power-of-two maximum
    v[2] = torch.tensor([127.0 / 64] + [-0.5] * 15)        # scaled maximum exactly 127
    v[3] = torch.tensor([-(2.0 - 2.0 ** -7)] + [0.1] * 15)   # max (1 + 2^-7) crosses the binade: E one up, scaled maximum 63.5
    v[4] = torch.tensor([127.5 / 64] + [0.0] * 15)         # between: 127.5 (1 + 2^-7) > 128: E one up again, not a saturated code
    e, u = X.mx8_encode(v)
    q = torch.exp2(e.double() - 134.0)
    err = (X.mx8_decode(e, u) - v.double()).abs()
    assert bool((err <= q[:, None]).all()), float((err / q[:, None]).max())
    assert int(e[0]) == 6 and bool((u[0] == 128).all())
    assert int(e[1]) == 127 and int(u[1, 0]) == 128 + 64 and int(e[2]) == 127 and int(u[2, 0]) == 255 and int(e[3]) == 128 and int(e[4]) == 128
    big = (u[1:] - 128).abs().amax(1)
    assert bool(((u[1:] >= 1) & (u[1:] <= 255)).all()) and int(big.min()) >= 63 and int(big.max()) <= 127
    assert bool((e[1:] > 6).all())
