"""tests/fwd_reference.py pinned on the CPU.

a. Its exact chain is the model: every nn.Linear of models.load_model(args).double() (forward hooks) and the four outputs, and
   oracle.satnerf_oracle.satnerf_mlp, to 1e-10.
b. A CPU simulation of the kernel -- the operand model with float32 accumulation (one rounding per MFMA k-step) and a float32 sine,
   pushed through the restated encoders into the decoded form tests/test_hip_fwd_reference.py reads from an acts workspace -- passes every gate of that test on its shapes, and
   planted faults fail them, each at the stage where it is planted and not earlier.  The worst ratio of every stage is printed.
c. The encoders' restatements at their edges."""
import math
import types

import pytest
import torch
import torch.nn as nn

from oracle import satnerf_oracle as O
from satnerf_amd import models, packing

from . import dx_reference as X
from . import fwd_reference as F

SHAPES = {256: [(1, 64), (3, 40), (5, 64), (41, 64)], 512: [(1, 64), (3, 40), (3, 64), (9, 64)]}
MATRIX = {256: [("bf16", 8), ("f16", 8), ("bf16", 16), ("f16", 16), ("bf16x3", 16)], 512: [("bf16", 8), ("f16", 8)]}


def inputs(n_rays, s, tau, snerf=False):
    """The per-point inputs of the GPU test's driver, made on the CPU (stratified depths from the oracle)."""
    rays, ts = O.synthetic_rays(n_rays, seed=9 + n_rays)
    u = torch.rand(n_rays, s, generator=torch.Generator().manual_seed(n_rays * s))
    z = O.stratified_depths(rays, s, u)
    if snerf:
        temb, ts = torch.zeros(1, tau), torch.zeros_like(ts)
    else:
        temb = O.procedural_uniform((30, tau), 1.0, 22)
    return F.points(rays[:, 0:3], rays[:, 3:6], z, rays[:, 8:11], temb, ts, s)


# ---------------------------------------------------------------------------------------------------------------- a
def model_recorded(m, xyz, sun, t):
    """models/satnerf.py:156-208 walked over the model's own modules (their forward is the fused kernel's: satnerf_amd modules hold
    parameters only), a forward hook on every nn.Linear -> ({state_dict prefix: its output}, (albedo, sigma, sun_v, beta))."""
    rec, hooks = {}, []
    for name, mod in m.named_modules():
        if isinstance(mod, nn.Linear):
            hooks.append(mod.register_forward_hook(lambda mod, i, o, name=name: rec.__setitem__(name, o.detach())))

    def run(seq, x, first=0):
        for i, mod in enumerate(seq):
            if i < first:
                continue
            x = torch.sin(mod.w0 * x) if isinstance(mod, models.Siren) else mod(x)
        return x

    h = xyz
    for i in range(8):
        if i == 4:
            h = torch.cat([xyz, h], -1)
        h = torch.sin(m.fc_net[2 * i + 1].w0 * m.fc_net[2 * i](h))
    sigma = run(m.sigma_from_xyz, h)[:, 0]
    feats = m.feats_from_xyz(h)
    albedo = run(m.rgb_from_xyzdir, feats) * (1 + 2 * m.rgb_padding) - m.rgb_padding
    sun_v = run(m.sun_v_net, torch.cat([feats, sun], -1))[:, 0]
    beta = run(m.beta_from_xyz, torch.cat([feats, t], -1))[:, 0]
    for hk in hooks:
        hk.remove()
    return rec, dict(albedo=albedo.detach(), sigma=sigma.detach(), sun_v=sun_v.detach(), beta=beta.detach())


@pytest.mark.parametrize("feat,tau,snerf", [(256, 4, False), (256, 16, False), (512, 4, False), (512, 16, False), (256, 4, True)],
                         ids=["w256-tau4", "w256-tau16", "w512-tau4", "w512-tau16", "s-nerf"])
def test_exact_chain_is_the_model(feat, tau, snerf):
    args = O.default_args(model="s-nerf" if snerf else "sat-nerf", t_embbeding_tau=tau, fc_units=feat)
    m = models.load_model(args)
    m.load_state_dict(O.procedural_snerf_params(feat, seed=21) if snerf else O.procedural_satnerf_params(feat, tau, seed=21))
    for p in m.parameters():      # (m.double() would fold the parameters back into the model's flat fp32 buffer: convert the views themselves)
        p.data = p.data.double()
    sd = {k: p.detach() for k, p in m.named_parameters()}
    assert all(p.dtype == torch.float64 for p in sd.values())
    pts = inputs(3, 40, tau, snerf)
    rec, outs = model_recorded(m, pts.xyz, pts.sun, pts.t)
    got = F.chain(sd, pts, feat, tau)
    linear = {s[0]: s[2] for s in F.steps(feat, tau)}
    linear["a0"] = "fc_net.0"
    assert set(linear.values()) == set(rec) - {"sky_color.0", "sky_color.2"} == set(F.LAYERS)
    head = {"h_rgb": slice(0, 3), "h_sun": slice(3, 4), "h_beta": slice(4, 5)}
    for key, name in linear.items():
        scale = 30.0 / F.TWO_PI if key == "a0" else 1.0 / F.TWO_PI if name in F.SIN_LAYERS else 1.0
        mine = got["head"][:, head[key]] if key in head else got[key]
        want = rec[name] * scale
        assert mine.shape == want.shape, key
        assert float((mine - want).abs().max()) <= 1e-10, (key, float((mine - want).abs().max()))
    for key in F.OUTPUTS:
        assert float((got[key] - outs[key]).abs().max()) <= 1e-10, key
    o = O.satnerf_mlp(sd, pts.xyz, pts.sun, pts.t)       # (the zero uncertainty head of s-nerf included: beta = softplus(0))
    for key, cols in zip(F.OUTPUTS, (slice(0, 3), 3, 4, 8)):
        assert float((got[key] - o[:, cols]).abs().max()) <= 1e-10, key
    aux = got["aux"]
    assert aux.shape[1] == 16 * ((8 + (tau + 7) // 8 * 8 + 15) // 16)
    assert torch.equal(aux[:, 0:3], pts.sun) and bool((aux[:, 3] == 1).all()) and torch.equal(aux[:, 4:7], pts.xyz)
    assert bool((aux[:, 7] == 0).all()) and torch.equal(aux[:, 8:8 + tau], pts.t) and float(aux[:, 8 + tau:].abs().sum()) == 0.0


def test_one_stage_mode_rebuilds_the_rounded_chain():
    """Fed the rounded chain's own hand-offs as zero-width intervals, every stage gives the chain's value again, and A bounds |M|."""
    feat, tau, mode = 256, 16, "bf16"
    sd = O.procedural_satnerf_params(feat, tau, seed=21)
    pts = inputs(3, 40, tau)
    M = F.chain(sd, pts, feat, tau, mode)
    ops, R = F.operands(sd, mode), F.rounder(mode)
    aux = {"xyz": R(pts.xyz), "sun": R(pts.sun), "t": R(pts.t)}
    head = {"h_rgb": slice(0, 3), "h_sun": slice(3, 4), "h_beta": slice(4, 5)}
    for st in F.steps(feat, tau):
        src = M[st[3]]
        x = R(src) if st[3] == "feats" else R(F.sin_rev(src))
        m, a, amb = F.stage(st, ops, x, x, aux)
        want = M["head"][:, head[st[0]]] if st[0] in head else M[st[0]]
        assert float((m - want).abs().max()) <= 1e-12 and bool((m.abs() <= a * (1 + 1e-12)).all()) and float(amb.abs().max()) == 0.0, st[0]


# ---------------------------------------------------------------------------------------------------------------- b
def sin32(acc):
    f = acc - torch.floor(acc)
    return torch.sin(f * torch.tensor(F.TWO_PI, dtype=torch.float32))


def mma32(acc, x, w):
    """acc + x w^T as the matrix pipe accumulates it: one fp32 rounding per k-step of 16 products (the products of two 16-bit operands
    and their 16-term sum are exact in float64), which is what the gates' k_steps 2^-24 A stands for."""
    for k in range(0, x.shape[1], 16):
        acc = (acc.to(torch.float64) + x[:, k:k + 16].to(torch.float64) @ w[:, k:k + 16].to(torch.float64).T).float()
    return acc


def simulate(sd, pts, feat, tau, mode, fmt, truncate8=False, mx_bump=0, no_c=(), flip=None):
    """The kernel as the operand model describes it, in float32: -> (decoded workspace as fwd_reference.decode gives it, the four outputs).
    Planted faults: ``truncate8`` (a PHASE8 encoder that truncates), ``mx_bump`` (added to every MX8 exponent), ``no_c`` (layers packed
    without c), ``flip`` = (layer, row, column): the sign bit of that packed weight; a changed ``sd`` gives the rest."""
    ops = F.operands(sd, mode, no_c=no_c)
    if flip is not None:
        ops[flip[0]][0][flip[1], flip[2]] *= -1.0
    R = F.rounder(mode)
    r32 = lambda v: R(v.to(torch.float64)).float()  # noqa: E731
    aux = {"xyz": r32(pts.xyz), "sun": r32(pts.sun), "t": r32(pts.t)}
    w0, b0 = ops["fc_net.0"]
    acc = {"a0": pts.xyz.float() @ w0.float().T + b0.float()}
    hand = {"a0": r32(sin32(acc["a0"]))}
    for key, kind, name, src, cols, auxs, _ in F.steps(feat, tau):
        w, b = ops[name][0].float(), ops[name][1].float()
        v = mma32(torch.zeros(hand[src].shape[0], w.shape[0]), hand[src], w[:, cols])
        rest = [b[None, :].expand(v.shape[0], -1)] + [aux[a] @ w[:, acols].T for a, acols in auxs]      # the aux k-step(s): exact products, one rounding
        acc[key] = (v.to(torch.float64) + sum(r.to(torch.float64) for r in rest)).float()
        if kind != F.LIN:
            hand[key] = r32(sin32(acc[key])) if kind == F.SIN else r32(acc[key])
    got = types.SimpleNamespace(fmt=fmt, n=pts.xyz.shape[0], rev={}, code={}, lanes=None, feats_q=None)
    for key in F.CHAIN:
        if key == "feats":
            continue
        got.code[key] = F.phase8(acc[key], truncate8) if fmt == 8 else F.unorm16(acc[key])
        got.rev[key] = got.code[key].to(torch.float64) / (256.0 if fmt == 8 else 65535.0)
    if fmt == 8:
        lan = F.to_lanes(acc["feats"])
        e, u = X.mx8_encode(lan)
        if mx_bump:
            e = e + mx_bump
            u = (torch.round(lan.to(torch.float64) * torch.exp2(133.0 - e.to(torch.float64))[..., None]).to(torch.int32) + 128) & 0xff
        got.lanes = (u, e)
        got.feats = F.from_lanes(X.mx8_decode(e, u))
        got.feats_q = F.from_lanes(torch.exp2(e.to(torch.float64) - 134.0)[..., None].expand(lan.shape).contiguous())
    else:
        got.feats = acc["feats"].to(torch.bfloat16).to(torch.float64)
    got.aux = F.aux_vector(pts, tau).float().to(torch.bfloat16).to(torch.float64)
    head = torch.cat([acc["h_rgb"], acc["h_sun"], acc["h_beta"]], 1)
    o = F.activations(acc["sigma_pre"], head)
    return got, tuple(o[k] for k in F.OUTPUTS)


def gates(sd, pts, feat, tau, mode, fmt, got, outs):
    """Every gate of tests/test_hip_fwd_reference.py on a decoded workspace -> (W ratios or None, S ratios or None, lane problems)."""
    n = got.n
    w = s = None
    if mode != "bf16x3":
        w = F.gate_w(got, outs, F.chain(sd, pts, feat, tau, mode), F.chain(sd, pts, feat, tau), n)
    if fmt == 16:
        s = F.gate_s(got, outs, sd, pts, feat, tau, mode, n)
    return w, s, F.gate_lanes(got, n) if fmt == 8 else []


def show(label, w, s):
    if w is not None:
        print(f"{label} (W): " + " ".join(f"{k} {r:.2f}" for k, r in w))
    if s is not None:
        print(f"{label} (S): " + " ".join(f"{k} {r:.2f}" for k, r, _ in s))


_SD = {}


def params(feat, tau):
    if (feat, tau) not in _SD:
        _SD[feat, tau] = O.procedural_satnerf_params(feat, tau, seed=21)
    return _SD[feat, tau]


@pytest.mark.parametrize("feat,tau,mode,fmt", [(f, t, m, k) for f in (256, 512) for t in (4, 16) for m, k in MATRIX[f]])
def test_the_clean_simulation_passes_every_gate(feat, tau, mode, fmt):
    sd = params(feat, tau)
    for n_rays, s in SHAPES[feat]:
        pts = inputs(n_rays, s, tau)
        got, outs = simulate(sd, pts, feat, tau, mode, fmt)
        w, sg, lanes = gates(sd, pts, feat, tau, mode, fmt, got, outs)
        show(f"clean w{feat} tau{tau} {mode} fmt{fmt} {n_rays}x{s}", w, sg)
        assert not lanes, lanes
        if w is not None:
            assert all(r <= 1.0 for k, r in w if k in F.CHAIN), w
            if F.OUTPUTS_IN_W:      # the rule that lets the outputs join (W) with q = 0
                assert all(r <= 0.5 for k, r in w if k in F.OUTPUTS), [x for x in w if x[0] in F.OUTPUTS]
        if sg is not None:
            assert all(bad == 0 for _, _, bad in sg), [x for x in sg if x[2]]
        # the stored aux fragments are the bf16 rounding of the aux vector in every mode
        assert torch.equal(got.aux, F.aux_vector(pts, tau).float().to(torch.bfloat16).to(torch.float64))


def with_(sd, **changes):
    out = dict(sd)
    out.update(changes)
    return out


def faults(sd, feat):
    """name -> (changed state_dict, simulate arguments, the stage where it is planted)."""
    w8 = sd["fc_net.8.weight"]
    r, c = divmod(int(w8[:, 3:].abs().argmax()), feat)
    wrong = w8.clone()
    wrong[:, 0:3] = sd["fc_net.6.weight"][:, 0:3]
    return {"missing bias in fc_net.10": (with_(sd, **{"fc_net.10.bias": torch.zeros_like(sd["fc_net.10.bias"])}), {}, "a5"),
            "skip layer's xyz columns from fc_net.6": (with_(sd, **{"fc_net.8.weight": wrong}), {}, "a4"),
            "c omitted on sun_v_net.2": (sd, {"no_c": ("sun_v_net.2",)}, "s2"),
            "sign bit of one weight of fc_net.8": (sd, {"flip": ("fc_net.8", r, 3 + c)}, "a4")}


@pytest.mark.parametrize("feat,mode,fmt,n_rays,s", [(256, "bf16", 8, 5, 64), (256, "f16", 8, 3, 40), (256, "bf16", 16, 5, 64), (256, "f16", 16, 3, 40),
                                                    (256, "bf16x3", 16, 5, 64), (512, "bf16", 8, 3, 64)])
def test_planted_faults_fail_at_their_own_stage(feat, mode, fmt, n_rays, s):
    tau = 4
    sd = params(feat, tau)
    pts = inputs(n_rays, s, tau)
    order = F.CHAIN + F.OUTPUTS
    for name, (sd_bad, kw, where) in faults(sd, feat).items():
        got, outs = simulate(sd_bad, pts, feat, tau, mode, fmt, **kw)
        w, sg, lanes = gates(sd, pts, feat, tau, mode, fmt, got, outs)      # the reference keeps the true weights
        show(f"{name}, w{feat} {mode} fmt{fmt}", w, sg)
        assert not lanes
        if w is not None:
            assert F.first_failure(w) == where, (name, w)
        if sg is not None:     # (S) restarts from the decoded stage above: the planted stage fails, and no stage before it
            failed = [k for k, _, bad in sg if bad]
            assert failed and failed[0] == where, (name, sg)
            assert all(order.index(k) >= order.index(where) for k in failed)
            if where in ("a4", "a5"):
                assert failed == [where], (name, sg)      # a trunk layer feeds nothing but the next stage's decoded input
    if fmt == 8:
        got, outs = simulate(sd, pts, feat, tau, mode, fmt, truncate8=True)
        w, _, lanes = gates(sd, pts, feat, tau, mode, fmt, got, outs)
        show(f"truncating PHASE8 encoder, w{feat} {mode}", w, None)
        # rms of a truncation error 1 / (256 sqrt 3) against the half step 1 / 512: 1.15 where the rounding-noise term is small, that is,
        # in the early layers only -- the exact-integer encoder check of the GPU test is what holds the deep layers
        assert F.first_failure(w) == "a0" and not lanes, w
        got, outs = simulate(sd, pts, feat, tau, mode, fmt, mx_bump=1)
        w, _, lanes = gates(sd, pts, feat, tau, mode, fmt, got, outs)
        show(f"MX8 exponent one too large, w{feat} {mode}", w, None)
        # (the value still decodes within its -- doubled -- half step: (W) cannot see it; the lane check does, at feats)
        assert lanes and lanes[0][0].startswith("max |u - 128|"), (lanes, w)
        assert all(r <= 1.0 for k, r in w[:F.CHAIN.index("feats")])


# ---------------------------------------------------------------------------------------------------------------- c
def test_phase8_restatement_is_the_magic_add():
    """codec8.h: the low mantissa byte of x + 49152.0f, computed here in float32 as the kernel does, against the restatement."""
    g = torch.Generator().manual_seed(5)
    x = torch.cat([(torch.rand(4096, generator=g) * 2 - 1) * 70.0, torch.arange(-1024, 1024).float() / 512.0,    # every tie (k + 1/2) / 256
                   torch.tensor([0.0, -0.0, 255.5 / 256, 255.75 / 256, -1 / 1024, 16.0, -16.0, 63.998046875, -64.0])])
    low = (x + 49152.0).view(torch.int32) & 0xff
    assert torch.equal(low.to(torch.int64), F.phase8(x))
    assert F.phase8(torch.tensor([0.5 / 256, 1.5 / 256, 2.5 / 256, 255.5 / 256, -0.5 / 256])).tolist() == [0, 2, 2, 0, 0]
    assert F.phase8(torch.tensor([1.5 / 256, 255.9 / 256]), truncate=True).tolist() == [1, 255]


def test_unorm16_restatement():
    x = torch.tensor([0.0, -0.0, 1.0, 0.5, 0.25, -0.25, 1 - 2.0 ** -24, -2.0 ** -30, 3.75, 2.0 ** -17, 2.0 ** -16, 16.125])
    want = [0, 0, 0, 32768, 16384, 49151, 65535, 65535, 49151, 0, 1, 8192]
    # (0.5 -> 32767.5 -> 32768 and 0.25 -> 16383.75 -> 16384: RNE; 0.75 -> 49151.25 -> 49151)
    assert F.unorm16(x).tolist() == want
    d = F.wrap(F.unorm16(x).to(torch.float64) / 65535.0 - x.to(torch.float64)).abs()
    assert float(d.max()) <= F.Q16 + 1e-12


def test_lane_arrangement_round_trips_and_matches_the_decoder():
    nat = torch.arange(3 * 512, dtype=torch.float64).view(3, 512)
    assert torch.equal(F.from_lanes(F.to_lanes(nat)), nat)
    lan = F.to_lanes(nat[:, :256])
    assert lan.shape == (3, 8, 2, 16)
    # lane (tile t, half h) holds slots 8 h .. 8 h + 7 of logical fragments 2 t and 2 t + 1 (dx_reference.lanes)
    s2f = packing.slot_to_feat(torch.arange(256).numpy())
    assert lan[0, 1, 1].tolist() == [float(s2f[32 + 8 + j]) for j in range(8)] + [float(s2f[48 + 8 + j]) for j in range(8)]


@pytest.mark.parametrize("mode", ["bf16", "f16", "bf16x3"])
def test_bias_patterns_land_on_the_cases_they_are_for(mode):
    """(E) of the GPU test: the pattern is inverted from the target codes; this is where it is checked to land there."""
    for layer, n in (("fc_net.0", 256), ("fc_net.8", 256), ("sun_v_net.2", 128), ("fc_net.14", 512)):
        b, landed, k = F.bias_pattern(layer, n, mode)
        assert b.shape == landed.shape == (n,) and b.dtype == torch.float32 and k >= 20
        c = F.pattern_classes(landed, b)
        print(layer, mode, k, c)
        assert c["codes"] == {0, 1, 127, 128, 255} and c["wraps"] and c["negative"], c
        assert (c["tie_even"] and c["tie_odd"]) or mode == "bf16x3", c      # (PHASE8's ties: the 8-bit format belongs to bf16 / f16)
        assert c["plus_zero"] and c["minus_zero"] and 16.0 <= c["biggest"] <= (64.0 if layer == "fc_net.0" else 16.0), c
        if layer == "fc_net.0":
            assert c["biggest"] == 64.0
    b, landed, _ = F.bias_pattern("feats_from_xyz", 256, mode)
    e, u = X.mx8_encode(F.to_lanes(landed[None].float())[0])
    assert int(e[0, 1]) == 6 and bool((u[0, 1] == 128).all())                       # the zero lane
    assert int(u[0, 0, 0]) == 128 + 64 and bool((u[0, 0, 1:] == 128).all())         # one large, fifteen tiny (they round to code 128)
    assert int(e[1, 0]) == 128 and int(u[1, 1, 0]) == 255 and int(e[1, 1]) == 127   # the crossing maximum, the scaled maximum 127


# ---------------------------------------------------------------------------------------------------------------- what the gates' choices rest on
def test_the_issues_literal_bounds_of_gate_s_fail_an_exact_simulation():
    """Gate (S) departs from two literal figures: 2^-9 |M| for bf16 feats, and q = 1 / 131070 without v_fract's rounding.  The clean
    simulation -- exact RNE, arithmetic within the gate's own terms -- misses both and meets the gate as it stands."""
    feat, tau, mode, fmt = 256, 4, "bf16", 16
    sd = params(feat, tau)
    pts = inputs(41, 64, tau)
    got, outs = simulate(sd, pts, feat, tau, mode, fmt)
    lit = {k: (r, bad) for k, r, bad in F.gate_s(got, outs, sd, pts, feat, tau, mode, got.n, literal=True)}
    now = {k: (r, bad) for k, r, bad in F.gate_s(got, outs, sd, pts, feat, tau, mode, got.n)}
    print(f"literal bounds: feats {lit['feats'][0]:.3f} ({lit['feats'][1]} elements over), s1 {lit['s1'][0]:.6f} ({lit['s1'][1]} over)")
    assert lit["feats"][0] > 1.5 and lit["feats"][1] > 0          # half a bf16 ulp reaches 2^-8 |M|
    assert 1.0 < lit["s1"][0] < 1.001 and lit["s1"][1] >= 1       # v_fract of a small negative value: up to 2^-25 more
    assert all(bad == 0 for _, bad in now.values())


def test_the_outputs_stay_out_of_gate_w():
    """The rule: the four outputs join (W) with q = 0 only if the simulation's worst output ratio is <= 0.5.  It is above it."""
    feat, tau = 256, 4
    sd = params(feat, tau)
    worst = 0.0
    for n_rays, s in SHAPES[feat]:
        pts = inputs(n_rays, s, tau)
        got, outs = simulate(sd, pts, feat, tau, "bf16", 8)
        w, _, _ = gates(sd, pts, feat, tau, "bf16", 8, got, outs)
        worst = max([worst] + [r for k, r in w if k in F.OUTPUTS])
    print(f"worst simulated output ratio of (W) with q = 0: {worst:.3f}")
    assert (worst <= 0.5) == F.OUTPUTS_IN_W and worst > 0.5


def test_gate_w_does_not_hold_downstream_of_a_constant_stage():
    """(E) of the GPU test zeroes one stage's weight: downstream every point holds the same pre-activation, a hand-off whose bf16 rounding
    the fp32 sine flips is flipped for all points at once, and a column's error no longer averages.  With the 16-bit half step the exact
    simulation then exceeds (W) downstream of the swept stage -- and nowhere else --, while the per-element gate (S) holds everywhere:
    that is why the GPU test asserts (S) there."""
    feat, tau, mode, fmt = 256, 4, "bf16", 16
    base = params(feat, tau)
    pts = inputs(3, 40, tau)
    layer, key = "feats_from_xyz", "feats"
    b, _, _ = F.bias_pattern(layer, feat, mode)
    sd = with_(base, **{layer + ".weight": torch.zeros_like(base[layer + ".weight"]), layer + ".bias": b})
    got, outs = simulate(sd, pts, feat, tau, mode, fmt)
    w = F.gate_w(got, outs, F.chain(sd, pts, feat, tau, mode), F.chain(sd, pts, feat, tau), got.n)
    over = [(k, round(r, 3)) for k, r in w if k in F.CHAIN and r > 1.0]
    print(f"swept {layer}, {mode} fmt{fmt}: (W) over 1 at {over}")
    assert over and all(k in F.downstream(key) for k, _ in over), w
    assert all(bad == 0 for _, _, bad in F.gate_s(got, outs, sd, pts, feat, tau, mode, got.n))
    assert F.downstream("a6") == ["a7", "feats", "rgbh", "s1", "e1", "s2", "s3"] and F.downstream("s1") == ["s2", "s3"] and F.downstream("e1") == []


@pytest.mark.parametrize("feat,tau", [(256, 4), (256, 16), (512, 4), (512, 16)])
def test_aux_columns_alone_rarely_straddle_a_code_boundary(feat, tau):
    """(E), second variant: the share of elements whose sum +- its fp32 bound straddles a code boundary stays under 5 %, and the
    simulation's codes are the encoder of the sum everywhere else."""
    sd = params(feat, tau)
    pts = inputs(3, 40, tau)
    for mode, fmt in MATRIX[feat]:
        for layer, hid in F.AUX_STAGES.items():
            w = sd[layer + ".weight"].clone()
            w[:, hid if hid is not None else slice(0, feat)] = 0.0
            sd2 = with_(sd, **{layer + ".weight": w})
            step = next(x for x in F.steps(feat, tau) if x[2] == layer)
            _, lo, mid, hi = F.aux_only(step, sd2, pts, feat, tau, mode, fmt)
            share = float((lo != hi).double().mean())
            assert share <= 0.05, (mode, fmt, layer, share)
            if mode != "bf16x3":      # (the simulation multiplies hi + lo whole; aux_only takes the lo lo products off as the kernel does)
                got, _ = simulate(sd2, pts, feat, tau, mode, fmt)
                code = got.code[step[0]].to(torch.int64)
                assert bool(((code == mid) | (lo != hi)).all()), (mode, fmt, layer)
