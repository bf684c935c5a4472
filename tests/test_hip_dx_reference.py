"""The dX kernel (sr_satnerf_mlp_bwd) against the float64 chain of tests/dx_reference.py, stage by stage.

The kernel is driven as test_generated_dx_trunk_writes_the_same_bytes_as_the_compiler_scheduled_one drives it: a real saved state from
ops.satnerf_mlp(..., acts=acts, fmt=fmt), seeded random output gradients, ops.satnerf_mlp_bwd; ops._ws_empty is patched so that every
workspace is pre-filled with a known byte and followed by a canary.

a. SR_FMT16 (width 256 only: width 512 has no 16-bit workspaces, the C ABI refuses them -- test_width_512_has_no_16_bit_workspaces):
   the workspace holds exactly the bf16 vector the next stage consumes, so every stage is checked from the DECODED output of the stage
   above, nothing modelled:   |got - M| <= 2^-8 |M| + (k_steps 2^-24 + eps_cos) A + 1e-30
   (one bf16 rounding; the deterministic fp32 accumulation bound; eps_cos = 2^-19, the assumption about v_cos_f32 stated in
   dx_reference.py; identity stages carry no cos term).  d_t is stored from the fp32 accumulator: |got - M| <= k_steps 2^-24 A.  The head
   rows are held to the float64 formulas within one bf16 ulp (room for expf).
b. SR_FMT8, both widths, generated trunk and SATNERF_BWD_V1=1: the whole chain under the operand model, per column (one slot of one
   fragment over the points below n_points):   |got - M_rounded|_2 <= |q|_2 + |M_rounded - M_exact|_2
   q = the half step 2^(E - 134) of each decoded lane (the deterministic MX8 quantisation bound; 0 for the bf16 rows), the second term the
   size of the arithmetic's own rounding noise.  Neither term comes from the kernel and neither is tuned.  d_t: sum |w| q of its input in
   place of |q|.  Asserted in chain order, so the first failing stage is the one reported.
c. MX8 self-consistency in exact integers; d. bitwise linearity in 2^k; e. NULL gradients = zero gradients; f. padding and bounds;
g. either side of the generated trunk's 32-bit offset bound; h. s-nerf; i. a flipped weight of fc_net.8 fails check b at bL4.

Width 512 therefore has only the whole-chain check (b) and the integer checks; the per-stage check (a) covers the pre-trunk C++ both
formats and both widths' sources share, and the compiler-scheduled trunk the byte-equality test ties the generated one to."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from oracle import satnerf_oracle as O

from . import dx_reference as X
from . import wgrad_reference as W

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL, CANARY = 0x5a, 4096
# width, tau-independent (n_rays, n_samples): two tiles / a quarter-full last tile / a second workgroup part live / several workgroups
SHAPES = {256: [(1, 64), (3, 40), (5, 64), (41, 64)], 512: [(1, 64), (3, 40), (3, 64), (9, 64)]}
CASES = [(feat, tau, r, s) for feat in (256, 512) for tau in (4, 16) for r, s in SHAPES[feat]]


class Arena:
    """ops._ws_empty with known content: every byte FILL, CANARY elements behind each workspace."""

    def __init__(self):
        self.bufs = []

    def __call__(self, n, dtype, device, slot):
        base = torch.empty(n + CANARY, dtype=dtype, device=device)
        base.view(torch.uint8).fill_(FILL)
        self.bufs.append((slot, base, n))
        return base[:n]

    def canaries_intact(self):
        return all(bool((base[n:].view(torch.uint8) == FILL).all()) for _, base, n in self.bufs)


@pytest.fixture(autouse=True)
def arena(monkeypatch):
    from satnerf_amd import ops

    a = Arena()
    monkeypatch.setattr(ops, "_ws_empty", a)
    return a


_MODELS = {}


def model_of(feat, tau, snerf=False):
    from satnerf_amd.models import load_model

    key = (feat, tau, snerf)
    if key not in _MODELS:
        args = O.default_args(model="s-nerf" if snerf else "sat-nerf", t_embbeding_tau=tau, fc_units=feat)
        m = load_model(args)
        m.load_state_dict(O.procedural_snerf_params(feat, seed=21) if snerf else O.procedural_satnerf_params(feat, tau, seed=21))
        m = m.to(DEV)
        if snerf:
            emb = m.dummy_embedding()
        else:
            emb = torch.nn.Embedding(30, tau)
            emb.load_state_dict({"weight": O.procedural_uniform((30, tau), 1.0, 22)})
            emb = emb.to(DEV)
        _MODELS[key] = (m, emb)
    return _MODELS[key]


def forward(feat, tau, n_rays, s, mode="bf16", fmt=8, snerf=False):
    """A real saved state: the packed streams of procedural weights, the forward's acts workspace and its four outputs."""
    from satnerf_amd import ops

    model, emb = model_of(feat, tau, snerf)
    rays, ts = O.synthetic_rays(n_rays, seed=9 + n_rays)
    rays, ts = rays.to(DEV), (torch.zeros_like(ts) if snerf else ts).to(DEV)
    n = n_rays * s
    model.repack(mode, backward=True)
    hi, lo, l0 = model.packed(mode)
    bstream, _ = model.packed_backward()
    u = torch.rand(n_rays, s, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n))
    z = ops.ray_sample(rays, u, s)
    acts = ops.acts_workspace(n, feat, DEV, fmt)
    outs = ops.satnerf_mlp(rays[:, 0:3], rays[:, 3:6], rays[:, 8:11], z, emb.weight.data, ts, n, s, feat, tau, mode, hi, lo, l0, acts=acts, fmt=fmt)
    sd = {k: p.detach() for k, p in model.named_parameters()}
    return types.SimpleNamespace(feat=feat, tau=tau, n=n, fmt=fmt, model=model, bstream=bstream, acts=acts, outs=outs, sd=sd, snerf=snerf)


def random_grads(n, seed=3, snerf=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    ga, gs, gv, gb = (torch.randn(n, 3, device=DEV, generator=g) * 1e-3, torch.randn(n, device=DEV, generator=g) * 1e-3,
                      torch.randn(n, device=DEV, generator=g) * 1e-3, torch.randn(n, device=DEV, generator=g) * 1e-4)
    return (ga, gs, gv, None if snerf else gb)


def backward(st, grads, v1=False):
    from satnerf_amd import ops

    mp = pytest.MonkeyPatch()
    mp.setenv("SATNERF_BWD_V1", "1" if v1 else "0")   # (read per launch)
    try:
        dpre, d_t = ops.satnerf_mlp_bwd(st.feat, st.tau, st.n, st.bstream, st.acts, *st.outs, *grads, fmt=st.fmt)
        torch.cuda.synchronize()
    finally:
        mp.undo()
    assert d_t.shape == (st.n, st.tau)
    return dpre, d_t


# ---------------------------------------------------------------------------------------------------------------- the checks
def decode(st, dpre):
    geo = X.geometry(st.feat, st.tau)
    rows, cols, emax = W.decode_workspaces(dpre, st.acts, st.n, st.feat, st.tau, st.fmt)
    phases = {k: v[:st.n] for k, v in X.phases_from_acts(cols, geo).items()}
    return geo, rows, phases, emax


def dead_slots_are_zero(rows, geo):
    """Slots of the two bf16 row fragments no head row lives in (rows 5 .. 15 of d_head, 1 .. 15 of d_sigma_pre) hold bf16 zero."""
    for k, live in geo["live"].items():
        v = X._natural(rows, geo["dp"][k][0], 16, lambda op: op.exact())
        assert float(v[:, live:].abs().max()) == 0.0, k


def chain_ratios(st, dpre, d_t, grads):
    """Check b: [(stage, key, worst |got - M_rounded|_2 / bound over the key's columns)] in chain order."""
    geo, rows, phases, _ = decode(st, dpre)
    dead_slots_are_zero(rows, geo)
    got = {k: v[:st.n] for k, v in X.decoded_vectors(rows, geo).items()}
    got["dt"] = d_t.to(torch.float64)
    q = {k: v[:st.n] for k, v in X.decoded_vectors(rows, geo, X.half_step).items()}
    wb = X.weights(st.sd, True, DEV)["beta_from_xyz.0.weight"][:, st.feat:st.feat + st.tau].abs()
    q["dt"] = q["e1"] @ wb                                  # sum |w| q of d_t's input
    exact = X.chain(st.sd, phases, st.outs, grads, st.feat, st.tau, rounded=False)
    model = X.chain(st.sd, phases, st.outs, grads, st.feat, st.tau, rounded=True)
    out = []
    for stage, key in [("head", "head"), ("head", "sigma")] + [(s[0], s[1]) for s in X.steps(st.feat, st.tau)]:
        err = (got[key] - model[key]).norm(dim=0)
        bound = q[key].norm(dim=0) + (model[key] - exact[key]).norm(dim=0)
        ok = err <= bound
        ratio = torch.where(ok & (bound == 0), torch.zeros_like(err), err / bound.clamp_min(1e-300))
        out.append((stage, key, float(ratio.max())))
    return out


def check_b(st, dpre, d_t, grads, label):
    ratios = chain_ratios(st, dpre, d_t, grads)
    stage, key, worst = max(ratios, key=lambda r: r[2])
    print(f"{label}: worst |got - M_rounded| / bound = {worst:.3f} at {stage} ({key})")
    for stage, key, r in ratios:   # chain order: the first failing stage is the one reported
        assert r <= 1.0, (label, stage, key, r)
    return worst


def check_c(st, dpre, zero_keys=()):
    """MX8 self-consistency of every lane of a valid point, and the table of exponent maxima recomputed from the bytes just written."""
    from satnerf_amd import packing

    geo, rows, _, emax = decode(st, dpre)
    for key in X.MX_KEYS:
        u, e = X.lanes(rows, geo, key)
        u, e = u[:st.n], e[:st.n]
        if key in zero_keys:   # (s-nerf: the frozen zero uncertainty head hands nothing on: the encoder's zero lane, code 128 at the clamp E = 6)
            assert bool((u == 128).all()) and bool((e == 6).all()), key
            continue
        big = (u - 128).abs().amax(-1)
        assert int(u.min()) >= 1 and int(u.max()) <= 255, key
        assert int(big.min()) >= 64 - 1 and int(big.max()) <= 127, (key, int(big.min()), int(big.max()))
        assert int(e.min()) > 6, key    # random gradients: no valid lane is all zero, so none sits at the clamp
    wt, n_tiles = W.ws_tiles(st.n), (st.n + 31) // 32
    dk, ak = packing.dpre8_units(st.feat), packing.act8_units(geo["auxs"], st.feat)
    D = dpre.view(torch.uint8)[:wt * dk * 1024].view(wt, dk, 64, 16)
    A = st.acts.view(torch.uint8)[:wt * ak * 1024].view(wt, ak, 64, 16)
    used = (n_tiles + W.EMAX_TILES - 1) // W.EMAX_TILES     # the entries of real tiles
    want = W.emax_table(D, A, st.n, st.feat, st.tau)[:used]
    assert torch.equal(emax[:used], want), (emax[:used] != want).nonzero()[:8]


# ---------------------------------------------------------------------------------------------------------------- a
def test_width_512_has_no_16_bit_workspaces():
    """packing.backward_maps says so; the C ABI agrees: no size for them, and the launch is refused before anything runs."""
    from satnerf_amd import _lib, ops

    lib = _lib.lib()
    assert lib.sr_dpre_workspace_elems(64, 512, 16) <= 0 and lib.sr_act_elems_per_tile(512, 16) <= 0
    assert lib.sr_dpre_workspace_elems(64, 512, 8) > 0 and lib.sr_dpre_workspace_elems(64, 256, 16) > 0
    with pytest.raises(ValueError):
        ops.acts_workspace(64, 512, DEV, 16)
    t = torch.zeros(64 * 4, device=DEV)
    with pytest.raises(_lib.SatRenderError, match="8-bit workspaces only"):
        _lib.call("sr_satnerf_mlp_bwd", 512, 4, 64, ops._p(t), ops._p(t), ops._p(t), ops._p(t), ops._p(t), ops._p(t), None, None, None, None,
                  ops._p(t), None, 16, ops._stream())


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("tau,n_rays,s", [(tau, r, s) for tau in (4, 16) for r, s in SHAPES[256]])
def test_every_stage_from_the_decoded_stage_above_fmt16(mode, tau, n_rays, s):
    st = forward(256, tau, n_rays, s, mode=mode, fmt=16)
    grads = random_grads(st.n)
    dpre, d_t = backward(st, grads)
    geo, rows, phases, _ = decode(st, dpre)
    dead_slots_are_zero(rows, geo)
    dec = {k: v[:st.n] for k, v in X.decoded_vectors(rows, geo).items()}
    dec["dt"] = d_t.to(torch.float64)
    # head rows: the float64 formulas within one bf16 ulp (room for expf)
    for key, want in zip(("head", "sigma"), X.head_grads(st.outs, grads)):
        ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(1e-300))) - 7)
        assert bool(((dec[key] - want).abs() <= ulp).all()), (key, float(((dec[key] - want).abs() / ulp).max()))
    wts = X.weights(st.sd, True, DEV)
    for step in X.steps(256, tau):
        stage, key, ph, k_steps, _ = step
        M, A = X.stage(step, dec, wts, phases)
        err = (dec[key] - M).abs()
        if key == "dt":   # stored from the fp32 accumulator
            gate = k_steps * 2.0 ** -24 * A
        else:
            gate = 2.0 ** -8 * M.abs() + (k_steps * 2.0 ** -24 + (X.EPS_COS if ph else 0.0)) * A + 1e-30
        bad = err > gate
        r = float(torch.where(gate > 0, err / gate.clamp_min(1e-300), err * 1e300).max())
        print(f"fmt16 {mode} tau{tau} {n_rays}x{s} {stage} ({key}): worst |got - M| / gate = {r:.3f}")
        assert not bad.any(), (stage, key, int(bad.sum()), r)


# ---------------------------------------------------------------------------------------------------------------- b, c
@pytest.mark.parametrize("feat,tau,n_rays,s", CASES)
def test_whole_chain_and_mx8_bytes_fmt8(feat, tau, n_rays, s):
    st = forward(feat, tau, n_rays, s)
    grads = random_grads(st.n)
    for v1 in (False, True):
        dpre, d_t = backward(st, grads, v1=v1)
        check_b(st, dpre, d_t, grads, f"fmt8 w{feat} tau{tau} {n_rays}x{s} {'compiler-scheduled' if v1 else 'generated'} trunk")
        check_c(st, dpre)


# ---------------------------------------------------------------------------------------------------------------- d
@pytest.mark.parametrize("feat,n_rays", [(256, 5), (512, 3)])
def test_scaling_the_gradients_by_a_power_of_two_is_bitwise(feat, n_rays):
    """2^k is exact in every operation of the chain (nothing near denormal or overflow at these magnitudes): identical MX8 codes, scale
    bytes and bf16 exponents shifted by k, d_t scaled exactly."""
    from satnerf_amd import packing

    tau = 4
    st = forward(feat, tau, n_rays, 64)
    grads = random_grads(st.n)
    g8 = packing.fmt8_geometry(feat)
    n_tiles, dk = st.n // 32, packing.dpre8_units(feat)
    view = lambda d: d.view(torch.uint8)[:n_tiles * dk * 1024].view(n_tiles, dk, 64, 16).to(torch.int32)  # noqa: E731
    dpre0, dt0 = backward(st, grads)
    _, _, phases, _ = decode(st, dpre0)
    D0 = view(dpre0)
    raw0 = dpre0.view(torch.uint8)[:n_tiles * dk * 1024].view(n_tiles, dk, 64, 16)[:, g8["D8_SIGMA"]:g8["D8_SCALE"]].contiguous().view(torch.int16).to(torch.int32) & 0xffff
    ref0 = X.chain(st.sd, phases, st.outs, grads, feat, tau, rounded=True)
    mt, gpu = g8["MT"], g8["GROUPS_PER_UNIT"]
    for k in (-20, 20):
        gk = tuple(g * 2.0 ** k for g in grads)
        refk = X.chain(st.sd, phases, st.outs, gk, feat, tau, rounded=True)
        assert all(torch.equal(refk[key], ref0[key] * 2.0 ** k) for key in ref0)   # the reference: exact
        dprek, dtk = backward(st, gk)
        Dk = view(dprek)
        assert torch.equal(Dk[:, :g8["D8_SIGMA"]], D0[:, :g8["D8_SIGMA"]]), k          # MX8 code bytes
        for g in range(14):                                                            # scale bytes of every group's tiles
            nb = mt if g < 9 else g8["MTH"]
            sl = (slice(None), g8["D8_SCALE"] + g // gpu, slice(None), slice((g % gpu) * mt, (g % gpu) * mt + nb))
            assert int(D0[sl].min()) > 6 and torch.equal(Dk[sl], D0[sl] + k), (k, g)
        rawk = dprek.view(torch.uint8)[:n_tiles * dk * 1024].view(n_tiles, dk, 64, 16)[:, g8["D8_SIGMA"]:g8["D8_SCALE"]].contiguous().view(torch.int16).to(torch.int32) & 0xffff
        want = torch.where((raw0 & 0x7fff) == 0, raw0, raw0 + (k << 7))                # bf16 rows: exponent field + k, zeros stay
        assert torch.equal(rawk, want), k
        assert torch.equal(dtk, dt0 * 2.0 ** k), k


# ---------------------------------------------------------------------------------------------------------------- e
@pytest.mark.parametrize("which", range(4), ids=["g_albedo", "g_sigma", "g_sun_v", "g_beta"])
def test_a_null_gradient_is_a_zero_gradient(which):
    """train.py's solar-correction and depth passes hand the kernel NULL for the gradients they do not have."""
    st = forward(256, 4, 5, 64)
    grads = random_grads(st.n)
    zeros = tuple(torch.zeros_like(g) if i == which else g for i, g in enumerate(grads))
    nulls = tuple(None if i == which else g for i, g in enumerate(grads))
    for v1 in (False, True):
        (d0, t0), (d1, t1) = backward(st, zeros, v1=v1), backward(st, nulls, v1=v1)
        assert torch.equal(d0, d1) and torch.equal(t0, t1), v1


# ---------------------------------------------------------------------------------------------------------------- f
@pytest.mark.parametrize("feat,fmt,mode", [(256, 8, "bf16"), (512, 8, "bf16"), (256, 16, "bf16x3")])
def test_padding_and_bounds(arena, feat, fmt, mode):
    """120 points, the last tile a quarter full, everything behind point 119 in acts random bytes, every per-point array exactly n_points
    long: zero pre-activation gradients at points >= n_points (code 128, scale byte 6, bf16 0), nothing written behind either output."""
    from satnerf_amd import _lib, ops, packing

    tau = 4
    st = forward(feat, tau, 3, 40, mode=mode, fmt=fmt)
    assert st.n == 120 and all(o.shape[0] == 120 for o in st.outs)
    auxs = packing.aux_steps(tau)
    ak = packing.act8_units(auxs, feat) if fmt == 8 else auxs + 9 * (feat // 16) + 5 * (feat // 32)
    a8 = st.acts.view(torch.uint8)
    gen = torch.Generator(device=DEV).manual_seed(4)
    rnd = torch.randint(0, 256, (a8.numel(),), device=DEV, dtype=torch.uint8, generator=gen)
    pad = torch.zeros(a8.numel(), dtype=torch.bool, device=DEV)
    pad[4 * ak * 1024:] = True
    pad[3 * ak * 1024:4 * ak * 1024].view(ak, 2, 32, 16)[:, :, 24:] = True      # lanes (p >= 24, h) of the last tile
    a8[pad] = rnd[pad]
    grads = random_grads(st.n)
    n_elems = _lib.lib().sr_dpre_workspace_elems(st.n, feat, fmt)
    dpre = arena(n_elems, torch.int16, DEV, 2)
    sentinel = 12345.0
    dt_base = torch.full((st.n * tau + CANARY,), sentinel, device=DEV)
    d_t = dt_base[:st.n * tau].view(st.n, tau)
    _lib.call("sr_satnerf_mlp_bwd", feat, tau, st.n, ops._p(st.bstream), ops._p(st.acts), *(ops._p(o) for o in st.outs), *(ops._p(g) for g in grads),
              ops._p(dpre), ops._p(d_t), fmt, ops._stream())
    torch.cuda.synchronize()
    assert arena.canaries_intact()
    assert bool((dt_base[st.n * tau:] == sentinel).all()) and bool((d_t != sentinel).all())
    geo, rows, _, _ = decode(st, dpre)
    for f, op in rows.items():   # the padding contract of the weight-gradient kernels, which mask nothing
        assert op.exact().shape[0] == 128 and float(op.exact()[st.n:].abs().max()) == 0.0, f
    if fmt == 8:
        g8 = packing.fmt8_geometry(feat)
        dk = packing.dpre8_units(feat)
        last = dpre.view(torch.uint8)[3 * dk * 1024:4 * dk * 1024].view(dk, 2, 32, 16)[:, :, 24:]
        assert bool((last[:g8["D8_SIGMA"]] == 128).all()) and bool((last[g8["D8_SIGMA"]:g8["D8_SCALE"]] == 0).all())
        mt, gpu = g8["MT"], g8["GROUPS_PER_UNIT"]
        for g in range(14):
            nb = mt if g < 9 else g8["MTH"]
            assert bool((last[g8["D8_SCALE"] + g // gpu, :, :, (g % gpu) * mt:(g % gpu) * mt + nb] == 6).all()), g
        check_b(st, dpre, d_t, grads, f"fmt8 w{feat} tau{tau} 3x40, random bytes behind the last point")
        check_c(st, dpre)


# ---------------------------------------------------------------------------------------------------------------- g
def offset_bound_case():
    """Width 256: the largest n_points whose workspaces stay below the generated trunk's 32-bit per-lane offsets (launch_bwd_fmt:
    ws_tiles max(kD8Units, act8_units(2)) 1024 < 2^32) and the smallest at the bound, which goes to the compiler-scheduled trunk.
    Synthetic acts (random phase bytes, feats scale bytes in synthetic_fmt8's range), written through plain slices only: an index kernel
    over a buffer past 4 GiB faults.  Check b on the first 8 and the last 8 tiles: the reference never sees more than 512 points."""
    from satnerf_amd import ops, packing

    feat, tau = 256, 4
    auxs = packing.aux_steps(tau)
    g8 = packing.fmt8_geometry(feat)
    dk, ak = packing.dpre8_units(feat), packing.act8_units(auxs, feat)
    per = max(dk, packing.act8_units(2, feat)) * 1024
    wt_hi = ((1 << 32) + per - 1) // per
    wt_hi = (wt_hi + 7) // 8 * 8
    wt_lo = wt_hi - 8
    assert wt_lo * per < (1 << 32) <= wt_hi * per
    model, _ = model_of(feat, tau)
    model.repack("bf16", backward=True)
    bstream, _ = model.packed_backward()
    sd = {k: p.detach() for k, p in model.named_parameters()}
    for n in (32 * wt_lo, 32 * wt_lo + 1):
        assert W.ws_tiles(n) == (wt_lo if n == 32 * wt_lo else wt_hi)
        n_tiles = (n + 31) // 32
        gen = torch.Generator(device=DEV).manual_seed(n % 1000)
        acts = ops.acts_workspace(n, feat, DEV, 8)
        a8 = acts.view(torch.uint8)
        step = 1 << 30
        for off in range(0, a8.numel(), step):
            m = min(step, a8.numel() - off)
            a8[off:off + m] = torch.randint(0, 256, (m,), device=DEV, dtype=torch.uint8, generator=gen)
        for t0 in range(0, n_tiles, 4096):   # feats scale bytes, a run of tiles at a time
            t1 = min(t0 + 4096, n_tiles)
            a8[t0 * ak * 1024:t1 * ak * 1024].view(t1 - t0, ak, 64, 16)[:, auxs + g8["A8_SCALE"], :, :g8["MT"]] = \
                torch.randint(118, 131, (t1 - t0, 64, g8["MT"]), device=DEV, dtype=torch.uint8, generator=gen)
        outs = (torch.rand(n, 3, device=DEV, generator=gen), torch.rand(n, device=DEV, generator=gen) * 2, torch.rand(n, device=DEV, generator=gen),
                torch.rand(n, device=DEV, generator=gen) + 0.05)
        grads = random_grads(n)
        dpre, d_t = ops.satnerf_mlp_bwd(feat, tau, n, bstream, acts, *outs, *grads, fmt=8)
        torch.cuda.synchronize()
        for name, tiles in (("first", range(0, 8)), ("last", range(n_tiles - 8, n_tiles))):
            p0, p1 = 32 * tiles[0], min(32 * (tiles[-1] + 1), n)
            st = types.SimpleNamespace(feat=feat, tau=tau, n=p1 - p0, fmt=8, sd=sd, acts=W.gather_tiles(a8, ak, tiles),
                                       outs=tuple(o[p0:p1] for o in outs))
            check_b(st, W.gather_tiles(dpre.view(torch.uint8), dk, tiles), d_t[p0:p1], tuple(g[p0:p1] for g in grads),
                    f"fmt8 w256 tau4 {n} points ({'below' if n == 32 * wt_lo else 'at'} the 32-bit bound), {name} 8 tiles")
        del acts, a8, dpre, d_t, outs, grads


BOUND_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from tests.test_hip_dx_reference import offset_bound_case
offset_bound_case()
"""


def test_either_side_of_the_generated_trunks_32_bit_offset_bound():
    """In a child process under its own time limit (two launches on 8.3 GB of workspaces each)."""
    need = 14 << 30
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"neither launch can be made here: the case needs {need >> 30} GiB of device memory for its workspaces, {free >> 30} GiB are free")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", BOUND_CHILD, ROOT], capture_output=True, text=True, cwd=ROOT)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------------------- h
def test_snerf_whole_chain_and_mx8_bytes():
    """s-nerf runs on the Sat-NeRF kernels with a frozen zero uncertainty head (models.ShadowNeRF; the entry test_hip_snerf.py's trainer
    reaches): g_beta NULL, ts = 0 into the one-row zero embedding.  d e1 and d_t are exactly zero: those lanes, and only those, are the
    encoder's zero lane."""
    st = forward(256, 4, 5, 64, snerf=True)
    grads = random_grads(st.n, snerf=True)
    assert grads[3] is None and all(float(p.abs().max()) == 0.0 for k, p in st.sd.items() if k.startswith("beta_from_xyz"))
    for v1 in (False, True):
        dpre, d_t = backward(st, grads, v1=v1)
        assert float(d_t.abs().max()) == 0.0
        check_b(st, dpre, d_t, grads, f"fmt8 s-nerf w256 5x64 {'compiler-scheduled' if v1 else 'generated'} trunk")
        check_c(st, dpre, zero_keys=("e1",))


# ---------------------------------------------------------------------------------------------------------------- i
def test_a_flipped_weight_of_the_skip_layer_fails_the_gate_at_bL4():
    """The check notices what it is for: one bf16 element of the packed transposed stream, in the part that holds fc_net.8, with its sign
    flipped (data, not code: nothing faults).  Check b passes up to bL5, fails at bL4, and passes everywhere without the flip."""
    from satnerf_amd import packing

    st = forward(256, 4, 5, 64)
    grads = random_grads(st.n)
    order = ["head"] + X.STAGES
    clean = chain_ratios(st, *backward(st, grads), grads)
    assert all(r <= 1.0 for _, _, r in clean)
    bm = packing.backward_maps(256, 4)
    off, shp = bm["offsets"]["fc_net.8.weight"]
    pos = np.nonzero((bm["idx"] >= off) & (bm["idx"] < off + shp[0] * shp[1]))[0]
    w = st.model.flat_params().detach()[torch.from_numpy(bm["idx"][pos].astype(np.int64)).to(DEV)].abs()
    at = int(pos[int(w.argmax())])                                   # the largest weight of the layer
    assert st.bstream[at].item() != 0
    st.bstream[at] ^= -32768
    try:
        bad = chain_ratios(st, *backward(st, grads), grads)
    finally:
        st.bstream[at] ^= -32768
    first = next(stage for stage, _, r in bad if r > 1.0)
    assert first == "bL4", bad
    assert all(r <= 1.0 for stage, _, r in bad if order.index(stage) < order.index("bL4"))
