"""The training forward (sr_satnerf_mlp_fwd with an acts workspace) against the float64 chain of tests/fwd_reference.py: what dX and the
weight-gradient kernels take as given.

Driven as tests/test_hip_dx_reference.py drives it: procedural weights, model.repack(mode, backward=True), ops.ray_sample +
ops.satnerf_mlp(..., acts=acts, fmt=fmt); ops._ws_empty is patched so that every workspace is pre-filled with a known byte and followed by
a canary.  Kernel matrix: width 256 -- (bf16, 8), (f16, 8) [satnerf_fwd2_kernel<SAVE>], (bf16, 16), (f16, 16) [the compiler-scheduled
satnerf_fwd_kernel], (bf16x3, 16) [satnerf_fwd3_kernel]; width 512 -- (bf16, 8), (f16, 8) [satnerf_fwd512g_kernel]; everything once more
under SATNERF_FWD_V1=1 (read once per process: ONE child process covers all cases with the compiler-scheduled kernel).

(W) the whole chain under the operand model, per column, in chain order; every case but bf16x3 (there the rounding-noise term is as small
    as the kernel's own fp32 error):   |wrap(got - M_rounded)|_2 <= |q|_2 + |wrap(M_rounded - M_exact)|_2      (fwd_reference.gate_w)
    The four outputs do NOT join it with q = 0: the CPU simulation's worst output ratio is 0.55 > 0.5 (fwd_reference.OUTPUTS_IN_W); their
    ratios are printed, (S) and the golden tests hold them.
(S) every stage from the decoded stage above, per element, the three 16-bit cases:
    |wrap(got - M)| <= q + k_steps n_pass 2^-24 A + amb                                                     (fwd_reference.gate_s)
(E) the encoders in exact integers: ONE stage's weight all zero, its bias a chosen pattern -- the accumulator is R(b c) x 1.0 on top of
    exact zeros, known exactly -- and every valid point's stored code must be the restated encoder of that value, bit for bit; swept over
    every stage of every kernel.  The other stages of such a launch still pass (W) -- except, in the 16-bit format, the stages
    DOWNSTREAM of the swept one, which get (S): there every point holds the same pre-activation, a hand-off whose rounding the fp32 sine
    flips is flipped for all points at once, and (W)'s noise term no longer covers it (tests/test_fwd_reference_host.py shows the exact
    CPU simulation over (W) in that state).  Second variant for the three stages with aux columns: hidden block zero, aux columns live.
(X) structure: aux fragments bitwise, MX8 lanes, determinism, canaries, the last workgroup's tiles, ts at both ends of the table, input
    strides, s-nerf, either side of the generated streams' 32-bit offset bound, a planted fault.

Left out on purpose: render_train (existing tests tie it to satnerf_mlp byte for byte), bwd_fmt = 32, classic NeRF."""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from oracle import satnerf_oracle as O

from . import dx_reference as X
from . import fwd_reference as F
from . import wgrad_reference as W
from .test_hip_dx_reference import CANARY, DEV, FILL, ROOT, SHAPES, Arena

pytestmark = pytest.mark.gpu

MATRIX = {256: [("bf16", 8), ("f16", 8), ("bf16", 16), ("f16", 16), ("bf16x3", 16)], 512: [("bf16", 8), ("f16", 8)]}
CASES = [(feat, tau, mode, fmt, r, s) for feat in (256, 512) for tau in (4, 16) for mode, fmt in MATRIX[feat] for r, s in SHAPES[feat]]
KERNELS = [(feat, mode, fmt) for feat in (256, 512) for mode, fmt in MATRIX[feat]]
V1 = os.environ.get("SATNERF_FWD_V1", "")[:1] == "1"


@pytest.fixture(autouse=True)
def arena(monkeypatch):
    from satnerf_amd import ops

    a = Arena()
    monkeypatch.setattr(ops, "_ws_empty", a)
    return a


_MODELS, _PARAMS = {}, {}


def params_of(feat, tau, snerf=False):
    key = (feat, tau, snerf)
    if key not in _PARAMS:
        _PARAMS[key] = O.procedural_snerf_params(feat, seed=21) if snerf else O.procedural_satnerf_params(feat, tau, seed=21)
    return _PARAMS[key]


def model_of(feat, tau, snerf=False):
    from satnerf_amd.models import load_model

    key = (feat, tau, snerf)
    if key not in _MODELS:
        args = O.default_args(model="s-nerf" if snerf else "sat-nerf", t_embbeding_tau=tau, fc_units=feat)
        m = load_model(args).to(DEV)
        emb = m.dummy_embedding().weight.data if snerf else O.procedural_uniform((30, tau), 1.0, 22).to(DEV)
        _MODELS[key] = (m, emb)
    return _MODELS[key]


def forward(feat, tau, n_rays, s, mode, fmt, sd=None, snerf=False, ts_ends=False, contiguous=False, tamper=None, outs=None):
    """One launch on a state_dict (default: the procedural weights; every call loads its own, so no case sees another's) -> the saved
    state, the outputs, the inputs as the reference wants them.  ``tamper(hi, lo, l0)`` runs between the packer and the launch;
    ``outs``: caller-owned output tensors (the raw C entry is called with them)."""
    from satnerf_amd import _lib, ops

    model, emb = model_of(feat, tau, snerf)
    model.load_state_dict(sd if sd is not None else params_of(feat, tau, snerf))
    rays, ts = O.synthetic_rays(n_rays, seed=9 + n_rays)
    if ts_ends:
        ts[0], ts[-1] = 0, emb.shape[0] - 1
    rays, ts = rays.to(DEV), (torch.zeros_like(ts) if snerf else ts).to(DEV)
    n = n_rays * s
    model.repack(mode, backward=True)
    hi, lo, l0 = model.packed(mode)
    if tamper is not None:
        tamper(hi, lo, l0)
    u = torch.rand(n_rays, s, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n))
    z = ops.ray_sample(rays, u, s)
    org, direction, sun = rays[:, 0:3], rays[:, 3:6], rays[:, 8:11]       # rows of stride 11
    if contiguous:
        org, direction, sun = org.contiguous(), direction.contiguous(), sun.contiguous()
    acts = ops.acts_workspace(n, feat, DEV, fmt)
    if outs is None:
        outs = ops.satnerf_mlp(org, direction, sun, z, emb, ts, n, s, feat, tau, mode, hi, lo, l0, acts=acts, fmt=fmt)
    else:
        inp = _lib.MlpInputs(ops._p(org), org.stride(0), ops._p(direction), direction.stride(0), ops._p(sun), sun.stride(0), ops._p(z), ops._p(emb),
                             ops._p(ts), n, s)
        _lib.call("sr_satnerf_mlp_fwd", C.byref(inp), feat, tau, ops.MODES[mode], ops._p(hi), ops._p(lo), ops._p(l0), *(ops._p(o) for o in outs),
                  ops._p(acts), int(fmt), ops._stream())
    torch.cuda.synchronize()
    sd_dev = {k: p.detach().clone() for k, p in model.named_parameters()}
    pts = F.points(org, direction, z, sun, emb, ts, s)
    return types.SimpleNamespace(feat=feat, tau=tau, n=n, s=s, mode=mode, fmt=fmt, acts=acts, outs=outs, sd=sd_dev, pts=pts, model=model, ts=ts)


def label_of(st, extra=""):
    return f"{'V1 ' if V1 else ''}w{st.feat} tau{st.tau} {st.mode} fmt{st.fmt} {st.n // st.s}x{st.s}{extra}"


def ratios_w(st, got):
    return F.gate_w(got, st.outs, F.chain(st.sd, st.pts, st.feat, st.tau, st.mode), F.chain(st.sd, st.pts, st.feat, st.tau), st.n)


def check_w(st, got, label):
    """(W): asserted in chain order, so the first failing stage is the one reported; the outputs' ratios are printed only."""
    res = ratios_w(st, got)
    print(f"{label} (W): " + " ".join(f"{k} {r:.3f}" for k, r in res))
    for key, r in res:
        if key in F.CHAIN:      # (fwd_reference.OUTPUTS_IN_W: the outputs' ratios are printed only)
            assert r <= 1.0, (label, key, r)
    return max(r for k, r in res if k in F.CHAIN)


def check_s(st, got, label):
    res = F.gate_s(got, st.outs, st.sd, st.pts, st.feat, st.tau, st.mode, st.n)
    print(f"{label} (S): " + " ".join(f"{k} {r:.3f}" for k, r, _ in res))
    for key, r, bad in res:
        assert bad == 0, (label, key, r, bad)
    return max(r for _, r, _ in res)


def check_aux(st, got):
    """(X) the aux fragments are the bf16 rounding (the backward kernels' operand format, in every mode) of [sun, 1, xyz, 0, t .., 0],
    bitwise; xyz = org + z dir in fp32, fused or not."""
    bf = lambda v: v.float().to(torch.bfloat16).to(torch.float64)  # noqa: E731
    a, b = bf(F.aux_vector(st.pts, st.tau)), bf(F.aux_vector(st.pts, st.tau, st.pts.xyz_fma))
    g = got.aux[:st.n]
    assert g.shape == a.shape and bool(((g == a) | (g == b)).all()), ((g != a) & (g != b)).nonzero()[:8]
    assert not bool(torch.signbit(g[:, 7]).any()) and bool((g[:, 3] == 1).all())


def check_case(st, label=None):
    label = label or label_of(st)
    got = F.decode(st.acts, st.n, st.feat, st.tau, st.fmt)
    check_aux(st, got)
    if st.fmt == 8:
        assert not F.gate_lanes(got, st.n), (label, F.gate_lanes(got, st.n))
    w = check_w(st, got, label) if st.mode != "bf16x3" else None
    s = check_s(st, got, label) if st.fmt == 16 else None
    return w, s


# ---------------------------------------------------------------------------------------------------------------- W, S
@pytest.mark.parametrize("feat,tau,mode,fmt,n_rays,s", CASES)
def test_whole_chain_and_every_stage(arena, feat, tau, mode, fmt, n_rays, s):
    st = forward(feat, tau, n_rays, s, mode, fmt)
    check_case(st)
    assert arena.canaries_intact()


# ---------------------------------------------------------------------------------------------------------------- E
def swept_layers():
    return list(F.LAYERS)


HEAD_LAYERS = ["sigma_from_xyz.0", "rgb_from_xyzdir.2", "sun_v_net.6", "beta_from_xyz.2"]


def encoder_sweep(feat, tau, mode, fmt, variant=0, layers=None):
    """(E) on 3 x 40 points: -> {layer: mismatching codes}; asserts what is not a count."""
    key_of = {s[2]: s[0] for s in F.steps(feat, tau)}
    key_of["fc_net.0"] = "a0"
    base = params_of(feat, tau)
    out = {}
    for layer in layers or swept_layers():
        n_out = base[layer + ".bias"].shape[0]
        b, landed, _ = F.bias_pattern(layer, n_out, mode, seed=variant)
        if layer in F.SIN_LAYERS or layer == "fc_net.0":
            c = F.pattern_classes(landed, b)      # the pattern lands where it is meant to (tests/test_fwd_reference_host.py checks every class)
            assert c["codes"] == {0, 1, 127, 128, 255} and c["wraps"] and c["negative"] and c["plus_zero"] and c["minus_zero"], (layer, c)
            assert (c["tie_even"] and c["tie_odd"]) or fmt == 16, (layer, c)      # PHASE8's exact ties
        sd = dict(base)
        sd[layer + ".weight"], sd[layer + ".bias"] = torch.zeros_like(base[layer + ".weight"]), b
        st = forward(feat, tau, 3, 40, mode, fmt, sd=sd)
        got = F.decode(st.acts, st.n, feat, tau, fmt)
        key, lab = key_of[layer], label_of(st, f" (E) {layer}")
        v = landed.to(DEV)
        if key in got.code:
            want = F.phase8(v.float()) if fmt == 8 else F.unorm16(v.float())
            out[layer] = int((got.code[key][:st.n].to(torch.int64) != want[None, :]).sum())
        elif key == "feats" and fmt == 8:
            e, u = X.mx8_encode(F.to_lanes(v[None].float()))
            gu, ge = got.lanes
            out[layer] = int((gu[:st.n] != u).sum()) + int((ge[:st.n] != e).sum())
            assert int(ge[:st.n, 0, 1].max()) == 6 and bool((gu[:st.n, 0, 1] == 128).all()), lab      # the zero lane
        elif key == "feats":
            want = v.float().to(torch.bfloat16).to(torch.float64)
            out[layer] = int((got.feats[:st.n] != want[None, :]).sum())
        else:   # sigma_from_xyz and the head rows: the activation of the exact value, to 4 fp32 ulps
            name, cols = {"sigma_pre": ("sigma", None), "h_rgb": ("albedo", slice(0, 3)), "h_sun": ("sun_v", None), "h_beta": ("beta", None)}[key]
            head = torch.zeros(1, 5, dtype=torch.float64, device=DEV)
            pre_sigma = torch.zeros(1, 1, dtype=torch.float64, device=DEV)
            if key == "sigma_pre":
                pre_sigma[0] = v
            else:
                head[0, {"h_rgb": slice(0, 3), "h_sun": slice(3, 4), "h_beta": slice(4, 5)}[key]] = v
            want = F.activations(pre_sigma, head)[name]
            o = st.outs[F.OUTPUTS.index(name)].to(torch.float64).reshape(st.n, -1)
            err = (o - want.reshape(1, -1)).abs()
            out[layer] = int((err > 4 * F.ulp32(want.reshape(1, -1))).sum())
        # the other stages still pass (W); in the 16-bit format the stages downstream of the swept one get (S) (module header)
        res = [(k, r) for k, r in ratios_w(st, got) if k in F.CHAIN] if mode != "bf16x3" else []
        down = F.downstream(key) if fmt == 16 and key in F.CHAIN else []
        assert all(r <= 1.0 for k, r in res if k not in down), (lab, [x for x in res if x[1] > 1.0 and x[0] not in down])
        over = [(k, round(r, 3)) for k, r in res if k in down and r > 1.0]
        if over:
            print(f"{lab}: (W) over 1 downstream of the constant stage (held by (S)): {over}")
        if fmt == 16:
            sg = F.gate_s(got, st.outs, st.sd, st.pts, feat, tau, mode, st.n)
            assert all(bad == 0 for _, _, bad in sg), (lab, [x for x in sg if x[2]])
    return out


@pytest.mark.parametrize("feat,mode,fmt", KERNELS)
def test_encoders_in_exact_integers(arena, feat, mode, fmt):
    miss = encoder_sweep(feat, 4, mode, fmt)
    print(f"{'V1 ' if V1 else ''}w{feat} {mode} fmt{fmt} (E): mismatching codes per swept stage: {miss}")
    assert set(miss) == set(F.LAYERS) and all(v == 0 for v in miss.values()), miss
    assert arena.canaries_intact()


@pytest.mark.parametrize("feat,mode,fmt", KERNELS)
def test_head_rows_second_values(arena, feat, mode, fmt):
    """The other head values (a sigma past softplus's threshold 20 among them), at tau 16: two aux k-steps, the bias column in the first."""
    miss = encoder_sweep(feat, 16, mode, fmt, variant=1, layers=HEAD_LAYERS)
    print(f"{'V1 ' if V1 else ''}w{feat} tau16 {mode} fmt{fmt} (E) head rows, second values: {miss}")
    assert set(miss) == set(HEAD_LAYERS) and all(v == 0 for v in miss.values()), miss
    assert arena.canaries_intact()


def aux_sweep(feat, tau, mode, fmt):
    """(E), second variant, for the three stages with aux columns (fc_net.8 <- xyz, sun_v_net.0 <- sun, beta_from_xyz.0 <- t): the hidden
    block zero, the aux columns and the bias as they are (fwd_reference.aux_only).  Wherever S +- e lies inside one code cell the stored
    code is within one step of the encoder of the float64 sum S; where it straddles a boundary, within one step of either neighbour.
    -> {layer: (codes further off, codes not EQUAL to the encoder of S outside the straddling ones, share of straddling ones)}."""
    base = params_of(feat, tau)
    span = 256 if fmt == 8 else 65536
    out = {}
    for layer, hid in F.AUX_STAGES.items():
        w = base[layer + ".weight"].clone()
        w[:, hid if hid is not None else slice(0, feat)] = 0.0
        sd = dict(base)
        sd[layer + ".weight"] = w
        st = forward(feat, tau, 3, 40, mode, fmt, sd=sd)
        got = F.decode(st.acts, st.n, feat, tau, fmt)
        step = next(x for x in F.steps(feat, tau) if x[2] == layer)
        _, lo, mid, hi = F.aux_only(step, st.sd, st.pts, feat, tau, mode, fmt)
        code = got.code[step[0]][:st.n].to(torch.int64)
        dist = lambda a, b: torch.minimum((a - b) % span, (b - a) % span)  # noqa: E731
        straddle = lo != hi
        ok = torch.where(straddle, torch.minimum(dist(code, lo), dist(code, hi)) <= 1, dist(code, mid) <= 1)
        out[layer] = (int((~ok).sum()), int(((code != mid) & ~straddle).sum()), float(straddle.double().mean()))
    return out


@pytest.mark.parametrize("feat,mode,fmt", KERNELS)
def test_aux_columns_alone_give_the_encoder_of_their_exact_sum(arena, feat, mode, fmt):
    for tau in (4, 16):
        res = aux_sweep(feat, tau, mode, fmt)
        print(f"{'V1 ' if V1 else ''}w{feat} tau{tau} {mode} fmt{fmt} (E) aux columns alone: (codes off, codes not equal, straddling share) {res}")
        assert all(bad == 0 and share <= 0.05 for bad, _, share in res.values()), res
    assert arena.canaries_intact()


# ---------------------------------------------------------------------------------------------------------------- X
def tiles_view(st):
    from satnerf_amd import _lib

    per = _lib.lib().sr_act_elems_per_tile(st.feat, st.fmt) * 2
    wt = _lib.lib().sr_workspace_tiles(st.n)
    assert st.acts.numel() * 2 == wt * per
    return st.acts.view(torch.uint8).view(wt, per)


@pytest.mark.parametrize("feat,mode,fmt", KERNELS)
def test_two_runs_write_the_same_bytes_and_nothing_else(arena, feat, mode, fmt):
    """Determinism, canaries behind acts and behind the four outputs, the tiles past n_points (dX and the weight-gradient kernels read
    whole tiles: whatever the kernel computes there for its clamped inputs is the same on both runs), ts at both ends of the table."""
    tau, n_rays, s = 4, 3, 40
    n = n_rays * s

    def owned():
        base = [torch.full((k + CANARY,), 12345.0, device=DEV) for k in (3 * n, n, n, n)]
        return base, (base[0][:3 * n].view(n, 3), base[1][:n], base[2][:n], base[3][:n])

    runs = []
    for _ in range(2):
        base, outs = owned()
        st = forward(feat, tau, n_rays, s, mode, fmt, ts_ends=True, outs=outs)
        assert int(st.ts.min()) == 0 and int(st.ts.max()) == 29
        assert all(bool((b[k:] == 12345.0).all()) for b, k in zip(base, (3 * n, n, n, n))) and all(bool((o != 12345.0).all()) for o in outs)
        runs.append((st, tiles_view(st).clone(), [o.clone() for o in outs]))
    assert arena.canaries_intact()
    (st, a0, o0), (_, a1, o1) = runs
    assert torch.equal(a0, a1) and all(torch.equal(x, y) for x, y in zip(o0, o1))
    n_tiles = (n + 31) // 32
    untouched = [t for t in range(a0.shape[0]) if bool((a0[t] == FILL).all())]
    print(f"{label_of(st)}: {a0.shape[0]} workspace tiles, {n_tiles} hold points, never written: {untouched}")
    assert all(t >= n_tiles for t in untouched)
    check_case(st, label_of(st, " ts at both ends"))
    # the same launch through ops.satnerf_mlp (its own output tensors) and with contiguous org / dir / sun rows: the same bytes
    for kw in ({}, {"contiguous": True}):
        st2 = forward(feat, tau, n_rays, s, mode, fmt, ts_ends=True, **kw)
        assert torch.equal(tiles_view(st2), a0) and all(torch.equal(x, y) for x, y in zip(st2.outs, o0)), kw


def test_snerf_whole_chain():
    """s-nerf runs on the Sat-NeRF kernels with a frozen zero uncertainty head, ts = 0 into the one-row zero embedding: e1 is phase 0."""
    st = forward(256, 4, 5, 64, "bf16", 8, snerf=True)
    assert all(float(p.abs().max()) == 0.0 for k, p in st.sd.items() if k.startswith("beta_from_xyz"))
    got = F.decode(st.acts, st.n, 256, 4, 8)
    assert bool((got.code["e1"][:st.n] == 0).all())
    assert float((st.outs[3] - float(np.log(2.0))).abs().max()) <= 1e-6        # beta = softplus(0)
    check_case(st, label_of(st, " s-nerf"))


def stream_position(feat, tau, name, model):
    """The position in the packed forward stream of the largest hidden-block weight of ``name``."""
    from satnerf_amd import packing

    fm = packing.forward_maps(feat, tau)
    off, shp = fm["offsets"][name]
    idx = fm["idx"].astype(np.int64)
    inside = (idx >= off) & (idx < off + shp[0] * shp[1]) & ((idx - off) % shp[1] >= 3)
    pos = np.nonzero(inside)[0]
    w = model.flat_params().detach()[torch.from_numpy(idx[pos]).to(DEV)].abs()
    return int(pos[int(w.argmax())])


@pytest.mark.parametrize("mode,fmt", [("bf16", 8), ("bf16", 16)])
def test_a_flipped_weight_of_the_skip_layer_fails_at_a4(mode, fmt):
    """The checks notice what they are for: the sign bit of one bf16 element of the packed stream, in fc_net.8's part (data, not code:
    nothing faults).  (W) passes up to a3 and fails at a4; (S) fails at a4 only."""
    feat, tau = 256, 4
    model, _ = model_of(feat, tau)
    model.load_state_dict(params_of(feat, tau))
    at = stream_position(feat, tau, "fc_net.8.weight", model)

    def flip(hi, lo, l0):
        assert hi[at].item() != 0
        hi[at] ^= -32768

    st = forward(feat, tau, 5, 64, mode, fmt, tamper=flip)
    got = F.decode(st.acts, st.n, feat, tau, fmt)
    res = ratios_w(st, got)
    print(f"{label_of(st)} flipped (W): " + " ".join(f"{k} {r:.3f}" for k, r in res))
    assert F.first_failure([r for r in res if r[0] in F.CHAIN]) == "a4", res
    if fmt == 16:
        sg = F.gate_s(got, st.outs, st.sd, st.pts, feat, tau, mode, st.n)
        assert [k for k, _, bad in sg if bad] == ["a4"], sg
    check_case(forward(feat, tau, 5, 64, mode, fmt))      # and without the flip everything passes


def offset_bound_case(arena):
    """Width 256, tau 4, bf16, 8-bit workspaces: the largest n_points whose workspace stays below the generated stream's 32-bit offsets
    (ws_tiles act8_units 1024 < 2^32) and the first at the bound, which goes to the compiler-scheduled kernel.  The net is pointwise: the
    reference sees the first 4,096 points, the last 4,096 and the 4,096 around byte 2^31 only.  One side is freed before the other."""
    from satnerf_amd import ops, packing

    feat, tau, mode, fmt, span = 256, 4, "bf16", 8, 4096
    per = packing.act8_units(packing.aux_steps(tau), feat) * 1024
    wt_hi = (((1 << 32) + per - 1) // per + 7) // 8 * 8
    wt_lo = wt_hi - 8
    assert wt_lo * per < (1 << 32) <= wt_hi * per
    model, emb = model_of(feat, tau)
    model.load_state_dict(params_of(feat, tau))
    model.repack(mode, backward=True)
    hi, lo, l0 = model.packed(mode)
    sd = {k: p.detach().clone() for k, p in model.named_parameters()}
    for n in (32 * wt_lo, 32 * wt_lo + 1):
        assert W.ws_tiles(n) == (wt_lo if n == 32 * wt_lo else wt_hi)
        g = torch.Generator(device=DEV).manual_seed(n % 1000)
        rays = torch.cat([torch.rand(n, 3, device=DEV, generator=g) * 2 - 1, torch.nn.functional.normalize(torch.randn(n, 3, device=DEV, generator=g), dim=1),
                          torch.zeros(n, 1, device=DEV), torch.rand(n, 1, device=DEV, generator=g) * 0.5 + 0.5,
                          torch.nn.functional.normalize(torch.rand(n, 3, device=DEV, generator=g) + 0.2, dim=1)], 1)
        ts = torch.randint(0, 30, (n,), device=DEV, generator=g)
        z = rays[:, 7:8] * torch.rand(n, 1, device=DEV, generator=g)      # one sample per ray (ops.ray_sample wants two)
        acts = ops.acts_workspace(n, feat, DEV, fmt)
        outs = ops.satnerf_mlp(rays[:, 0:3], rays[:, 3:6], rays[:, 8:11], z, emb, ts, n, 1, feat, tau, mode, hi, lo, l0, acts=acts, fmt=fmt)
        torch.cuda.synchronize()
        a8 = acts.view(torch.uint8)
        mid = ((1 << 31) // per) * 32
        for name, p0 in (("first", 0), ("around byte 2^31", mid - span // 2), ("last", ((n - 1) // 32 + 1) * 32 - span)):
            p1 = min(p0 + span, n)
            pts = F.points(rays[p0:p1, 0:3], rays[p0:p1, 3:6], z[p0:p1], rays[p0:p1, 8:11], emb, ts[p0:p1], 1)
            st = types.SimpleNamespace(feat=feat, tau=tau, n=p1 - p0, s=1, mode=mode, fmt=fmt, sd=sd, pts=pts, outs=tuple(o[p0:p1] for o in outs),
                                       acts=W.gather_tiles(a8, per // 1024, range(p0 // 32, (p1 + 31) // 32)))
            check_case(st, f"w256 tau4 bf16 fmt8 {n} points ({'below' if n == 32 * wt_lo else 'at'} the 32-bit bound), {name} {p1 - p0}")
        del acts, a8, outs, rays, z, ts, st
        assert arena.canaries_intact()
        arena.bufs.clear()              # one side (4 GiB) is freed before the other is allocated
        torch.cuda.empty_cache()


def test_either_side_of_the_generated_streams_32_bit_offset_bound(arena):
    offset_bound_case(arena)


# ---------------------------------------------------------------------------------------------------------------- the V1 leg
def v1_leg():
    """Everything above that depends on the kernel, in a process started with SATNERF_FWD_V1=1."""
    from satnerf_amd import ops

    assert V1
    a = Arena()
    ops._ws_empty = a
    worst = {}
    for feat, tau, mode, fmt, n_rays, s in CASES:
        print(f"V1 next: w{feat} tau{tau} {mode} fmt{fmt} {n_rays}x{s}", flush=True)     # (a time limit's tail then names the case it stopped in)
        st = forward(feat, tau, n_rays, s, mode, fmt)
        w, sg = check_case(st)
        k = (feat, mode, fmt)
        worst[k] = (max(worst.get(k, (0, 0))[0], w or 0.0), max(worst.get(k, (0, 0))[1], sg or 0.0))
    for feat, mode, fmt in KERNELS:
        print(f"V1 next: (E) w{feat} {mode} fmt{fmt}", flush=True)
        miss = encoder_sweep(feat, 4, mode, fmt)
        print(f"V1 w{feat} {mode} fmt{fmt} (E): mismatching codes per swept stage: {miss}")
        assert all(v == 0 for v in miss.values()), miss
        for tau in (4, 16):
            res = aux_sweep(feat, tau, mode, fmt)
            print(f"V1 w{feat} tau{tau} {mode} fmt{fmt} (E) aux columns alone: (codes off, codes not equal, straddling share) {res}")
            assert all(bad == 0 and share <= 0.05 for bad, _, share in res.values()), res
        miss = encoder_sweep(feat, 16, mode, fmt, variant=1, layers=HEAD_LAYERS)
        assert all(v == 0 for v in miss.values()), miss
    assert a.canaries_intact()
    for k, (w, sg) in worst.items():
        print(f"V1 worst of w{k[0]} {k[1]} fmt{k[2]}: (W) {w:.3f} (S) {sg:.3f}")


V1_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from tests.test_hip_fwd_reference import v1_leg
v1_leg()
"""


def test_the_compiler_scheduled_kernels_pass_the_same_checks():
    """SATNERF_FWD_V1=1 is read once per process: one fresh child process runs every case of the matrix through (W), (S), (X)'s aux and
    lane checks and (E) with the compiler-scheduled satnerf_fwd_kernel.  The child takes about half a minute on an MI355X (measured: 21 s
    before the second (E) variant joined it); the limit of 600 s is there for a hang, not as a budget."""
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-c", V1_CHILD, ROOT], env=dict(os.environ, SATNERF_FWD_V1="1"),
                       capture_output=True, text=True, cwd=ROOT)
    print(r.stdout[-20000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
