"""High-precision reference of the training forward (sr_satnerf_mlp_fwd with an acts workspace: satnerf_fwd2_kernel<SAVE>, satnerf_fwd3_kernel,
satnerf_fwd512g_kernel and the compiler-scheduled satnerf_fwd_kernel), restated in float64 from models/satnerf.py semantics
(oracle.satnerf_oracle.satnerf_mlp).  Torch: the same code runs on the CPU (tests/test_fwd_reference_host.py pins it to the model and runs
a simulated kernel through its gates) and on the GPU (tests/test_hip_fwd_reference.py holds the kernels to it).

* Inputs: the model's state_dict in natural feature order and the per-point inputs the kernel reads (org, dir, z, sun, the embedding table,
  ts).  The packed forward stream and the fc_net.0 table are NOT read: they are inputs of the kernel under test, and packing.forward_maps /
  sr_pack_all are under test with it.
* Output: one vector per key.  Sin stages are in REVOLUTIONS (pre-activation / 2 pi, fc_net.0's factor 30 included): ``a0`` .. ``a7`` (the
  trunk), ``rgbh`` / ``s1`` / ``e1`` / ``s2`` / ``s3`` (the hidden layers of the colour, sun and uncertainty heads).  ``feats`` and the head
  pre-activations ``sigma_pre`` and ``head`` (albedo logits 0..2, sun logit 3, beta pre-softplus 4) are plain values; ``albedo``, ``sigma``,
  ``sun_v``, ``beta`` are the four outputs; ``aux`` is the vector [sun(3), 1, xyz(3), 0, t(tau) .., 0 ..] every stage's last k-step(s) read.
* Two evaluations of one chain (``chain``): exact (``mode`` None: float64 throughout) and rounded (the kernel's operand model of ``mode``).

  MODELLED: weights and biases R(float32(W) float32(c)) -- c = packing.INV_2PI for sin stages, 1 for identity and head rows, the product
  rounded once in fp32 as the packer does; the aux vector R(.); each stage's hand-off R(sin(2 pi frac)) resp. R(feats); fc_net.0 as the
  24-bit table product float32(W) float32(30 / 2 pi) on the fp32 sample position, at every mode.  R = bf16 RNE (``bf16``), fp16 RNE
  (``f16``), hi + lo = bf16(v) + bf16(v - hi), 16 significant bits (``bf16x3``).  Accumulation is float64.
  NOT MODELLED: the order and rounding of the fp32 accumulation, the hardware sine (v_sin_f32: taken to be within EPS_SIN of the true
  sine, the assumption wgrad_reference.py states), the lo x lo product the bf16x3 kernels leave out (<= 2^-18 |w| |x| per term), expf /
  log1pf of the output activations.
* One-stage mode (``stage``): from an interval around each input, M, the magnitude sum A and the operand ambiguity amb of ONE stage.
* The workspace encoders restated (``phase8``, ``unorm16``; MX8 is dx_reference.mx8_encode) and the decoder of an acts workspace into the
  chain's keys (``decode``).
* The gates of tests/test_hip_fwd_reference.py (``gate_w``, ``gate_s``, ``gate_lanes``), shared with the CPU simulation.

A plain helper module, imported by the tests (not a conftest)."""
import math
import types

import numpy as np
import torch

from satnerf_amd import packing

from . import dx_reference as X
from . import wgrad_reference as W
from .wgrad_reference import EPS_SIN   # 2^-19: wgrad_reference.py's stated ASSUMPTION about v_sin_f32, not a documented bound

SIN, ID, LIN = "sin", "id", "lin"
CHAIN = [f"a{l}" for l in range(8)] + ["feats", "rgbh", "s1", "e1", "s2", "s3"]      # the order the gates walk
OUTPUTS = ["albedo", "sigma", "sun_v", "beta"]
# (W) on the four outputs with q = 0 only if the CPU simulation's worst output ratio is <= 0.5.  It is not (tests/test_fwd_reference_host.py
# asserts that it exceeds 0.5: a hand-off whose bf16 rounding the fp32 sine flips moves an output by as much as the operand rounding
# itself), so the outputs are held by (S) and the golden tests and (W) prints their ratios only.
OUTPUTS_IN_W = False
TWO_PI = 2.0 * math.pi
Q8, Q16 = 1.0 / 512.0, 1.0 / 131070.0          # half steps of PHASE8 and unorm16, revolutions
# v_fract of a NEGATIVE pre-activation rounds: 1 - |x| for a small |x| needs more bits than fp32 has below 1, half an ulp of [0.5, 1) at the
# worst.  It is part of the unorm16 codec (v_cvt_pknorm_u16 of v_fract) and stands beside the half step in the per-element gate (S);
# tests/test_fwd_reference_host.py shows that an exact simulation does not meet the gate without it.
FRACT16 = 2.0 ** -25
DELTA16 = TWO_PI / 131070.0 + EPS_SIN          # what a saved unorm16 phase leaves open of the next stage's operand sin(2 pi x)
L0_STEPS = 4   # fc_net.0's fp32 error in units of 2^-24 A: three fma roundings (compiler-scheduled kernel), or two k-steps of exact bf16 x bf16 products plus the dropped cross terms m l + l m + l l <= 2^-23 |w x| of the three-way split (generated kernels)


# ---------------------------------------------------------------------------------------------------------------- the network
def steps(feat, tau):
    """Every stage after fc_net.0 in chain order: (key, kind, layer, input key, hidden columns of the weight, [(aux name, weight columns)],
    MFMA k-steps of one output, the aux k-step(s) included)."""
    ks, hs, auxs = feat // 16, feat // 32, packing.aux_steps(tau)
    al, hid = slice(None), slice(0, feat)
    out = [(f"a{l}", SIN, f"fc_net.{2 * l}", f"a{l - 1}", slice(3, None) if l == 4 else al, [("xyz", slice(0, 3))] if l == 4 else [], ks + auxs)
           for l in range(1, 8)]
    out += [("feats", ID, "feats_from_xyz", "a7", al, [], ks + auxs),
            ("sigma_pre", LIN, "sigma_from_xyz.0", "a7", al, [], ks + auxs),
            ("rgbh", SIN, "rgb_from_xyzdir.0", "feats", hid, [], ks + auxs),
            ("s1", SIN, "sun_v_net.0", "feats", hid, [("sun", slice(feat, feat + 3))], ks + auxs),
            ("e1", SIN, "beta_from_xyz.0", "feats", hid, [("t", slice(feat, feat + tau))], ks + auxs),
            ("s2", SIN, "sun_v_net.2", "s1", al, [], hs + auxs),
            ("s3", SIN, "sun_v_net.4", "s2", al, [], hs + auxs),
            ("h_rgb", LIN, "rgb_from_xyzdir.2", "rgbh", al, [], hs + auxs),
            ("h_sun", LIN, "sun_v_net.6", "s3", al, [], hs + auxs),
            ("h_beta", LIN, "beta_from_xyz.2", "e1", al, [], hs + auxs)]
    return out


def downstream(key):
    """The keys of CHAIN whose input depends on stage ``key``."""
    after = {"feats": ["rgbh", "s1", "e1", "s2", "s3"], "s1": ["s2", "s3"], "s2": ["s3"]}
    if key in after:
        return after[key]
    return CHAIN[CHAIN.index(key) + 1:] if key[0] == "a" else []


LAYERS = ["fc_net.0"] + [s[2] for s in steps(256, 4)]
SIN_LAYERS = {s[2] for s in steps(256, 4) if s[1] == SIN}


def rounder(mode):
    """R of the operand model: float64 -> float64 (through fp32, as the kernels round an fp32 value)."""
    if mode is None:
        return lambda v: v
    if mode == "bf16":
        return lambda v: v.float().to(torch.bfloat16).to(torch.float64)
    if mode == "f16":
        return lambda v: v.float().to(torch.float16).to(torch.float64)
    assert mode == "bf16x3"

    def r(v):
        v = v.float()
        hi = v.to(torch.bfloat16).float()
        return hi.to(torch.float64) + (v - hi).to(torch.bfloat16).to(torch.float64)
    return r


def operands(sd, mode, device=None, no_c=()):
    """{layer: (W float64 [out, in], b float64 [out])} as the kernel multiplies them (``mode`` None: exact).  ``no_c``: layers packed without
    their factor c (a planted fault of the CPU simulation)."""
    R = rounder(mode)
    out = {}
    for name in LAYERS:
        w, b = sd[name + ".weight"].detach(), sd[name + ".bias"].detach()
        if device is not None:
            w, b = w.to(device), b.to(device)
        if mode is None:
            c = 30.0 / TWO_PI if name == "fc_net.0" else 1.0 / TWO_PI if name in SIN_LAYERS and name not in no_c else 1.0
            out[name] = (w.to(torch.float64) * c, b.to(torch.float64) * c)
            continue
        if name == "fc_net.0":      # the fp32 table (sr_gather_scale_f32): one fp32 product, no operand rounding
            c = torch.tensor(float(np.float32(packing.W0_FIRST) * packing.INV_2PI), dtype=torch.float32, device=w.device)
            out[name] = ((w.float() * c).to(torch.float64), (b.float() * c).to(torch.float64))
            continue
        c = torch.tensor(float(packing.INV_2PI) if name in SIN_LAYERS and name not in no_c else 1.0, dtype=torch.float32, device=w.device)
        out[name] = (R((w.float() * c).to(torch.float64)), R((b.float() * c).to(torch.float64)))
    return out


def points(org, direction, z, sun, temb, ts, n_samples):
    """The per-point inputs as the kernel forms them (point p belongs to ray p // n_samples): xyz = org + z dir in fp32, unfused (the
    kernel's contract(off) block) and fused (``xyz_fma``: what X accepts as well), sun, t = temb[ts[ray]]; float64 copies of fp32 values."""
    z = z.reshape(-1).float()
    ray = torch.arange(z.numel(), device=z.device) // n_samples
    o, d = org.float()[ray], direction.float()[ray]
    xyz = o + d * z[:, None]
    fma = (o.to(torch.float64) + d.to(torch.float64) * z[:, None].to(torch.float64)).float()
    t = temb.float()[ts[ray]] if ts is not None else temb.float()[ray]
    return types.SimpleNamespace(xyz=xyz.to(torch.float64), xyz_fma=fma.to(torch.float64), sun=sun.float()[ray].to(torch.float64), t=t.to(torch.float64))


def aux_vector(pts, tau, xyz=None):
    """[P, 16 aux_steps(tau)]: slots [sun(3), 1, xyz(3), 0 | t(0..tau) .., 0 ..]."""
    xyz = pts.xyz if xyz is None else xyz
    one = torch.ones_like(xyz[:, :1])
    pad = torch.zeros(xyz.shape[0], 16 * packing.aux_steps(tau) - 8 - tau, dtype=xyz.dtype, device=xyz.device)
    return torch.cat([pts.sun, one, xyz, 0 * one, pts.t, pad], 1)


def sin_rev(x):
    return torch.sin(TWO_PI * (x - torch.floor(x)))


def activations(pre_sigma, head):
    """The four outputs from the head pre-activations (rgb_padding = 0.001)."""
    sp = torch.nn.functional.softplus
    return dict(albedo=torch.sigmoid(head[:, 0:3]) * 1.002 - 0.001, sigma=sp(pre_sigma[:, 0]), sun_v=torch.sigmoid(head[:, 3]), beta=sp(head[:, 4]))


def chain(sd, pts, feat, tau, mode=None, no_c=()):
    """The whole forward -> {key: [P, n]} (module header); ``mode`` None = exact, else the operand model of that mode."""
    ops = operands(sd, mode, pts.xyz.device, no_c)
    R = rounder(mode)
    aux = {"xyz": R(pts.xyz), "sun": R(pts.sun), "t": R(pts.t)}
    w0, b0 = ops["fc_net.0"]
    M = {"a0": pts.xyz @ w0.T + b0}
    hand = {"a0": R(sin_rev(M["a0"]))}
    for key, kind, name, src, cols, auxs, _ in steps(feat, tau):
        w, b = ops[name]
        v = hand[src] @ w[:, cols].T + b
        for a, acols in auxs:
            v = v + aux[a] @ w[:, acols].T
        M[key] = v
        if kind != LIN:
            hand[key] = R(sin_rev(v)) if kind == SIN else R(v)
    M["head"] = torch.cat([M.pop("h_rgb"), M.pop("h_sun"), M.pop("h_beta")], 1)
    M.update(activations(M["sigma_pre"], M["head"]))
    M["aux"] = R(aux_vector(pts, tau))
    return M


def stage(step, ops, lo, hi, aux):
    """One stage from the interval [lo, hi] of each hidden input and the (rounded) aux inputs: M = W (lo + hi) / 2 + aux terms + b,
    A = |W| |mid| + |aux terms| + |b|, amb = |W| (hi - lo) / 2; [P, n_out]."""
    _, _, name, _, cols, auxs, _ = step
    w, b = ops[name]
    mid, rad = (lo + hi) / 2, (hi - lo) / 2
    wh = w[:, cols]
    M = mid @ wh.T + b
    A = mid.abs() @ wh.abs().T + b.abs()
    for a, acols in auxs:
        M = M + aux[a] @ w[:, acols].T
        A = A + aux[a].abs() @ w[:, acols].abs().T
    return M, A, rad @ wh.abs().T


AUX_STAGES = {"fc_net.8": slice(3, None), "sun_v_net.0": None, "beta_from_xyz.0": None}      # layer -> its hidden columns (None: the first ``feat``)


def aux_only(step, sd, pts, feat, tau, mode, fmt):
    """(E), second variant: stage ``step`` with its hidden block zero, the aux columns and the bias as they are.  The pre-activation is a
    sum of <= 1 + 24 exact products of 16-bit operands per pass (bf16x3: hi hi + lo hi + hi lo, the lo lo products the kernel leaves out
    taken off here) -> (S float64, the codes of S - e, S, S + e with e = aux k-steps x n_pass x 2^-24 A, + FRACT16 in the 16-bit format)."""
    R = rounder(mode)
    w, b = operands(sd, mode, pts.xyz.device)[step[2]]
    M, A = b.expand(pts.xyz.shape[0], -1).clone(), b.abs().expand(pts.xyz.shape[0], -1).clone()
    bf = lambda v: v.float().to(torch.bfloat16).to(torch.float64)  # noqa: E731
    for a, cols in step[5]:
        x, wa = R(getattr(pts, a)), w[:, cols]
        M = M + x @ wa.T
        A = A + x.abs() @ wa.abs().T
        if mode == "bf16x3":
            M = M - (x - bf(x)) @ (wa - bf(wa)).T
    e = packing.aux_steps(tau) * (3 if mode == "bf16x3" else 1) * 2.0 ** -24 * A + (FRACT16 if fmt == 16 else 0.0)      # (unorm16: v_fract rounds)
    enc = (lambda v: phase8(v)) if fmt == 8 else (lambda v: torch.round((v - torch.floor(v)) * 65535.0).to(torch.int64))
    return M, enc(M - e), enc(M), enc(M + e)


# ---------------------------------------------------------------------------------------------------------------- encoders, decoder
def phase8(x, truncate=False):
    """codec8.h restated: u = RNE(x 256) mod 256 -- what x + 49152.0f leaves in the low mantissa byte.  x float32 -> int64.
    (``truncate``: the planted fault, floor in place of RNE.)"""
    s = x.to(torch.float64) * 256.0
    return (torch.floor(s) if truncate else torch.round(s)).to(torch.int64) & 0xff        # torch.round: half to even


def unorm16(x):
    """u = RNE(frac(x) 65535), as v_cvt_pknorm_u16 of v_fract gives (v_fract: x - floor(x) in fp32, below 1)."""
    x = x.float()
    f = torch.clamp(x - torch.floor(x), max=float.fromhex("0x1.fffffep-1"))
    return torch.round(f.to(torch.float64) * 65535.0).to(torch.int64)


def bf16_half_ulp(v):
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 8.0)


def ulp32(v):
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 23.0)


def to_lanes(nat):
    """[P, n] natural order -> [P, n / 32, 2, 16]: the 16 values MX8 lane (p, h) of double fragment t holds (dx_reference.lanes)."""
    P, n = nat.shape
    s2f = torch.from_numpy(packing.slot_to_feat(np.arange(n))).to(nat.device)
    return nat[:, s2f].view(P, n // 32, 2, 2, 8).permute(0, 1, 3, 2, 4).reshape(P, n // 32, 2, 16)


def from_lanes(lan):
    """Inverse of to_lanes."""
    P, t = lan.shape[:2]
    n = 32 * t
    slot = lan.view(P, t, 2, 2, 8).permute(0, 1, 3, 2, 4).reshape(P, n)
    inv = torch.from_numpy(packing.feat_to_slot(n)).to(lan.device)
    return slot[:, inv]


def decode(acts, n_points, feat, tau, fmt):
    """An acts workspace -> what the forward saved, over the whole tiles a kernel reads (rows >= n_points: the last tile's padding):
    ``rev`` {sin key: revolutions}, ``code`` {sin key: the stored integers}, ``feats`` / ``feats_q`` (value and half step), ``lanes``
    (MX8 codes [P, tiles, 2, 16], E [P, tiles, 2]) or None, ``aux`` [P, 16 auxs] (the stored bf16 values)."""
    geo = X.geometry(feat, tau)
    dk = packing.dpre8_units(feat) if fmt == 8 else 9 * geo["KS"] + 1 + 5 * geo["HS"] + 1
    dummy = torch.zeros(W.ws_tiles(n_points) * dk * 1024 + 4096, dtype=torch.uint8, device=acts.device)     # (no dpre workspace here)
    _, cols, _ = W.decode_workspaces(dummy, acts, n_points, feat, tau, fmt)
    out = types.SimpleNamespace(fmt=fmt, n=n_points)
    out.rev = X.phases_from_acts(cols, geo)
    out.code = {k: X._natural(cols, f0, n, lambda op: op.u) for k, (f0, n) in geo["act"].items()}
    f0 = geo["auxs"] + 8 * geo["KS"]
    out.feats = X._natural(cols, f0, feat, lambda op: op.exact())
    out.aux = torch.cat([cols[("aux", a)].val for a in range(geo["auxs"])], 1)
    if fmt == 8:
        out.feats_q = X._natural(cols, f0, feat, X.half_step)
        out.lanes = X.lanes(cols, {"dp": {"feats": (f0, feat)}}, "feats")
    else:
        out.feats_q, out.lanes = None, None
    return out


# ---------------------------------------------------------------------------------------------------------------- gates
def wrap(d):
    """The circular difference in revolutions."""
    return d - torch.round(d)


def gate_w(got, outs, rounded, exact, n):
    """(W) the whole chain under the operand model, per column (one feature of one key over the points < n), in chain order:
    |wrap(got - M_rounded)|_2 <= |q|_2 + |wrap(M_rounded - M_exact)|_2.  q = the codec's half step: 1/512 (PHASE8), 1/131070 (unorm16),
    2^(E - 134) of the lane's stored scale byte (MX8 feats), half a bf16 ulp of M_rounded (bf16 feats); 0 for the four outputs (``outs``
    None: left out).  -> [(key, worst ratio over the key's columns)]."""
    res = []

    def ratio(err, bound):
        ok = err <= bound
        return float(torch.where(ok & (bound == 0), torch.zeros_like(err), err / bound.clamp_min(1e-300)).max())

    for key in CHAIN:
        mr, me = rounded[key][:n], exact[key][:n]
        if key == "feats":
            d, noise = got.feats[:n] - mr, mr - me
            q = got.feats_q[:n] if got.fmt == 8 else bf16_half_ulp(mr)
        else:
            d, noise = wrap(got.rev[key][:n] - mr), wrap(mr - me)
            q = torch.full_like(mr, Q8 if got.fmt == 8 else Q16)
        res.append((key, ratio(d.norm(dim=0), q.norm(dim=0) + noise.norm(dim=0))))
    if outs is not None:
        for key, o in zip(OUTPUTS, outs):
            o = o.to(torch.float64).reshape(n, -1)
            mr, me = rounded[key].reshape(n, -1), exact[key].reshape(n, -1)
            res.append((key, ratio((o - mr).norm(dim=0), (mr - me).norm(dim=0))))
    return res


def gate_s(got, outs, sd, pts, feat, tau, mode, n, no_c=(), literal=False):
    """(S) every stage from the DECODED stage above (16-bit workspaces), per element:
    |wrap(got - M)| <= q + k_steps n_pass 2^-24 A + amb   (q = Q16 + FRACT16; bf16 feats: half a bf16 ulp of M in place of q; fc_net.0: L0_STEPS, no n_pass).
    (Half a bf16 ulp is 2^(floor(log2 |M|) - 8), between 2^-9 |M| and 2^-8 |M|: bf16 keeps 8 significant bits, so 2^-9 |M| for every M
    is not met by a correct round-to-nearest-even.  ``literal``: q = Q16 alone and 2^-9 |M| for bf16 feats, the two bounds
    tests/test_fwd_reference_host.py shows an exact simulation to miss.)
    The operand of the next stage is sin(2 pi x) of a phase x within 1/131070 of the saved one, evaluated by a sine within EPS_SIN:
    the interval sin(2 pi saved) +- DELTA16, rounded at both ends.  Saved bf16 feats ARE the operand in ``bf16``; in ``f16`` / ``bf16x3`` the
    operand is a finer rounding of a value within half a bf16 ulp of the saved one.  The outputs: |got - f(M)| <= max|f'| (gate of the
    logit) + 4 fp32 ulps of f(M).  -> [(key, worst ratio, elements over the gate)] in chain order."""
    assert got.fmt == 16
    ops = operands(sd, mode, pts.xyz.device, no_c)
    R = rounder(mode)
    n_pass = 3 if mode == "bf16x3" else 1
    aux = {"xyz": R(pts.xyz), "sun": R(pts.sun), "t": R(pts.t)}
    iv = {}
    for key in got.rev:
        v = sin_rev(got.rev[key][:n])
        iv[key] = (R(v - DELTA16), R(v + DELTA16))
    f = got.feats[:n]
    h = torch.zeros_like(f) if mode == "bf16" else bf16_half_ulp(f)
    iv["feats"] = (R(f - h), R(f + h))
    res = []

    def note(key, err, gate):
        bad = err > gate
        res.append((key, float(torch.where(gate > 0, err / gate.clamp_min(1e-300), err * 1e300).max()), int(bad.sum())))

    w0, b0 = ops["fc_net.0"]
    M = pts.xyz @ w0.T + b0
    A = pts.xyz.abs() @ w0.abs().T + b0.abs()
    q16 = Q16 if literal else Q16 + FRACT16
    note("a0", wrap(got.rev["a0"][:n] - M).abs(), q16 + L0_STEPS * 2.0 ** -24 * A)
    logit = {}
    for st in steps(feat, tau):
        key, kind, _, src, _, _, k = st
        M, A, amb = stage(st, ops, iv[src][0], iv[src][1], aux)
        arith = k * n_pass * 2.0 ** -24 * A + amb
        if kind == SIN:
            note(key, wrap(got.rev[key][:n] - M).abs(), q16 + arith)
        elif kind == ID:
            note(key, (got.feats[:n] - M).abs(), (2.0 ** -9 * M.abs() if literal else bf16_half_ulp(M)) + arith)
        else:
            logit[key] = (M, arith)
    if outs is not None:
        hm = torch.cat([logit[k][0] for k in ("h_rgb", "h_sun", "h_beta")], 1)
        hg = torch.cat([logit[k][1] for k in ("h_rgb", "h_sun", "h_beta")], 1)
        want = activations(logit["sigma_pre"][0], hm)
        slope = dict(albedo=0.25 * 1.002, sigma=1.0, sun_v=0.25, beta=1.0)       # max |f'| of sigmoid (with the rgb padding) and softplus
        lg = dict(albedo=hg[:, 0:3], sigma=logit["sigma_pre"][1][:, 0], sun_v=hg[:, 3], beta=hg[:, 4])
        for key, o in zip(OUTPUTS, outs):
            note(key, (o.to(torch.float64) - want[key]).abs(), slope[key] * lg[key] + 4 * ulp32(want[key]))
    return res


def gate_lanes(got, n, zero_ok=False):
    """(X) every MX8 feats lane of a valid point: codes in 1 .. 255, 63 <= max |u - 128| <= 127 (the scale is the smallest that holds the
    lane's maximum), no exponent at the clamp.  -> list of problems (empty = fine)."""
    u, e = got.lanes
    u, e = u[:n], e[:n]
    big = (u - 128).abs().amax(-1)
    bad = []
    if int(u.min()) < 1 or int(u.max()) > 255:
        bad.append(("code outside 1..255", int(u.min()), int(u.max())))
    if int(big.min()) < 63 or int(big.max()) > 127:
        bad.append(("max |u - 128| outside 63..127", int(big.min()), int(big.max())))
    if not zero_ok and int(e.min()) <= 6:
        bad.append(("exponent at the clamp", int(e.min())))
    return bad


def first_failure(ratios):
    """The first key of a gate's result (chain order) over its bound, or None."""
    return next((r[0] for r in ratios if r[1] > 1.0), None)


# ---------------------------------------------------------------------------------------------------------------- (E) bias patterns
def _invert(t, c, R):
    """A float32 bias b with R(float32(b) float32(c)) == t where one exists within 8 fp32 steps of t / c -> (b, landed): ``landed`` is
    what the pattern really puts into the accumulator, R(b c) as float64."""
    c = torch.tensor(float(c), dtype=torch.float32)
    b = (t / float(c)).float()
    best, hit = b.clone(), torch.zeros_like(b, dtype=torch.bool)
    for k in [0] + [s * j for j in range(1, 9) for s in (1, -1)]:
        cand = torch.where(b == 0, b, (b.view(torch.int32) + k).view(torch.float32))
        ok = (R((cand * c).to(torch.float64)) == t) & ~hit
        best = torch.where(ok, cand, best)
        hit |= ok
    return best, R((best * c).to(torch.float64)), hit


def bias_pattern(layer, n, mode, seed=0):
    """(E): the bias of the swept stage ``layer`` (n features; its 2-D weight is all zero, so the accumulator is R(b c) x 1.0 exactly) ->
    (b float32 [n], landed float64 [n], n_special).  The first n_special features hold the chosen targets that ``mode``'s operand format
    can represent (``bf16x3``: near misses of most, see below) -- codes 0, 1, 127, 128, 255, exact ties (k + 1/2) / 256 for even and odd k, values that round up to 256 = 0, negative
    pre-activations, |pre| >= 1 up to 16 revolutions (fc_net.0: 64), +-0 --, the rest seeded random values.  feats_from_xyz: MX8 lanes
    with one large and fifteen tiny values, an all-zero lane, a maximum whose (1 + 2^-7) crosses a power of two, a scaled maximum of
    exactly 127.  Head rows: a few plain values (sigma: one past softplus's threshold 20 in the second variant ``seed`` 1)."""
    g = torch.Generator().manual_seed(1000 + seed)
    first = layer == "fc_net.0"
    R = (lambda v: v.float().to(torch.float64)) if first else rounder(mode)
    if layer in SIN_LAYERS or first:
        c = float(np.float32(packing.W0_FIRST) * packing.INV_2PI) if first else float(packing.INV_2PI)
        t = [k / 256 for k in (0, 1, 127, 128, 255)] + [(k + 0.5) / 256 for k in (2, 3, 126, 127)] + [255.75 / 256, -1 / 1024, -1 / 512]
        t += [-k / 256 for k in (1, 127, 128, 255)] + [-(k + 0.5) / 256 for k in (2, 3)]
        t += [1.0, -1.0, 1 + 1 / 128, 1 + 3 / 256, 3.5, -7.25, 15.9375, -16.0, 16.0, 2.5 / 256 + 8]
        if first:
            t += [31.5, -63.984375, 64.0, 40 + 2.5 / 256]
        t = torch.tensor(t, dtype=torch.float64)
        t = t[R(t) == t]
        b, landed, hit = _invert(t, c, R)      # (no hit: the nearest bias, a near miss of the target -- bf16x3 keeps hi + lo of ANY fp32 product, so it lands on a target only where the fp32 product itself does)
        zeros = torch.tensor([0.0, -0.0])
        rnd = ((torch.rand(n - len(b) - 2, generator=g, dtype=torch.float64) * 4 - 2) / c).float()
        b = torch.cat([b, zeros, rnd])
        return b, R((b * torch.tensor(c, dtype=torch.float32)).to(torch.float64)), len(t) + 2
    if layer == "feats_from_xyz":
        lan = torch.randn(n // 32, 2, 16, generator=g, dtype=torch.float64) * torch.exp2(torch.randint(-12, 3, (n // 32, 2, 1), generator=g).double())
        lan[0, 0] = torch.tensor([1.0] + [2.0 ** -12] * 15)                 # one large, fifteen tiny
        lan[0, 1] = 0.0                                                    # the zero lane: code 128, E at the clamp 6
        lan[1, 0] = torch.tensor([-(2.0 - 2.0 ** -7)] + [0.1] * 15)        # max (1 + 2^-7) crosses the binade
        lan[1, 1] = torch.tensor([127.0 / 64] + [-0.5] * 15)               # scaled maximum exactly 127
        lan[2, 0] = torch.tensor([2.0 ** -12] * 15 + [-3.0])
        b = from_lanes(R(lan)[None])[0].float()
        return b, R(b.to(torch.float64)), 5 * 16
    vals = {"sigma_from_xyz.0": [[1.25], [25.0]], "rgb_from_xyzdir.2": [[-3.0, 0.0, 2.5], [0.375, -0.0, 9.0]], "sun_v_net.6": [[-0.75], [6.5]],
            "beta_from_xyz.2": [[0.375], [-4.0]]}[layer][seed % 2]
    b = torch.tensor(vals, dtype=torch.float32)
    return b, R(b.to(torch.float64)), len(vals)


def pattern_classes(landed, b):
    """Which of the required cases a sin stage's pattern really holds (asserted on the host before anything runs)."""
    x = landed
    u = phase8(x.float())
    s = x * 256.0
    tie = (s - torch.floor(s)) == 0.5
    fl = torch.floor(s).to(torch.int64)
    f = x - torch.floor(x)
    return dict(codes={k for k in (0, 1, 127, 128, 255) if bool((u == k).any())}, tie_even=bool((tie & (fl % 2 == 0)).any()),
                tie_odd=bool((tie & (fl % 2 == 1)).any()), wraps=bool(((f * 256.0 > 255.5) & (u == 0)).any()), negative=bool((x < 0).any()),
                biggest=float(x.abs().max()), plus_zero=bool(((b == 0) & ~torch.signbit(b)).any()), minus_zero=bool(((b == 0) & torch.signbit(b)).any()))
