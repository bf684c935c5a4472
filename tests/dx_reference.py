"""High-precision reference of the dX chain (sr_satnerf_mlp_bwd: csrc/mlp_bwd.inc and the generated trunks), restated in float64 from
models/satnerf.py semantics -- the transpose of oracle.satnerf_oracle.satnerf_mlp, layer by layer.  Torch: the same code runs on the CPU
(tests/test_dx_reference_host.py pins it to autograd) and on the GPU (tests/test_hip_dx_reference.py holds the kernel to it).

* Inputs: the model's state_dict in natural feature order, the saved phases of every sin stage (decoded from the acts workspace by
  wgrad_reference.decode_workspaces), the four outputs and their gradients (each may be None).  The transposed weight stream is NOT
  read: it is an input of the kernel under test, and the packer that builds it is under test with it.
* Two evaluations of one chain: ``exact`` (float64 throughout) and ``rounded`` (the kernel's operand model: weights bf16(W) -- the stream
  holds the high half only, scale 1 --, the vector handed from one stage to the next rounded to bf16, accumulation float64).
* One-stage mode (``stage``): from the decoded output of the stage above, this stage's M = (W^T d_in) cos and A = (|W|^T |d_in|) |cos|.
* MX8 helpers: the half step of a decoded lane and a restatement of the encoder (codec8.h).

Names.  A vector of the chain is known by a key: ``head`` (the five head rows: albedo 0..2, sun 3, beta 4), ``sigma`` (d sigma_pre),
``rgbh`` / ``s3`` / ``e1`` / ``s2`` / ``s1`` (the hidden layers of the colour, sun and uncertainty heads), ``feats``, ``dt`` and
``pre7`` .. ``pre0`` (the trunk; ``pre0`` is the gradient with respect to the ARGUMENT of fc_net.0's sine: the factor 30 lives in the gather
scale of its weight gradient, not in dpre).  Phases are known by ``a0`` .. ``a7`` and the hidden layers' keys.  Stages in chain order:
bH, bS3, bS2, bG2, bDT, bG1, bL7 .. bL1 (bL4 multiplies by columns 3: of fc_net.8.weight, the skip layer).

A plain helper module, imported by the tests (not a conftest)."""
import math

import torch

from satnerf_amd import packing

# The cos accuracy below is an assumption, not a documented bound: the CDNA ISA guides give no error bound for v_cos_f32.  It is the same
# assumption wgrad_reference.py makes about v_sin_f32 (within 2^-19 of the true value): a hardware cos further from the true value than
# assumed would show in tests/test_hip_dx_reference.py as a gate failure, not pass unnoticed.
EPS_COS = 2.0 ** -19
STAGES = ["bH", "bS3", "bS2", "bG2", "bDT", "bG1"] + [f"bL{l}" for l in range(7, 0, -1)]


def geometry(feat, tau):
    """Fragment offsets of both workspaces, as packing.backward_maps numbers them (activation fragments include the aux offset)."""
    auxs = packing.aux_steps(tau)
    KS, HS = feat // 16, feat // 32
    A = auxs
    ACT_FEATS = A + 8 * KS
    ACT_RGBH, ACT_S1, ACT_E1, ACT_S2, ACT_S3 = (ACT_FEATS + KS + k * HS for k in range(5))
    DP_FEATS, DP_SIGMA = 8 * KS, 9 * KS
    DP_RGBH = DP_SIGMA + 1
    DP_S1, DP_E1, DP_S2, DP_S3, DP_HEAD = (DP_RGBH + k * HS for k in range(1, 6))
    half = feat // 2
    dp = {f"pre{l}": (KS * l, feat) for l in range(8)}
    dp.update(feats=(DP_FEATS, feat), sigma=(DP_SIGMA, 16), rgbh=(DP_RGBH, half), s1=(DP_S1, half), e1=(DP_E1, half), s2=(DP_S2, half),
              s3=(DP_S3, half), head=(DP_HEAD, 16))
    act = {f"a{l}": (A + KS * l, feat) for l in range(8)}
    act.update(rgbh=(ACT_RGBH, half), s1=(ACT_S1, half), e1=(ACT_E1, half), s2=(ACT_S2, half), s3=(ACT_S3, half))
    return dict(feat=feat, half=half, tau=tau, auxs=auxs, KS=KS, HS=HS, dp=dp, act=act, live={"head": 5, "sigma": 1})


def steps(feat, tau):
    """The chain as a list of (stage, output key, phase key or None, MFMA k-steps of one output, terms); a term (input key, input columns,
    weight name, weight columns) contributes d_in[:, input columns] @ W[name][:, weight columns]."""
    KS, HS = feat // 16, feat // 32
    al = slice(None)
    out = [("bH", "rgbh", "rgbh", 1, [("head", slice(0, 3), "rgb_from_xyzdir.2.weight", al)]),
           ("bH", "s3", "s3", 1, [("head", slice(3, 4), "sun_v_net.6.weight", al)]),
           ("bH", "e1", "e1", 1, [("head", slice(4, 5), "beta_from_xyz.2.weight", al)]),
           ("bS3", "s2", "s2", HS, [("s3", al, "sun_v_net.4.weight", al)]),
           ("bS2", "s1", "s1", HS, [("s2", al, "sun_v_net.2.weight", al)]),
           ("bG2", "feats", None, 3 * HS, [("rgbh", al, "rgb_from_xyzdir.0.weight", slice(0, feat)), ("s1", al, "sun_v_net.0.weight", slice(0, feat)),
                                           ("e1", al, "beta_from_xyz.0.weight", slice(0, feat))]),
           ("bDT", "dt", None, HS, [("e1", al, "beta_from_xyz.0.weight", slice(feat, feat + tau))]),
           ("bG1", "pre7", "a7", KS + 1, [("feats", al, "feats_from_xyz.weight", al), ("sigma", slice(0, 1), "sigma_from_xyz.0.weight", al)])]
    for l in range(7, 0, -1):
        out.append((f"bL{l}", f"pre{l - 1}", f"a{l - 1}", KS, [(f"pre{l}", al, f"fc_net.{2 * l}.weight", slice(3, None) if l == 4 else al)]))
    return out


def bf16(v):
    return v.to(torch.bfloat16).to(torch.float64)


def weights(state_dict, rounded, device=None):
    """float64 copies of the 2-D weights the chain multiplies by; ``rounded``: bf16(W), what model.packed_backward() packs."""
    names = {t[2] for s in steps(256, 4) for t in s[4]}
    out = {}
    for k in names:
        w = state_dict[k].detach()
        w = w.to(device) if device is not None else w
        out[k] = bf16(w.float()) if rounded else w.to(torch.float64)
    return out


# ---------------------------------------------------------------------------------------------------------------- workspaces -> vectors
def _natural(ops, f0, n, fn):
    """Fragments f0 .. of a slot space of n slots -> [P, n] in natural feature order (packing.feat_to_slot)."""
    x = torch.cat([fn(ops[f0 + i]) for i in range(n // 16)], 1)
    inv = packing.feat_to_slot(max(n, 32))[:n]
    return x[:, torch.from_numpy(inv).to(x.device)]


def decoded_vectors(rows, geo, fn=None):
    """{key: [P, n]} of every dpre vector in natural order; ``fn`` maps an Operand to [P, 16] (default: its decoded value)."""
    fn = fn or (lambda op: op.exact())
    out = {}
    for k, (f0, n) in geo["dp"].items():
        v = _natural(rows, f0, n, fn)
        out[k] = v[:, :geo["live"][k]] if k in geo["live"] else v
    return out


def half_step(op):
    """q = 2^(E - 134) per element: half the step of the lane's MX8 scale, read from the stored scale byte; 0 for the bf16 rows."""
    if op.codec == "mx":
        return torch.exp2(op.e.to(torch.float64) - 134.0)
    return torch.zeros_like(op.val)


def phases_from_acts(cols, geo):
    """{phase key: [P, n] revolutions, natural order} of every sin stage the forward saved."""
    return {k: _natural(cols, f0, n, lambda op: op.revolutions()) for k, (f0, n) in geo["act"].items()}


# ---------------------------------------------------------------------------------------------------------------- the chain
def head_grads(outs, grads):
    """Gradients of the head pre-activations: ([P, 5] albedo logits 0..2, sun logit 3, beta pre-softplus 4; [P, 1] sigma pre-softplus).
    sigmoid' from the output (the albedo's through the rgb_padding affine), softplus' = 1 - exp(-softplus)."""
    albedo, sigma, sun_v, beta = (x.detach().to(torch.float64) for x in outs)
    g_albedo, g_sigma, g_sun, g_beta = (None if g is None else g.detach().to(torch.float64) for g in grads)
    z = torch.zeros_like(sigma)
    s = (albedo + 0.001) / 1.002
    d_alb = torch.zeros_like(albedo) if g_albedo is None else g_albedo * 1.002 * s * (1.0 - s)
    d_sun = z if g_sun is None else g_sun * sun_v * (1.0 - sun_v)
    d_sig = z if g_sigma is None else g_sigma * (1.0 - torch.exp(-sigma))
    d_beta = z if g_beta is None else g_beta * (1.0 - torch.exp(-beta))
    return torch.cat([d_alb, d_sun[:, None], d_beta[:, None]], 1), d_sig[:, None]


def stage(step, d_in, wts, phases):
    """One stage from given inputs: M = (W^T d_in) cos(2 pi phase), A = (|W|^T |d_in|) |cos| (identity stages: cos = 1); [P, n_out]."""
    _, _, ph, _, terms = step
    M = A = 0.0
    for key, icols, name, wcols in terms:
        x, w = d_in[key][:, icols], wts[name][:, wcols]
        M = M + x @ w
        A = A + x.abs() @ w.abs()
    if ph is not None:
        c = torch.cos(2.0 * math.pi * phases[ph])
        M, A = M * c, A * c.abs()
    return M, A


def chain(state_dict, phases, outs, grads, feat, tau, rounded, want_abs=False):
    """The whole chain -> {key: [P, n]} of every vector the kernel writes, BEFORE the bf16 hand-off to the next stage (what the MX8 copy
    encodes); ``head`` and ``sigma`` are the handed values themselves (the kernel keeps those rows as bf16 in both formats).
    ``want_abs``: also each stage's magnitude sum A (``stage``; |value| for the head rows)."""
    wts = weights(state_dict, rounded, outs[0].device)
    hand = bf16 if rounded else (lambda v: v)
    d_head, d_sig = head_grads(outs, grads)
    M = {"head": hand(d_head), "sigma": hand(d_sig)}
    A = {k: v.abs() for k, v in M.items()}
    handed = dict(M)
    for st in steps(feat, tau):
        M[st[1]], A[st[1]] = stage(st, handed, wts, phases)
        handed[st[1]] = hand(M[st[1]])
    return (M, A) if want_abs else M


# ---------------------------------------------------------------------------------------------------------------- MX8
def mx8_encode(v):
    """codec8.h restated: v [..., 16] float32 -> (E [...] int32, codes [..., 16] int32).  E = biased exponent of max|v| (1 + 2^-7), clamped
    to [6, 254]; code = RNE(v 2^(133 - E)) + 128, the low byte of one fused rounding (v 2^(133 - E) is exact: a power-of-two scale)."""
    v = v.to(torch.float32)
    m = v.abs().amax(-1)
    m = m * 0.0078125 + m          # (m 2^-7 is exact, so the sum rounds once, as the kernel's fma does)
    e = (m.view(torch.int32) >> 23).clamp(6, 254)
    scaled = v.to(torch.float64) * torch.exp2(133.0 - e.to(torch.float64))[..., None]
    return e, (torch.round(scaled).to(torch.int32) + 128) & 0xff   # torch.round: half to even


def mx8_decode(e, codes):
    return (codes.to(torch.float64) - 128.0) * torch.exp2(e.to(torch.float64) - 133.0)[..., None]


def lanes(rows, geo, key):
    """The MX8 lanes of dpre vector ``key``: (codes [P, tiles, 2, 16], E [P, tiles, 2]) -- the 16 bytes lane (p, h) holds of double fragment
    t are slots 8 h .. 8 h + 7 of logical fragments 2 t and 2 t + 1, under one scale byte."""
    f0, n = geo["dp"][key]
    u = torch.stack([rows[f0 + i].u for i in range(n // 16)], 1)    # [P, frags, 16]
    e = torch.stack([rows[f0 + i].e for i in range(n // 16)], 1)
    P = u.shape[0]
    u = u.view(P, n // 32, 2, 2, 8).permute(0, 1, 3, 2, 4).reshape(P, n // 32, 2, 16)   # [P, tile, h, half * 8 + j]
    e = e.view(P, n // 32, 2, 2, 8)
    assert bool((e == e[:, :, :1, :, :1]).all())   # one scale byte per lane: both halves, every element
    return u, e[:, :, 0, :, 0]


MX_KEYS = [f"pre{l}" for l in range(8)] + ["feats", "rgbh", "s1", "e1", "s2", "s3"]   # scale groups 0..13 in mlp_layout.h's order
