"""float64 restatement of the layer-by-layer path's kernels (satnerf_amd/csrc/linear.hip): the three matrix products of an nn.Linear whose
input is the concatenation of one or two sources with an activation applied on load, the bias-gradient column sum, and the two small
kernels of the same file (points_along, positional_map).

    FWD  y[p][n]     = out_act( sum_f acat[p][f] W[n][f] + b[n] )
    DX   d_src[p][k] = ( sum_n G[p][n] W[n][col0 + k] ) * act'(src[p][k])
    DW   dW[n][f]   += sum_p G[p][n] acat[p][f],   db[n] += sum_p G[p][n]
    acat[p] = [ act0(src0[p // div0]) | act1(src1[p // div1]) ],   G = gy * out_act'(y)   (out_act' taken from the OUTPUT y)

tests/test_linear_reference_host.py pins these formulas (mode "exact": nothing rounded) to torch.autograd through a float64 nn.Linear
restatement, holds a float32 emulation of the kernel's arithmetic (``Emu``) to every gate, and shows that every planted fault (FAULTS)
leaves one.  tests/test_hip_linear_reference.py holds the kernels to the same gates.  Everything here runs on the CPU.

MODELLED (reproduced bit for bit in float32: the kernel computes them unfused, ``fp contract(off)``, and what follows has large gain):
  the sine phase  t = fl(fl(w0 * v) * 0.15915494f),  fr = min(fl(t - floor(t)), 1 - 2^-24)  (v_fract_f32; exact for t >= 0, one rounding
  of 1 + t for -1 < t < 0);  the reference takes sin / cos of 2 pi fr in float64.  With w0 = 30 one rounding of the phase is ~1e-5 of
  the operand, far outside any gate below, so it is modelled, not bounded.
  points_along  fl(o + fl(d * z)):  compared bit for bit (``points_along``).
  positional_map's argument 2^f * x is exact in float32; the reference is the float64 sin / cos of that float32 number.
  The constants 0.001f and 1.002f of sigmoid_rgb are the float32 numbers the kernel holds.
ASSUMED (named, imported, not restated):
  EPS_SIN (wgrad_reference.py): v_sin_f32 / v_cos_f32 within 2^-19 of the true value, absolute.
  EPS_EXP / EPS_LOG (ray_reference.py): expf / log1pf within one ulp, plus half an ulp for rounding the float64 value; relative.
  EPS_SINF = EPS_EXP: the library sinf / cosf of positional_map_kernel likewise within one ulp.  The HIP math API reference (the HIP
  documentation's "HIP math API" page, table "Single precision mathematical functions") lists sinf and cosf with a maximum error of 1 ULP,
  measured over a bounded test range.  A ROCm installation carries the headers and the device library but no copy of that table (none
  was found under /opt/rocm), so the figure is quoted from the public document and, for arguments of thousands of radians, is an
  assumption about the library's range reduction.  A sinf further off would show as a gate failure of positional_map, not pass unnoticed.

THE GATE of a GEMM output element with operand rows a, b, contraction length K and A = sum_k |a_k| |b_k|:

    |got - M| <= [ 3 * 2^-16 + R * 2^-24 ] A + sum_k ( da_k |b_k| + |a_k| db_k ) + floor

* 3 * 2^-16: the kernel splits each fp32 operand into bf16 hi + lo (RNE) and issues hi*hi + lo*hi + hi*lo.  bf16 has u = 2^-8: the
  residual x - hi - lo is at most 2^-16 |x| per operand and the dropped |lo_a lo_b| <= 2^-16 |a b|.
* R: fp32 roundings on a term's path: 3 * ceil(K / 16) MFMA accumulations (one rounding per v_mfma_f32_32x32x16_bf16, whose 16 products
  of bf16 pairs are exact), + 1 for the bias add (FWD), and for DW, whose contraction is cut into chunks of 1024 points that meet in
  fp32 atomics, K is the chunk length and every atomic but the first onto a zero buffer rounds once more: + (splits - 1), + 1 when the
  buffer held something (those roundings are relative to A + |what the buffer held|).
  colsum_kernel adds fp32 numbers only (no bf16 term): a thread's accumulator takes at most 128 / 4 = 32 unrolled adds + 3 of the tail
  loop, then s += s1 + s2 + s3 (3), the sum of the four row phases (3), and one atomic per 512-row slab: R = 41 + (slabs - 1) [+ 1].
* da, db: the absolute ambiguity of an operand that is a function value: EPS_SIN for a sine operand; for G, |gy| times the fp32 error
  of out_act' evaluated at the y the kernel is handed (the device's own y, which is data to DX and DW), + 2^-24 |G| for the product:
    softplus     1 - expf(-y):                      2^-24 + EPS_EXP e^-y     (absolute: y tiny leaves G tiny but not this error)
    sigmoid      y (1 - y):                         2 * 2^-24 |value|
    sigmoid_rgb  s = (y + 0.001f) / 1.002f, 1.002f s (1 - s):   2^-24 ( 3 |value| + 2 * 1.002 |1 - 2 s| s )
  ReLU and its derivative are exact functions of data.
* DX multiplies the accumulator by act'(src) in its epilogue: gate_acc |act'| + |acc| d_act' + 2^-24 |M| + 2^-126, with d_act' =
  |w0| EPS_SIN + 2^-24 |act'| for the sine (fl(w0 * cos)).
* FWD with an output activation f: gate_pre * |f'(pre)| * e^gate_pre + amb_f.  For all three activations |f''| <= |f'|, so |f'| anywhere
  within gate_pre of pre is at most |f'(pre)| e^gate_pre: the push through is a bound, not a first-order estimate.  amb_f:
    softplus     log1pf(expf(x)):  EPS_EXP e^x / (1 + e^x) + EPS_LOG y    (x > 20 returns x: within e^-20 = 1e-10 y of the same value)
    sigmoid      1 / (1 + expf(-x)):  d_s = EPS_EXP s (1 - s) + 2 * 2^-24 s
    sigmoid_rgb  fl(fl(1.002f s) - 0.001f):  1.002 d_s + 2^-24 (1.002 s + |y|)
* floor = (K + 2) 2^-126: a product or partial sum below the normal range is off by at most 2^-126.
Every element is gated.  Every constant comes from the arithmetic above; none was chosen by looking at a kernel's error.

``fault=`` plants one named fault (FAULTS) into the float32 emulation; only the host self-test sets it."""
import math
import types
import zlib

import torch

from .ray_reference import EPS_EXP, EPS_LOG, TINY, U
from .wgrad_reference import EPS_SIN

EPS_SINF = EPS_EXP          # ASSUMED: library sinf / cosf within one ulp (docstring)
SPLIT = 3 * 2.0 ** -16      # bf16 hi/lo split, lo*lo dropped
KCHUNK, SLAB = 1024, 512    # linear.hip: points per DW workgroup (kchunk), rows per colsum block (kColsumRows)
INV_2PI = 0.15915494309189533577
FR_MAX = 1.0 - 2.0 ** -24   # v_fract_f32 never returns 1
OUT_ACTS = (None, "softplus", "sigmoid", "sigmoid_rgb")

FAULTS = ("drop_lo", "k_late", "k_early", "src_boundary", "no_row_div", "no_col0", "softplus_sigmoid_y", "no_rgb_pad", "drop_chunk",
          "drop_slab", "bias_twice", "dw_overwrite")


def _f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def _ceil(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------- activations
def phase32(x, w0):
    """The fraction of a revolution the kernel hands v_sin_f32 / v_cos_f32, float32, bit for bit."""
    t = (x.float() * _f32(w0)) * _f32(INV_2PI)
    return torch.minimum(t - torch.floor(t), _f32(FR_MAX))


def act_fwd(x, act, w0, mode):
    """act(x) -> (value, ambiguity); mode "ref" (float64 of the modelled float32 phase), "exact" (float64, nothing rounded), "emu" (float32)."""
    if act == "sin":
        if mode == "exact":
            v = torch.sin(w0 * x.double())
            return v, torch.zeros_like(v)
        v = torch.sin(2 * math.pi * phase32(x, w0).double())
        return (v.float(), None) if mode == "emu" else (v, torch.full_like(v, EPS_SIN))
    x = x.float() if mode == "emu" else x.double()
    v = torch.where(x > 0, x, torch.zeros_like(x)) if act == "relu" else x.clone()     # relu(-0) = +0, as v > 0 ? v : 0
    return v, (None if mode == "emu" else torch.zeros_like(v))


def act_grad(x, act, w0, mode):
    if act == "sin":
        if mode == "exact":
            v = w0 * torch.cos(w0 * x.double())
            return v, torch.zeros_like(v)
        c = torch.cos(2 * math.pi * phase32(x, w0).double())
        if mode == "emu":
            return _f32(w0) * c.float(), None
        v = float(_f32(w0)) * c
        return v, abs(float(_f32(w0))) * EPS_SIN + U * v.abs()
    x = x.float() if mode == "emu" else x.double()
    v = (x > 0).to(x.dtype) if act == "relu" else torch.ones_like(x)
    return v, (None if mode == "emu" else torch.zeros_like(v))


def _pad(mode):
    """The 0.001 / 1.002 of sigmoid_rgb as the mode holds them."""
    return (0.001, 1.002) if mode == "exact" else (float(_f32(0.001)), float(_f32(1.002)))


def out_fwd(pre, oa, mode, fault=None):
    """out_act(pre) -> (y, |f'(pre)|, amb_f) in float64, or the float32 y of the emulation."""
    if mode == "emu":
        x = pre.float()
        if oa == "softplus":
            return torch.where(x > 20, x, torch.log1p(torch.exp(x)))
        if oa in ("sigmoid", "sigmoid_rgb"):
            s = 1.0 / (1.0 + torch.exp(-x))
            return s if oa == "sigmoid" or fault == "no_rgb_pad" else s * _f32(1.002) - _f32(0.001)
        return x
    x = pre.double()
    if oa is None:
        return x, torch.ones_like(x), torch.zeros_like(x)
    s = torch.sigmoid(x)
    if oa == "softplus":
        y = torch.nn.functional.softplus(x, threshold=1e9)
        return y, s, EPS_EXP * s + EPS_LOG * y
    ds = EPS_EXP * s * (1 - s) + 2 * U * s
    if oa == "sigmoid":
        return s, s * (1 - s), ds
    c0, c1 = _pad(mode)
    y = s * c1 - c0
    return y, c1 * s * (1 - s), c1 * ds + U * (c1 * s + y.abs())


def out_grad(y, oa, mode, fault=None):
    """out_act' from the output y -> (value, absolute fp32 error of the kernel's formula)."""
    if mode == "emu":
        y = y.float()
        if oa == "softplus":
            return (1.0 / (1.0 + torch.exp(-y)) if fault == "softplus_sigmoid_y" else 1.0 - torch.exp(-y)), None
        if oa == "sigmoid" or (oa == "sigmoid_rgb" and fault == "no_rgb_pad"):
            return y * (1.0 - y), None
        if oa == "sigmoid_rgb":
            s = (y + _f32(0.001)) / _f32(1.002)
            return _f32(1.002) * s * (1.0 - s), None
        return torch.ones_like(y), None
    y = y.double()
    if oa is None:
        return torch.ones_like(y), torch.zeros_like(y)
    if oa == "softplus":
        return -torch.expm1(-y), U + EPS_EXP * torch.exp(-y)
    if oa == "sigmoid":
        v = y * (1 - y)
        return v, 2 * U * v.abs()
    c0, c1 = _pad(mode)
    s = (y + c0) / c1
    v = c1 * s * (1 - s)
    return v, U * (3 * v.abs() + 2 * c1 * (1 - 2 * s).abs() * s.abs())


def acat(srcs, p, mode, fault=None):
    """[act0(src0[p // div0]) | act1(src1[p // div1])] -> (value (P, K), ambiguity)."""
    vals, ambs = [], []
    for x, act, w0, div in srcs:
        rows = torch.arange(p) // (1 if fault == "no_row_div" else div)
        v, a = act_fwd(x[rows.clamp(max=x.shape[0] - 1)], act, w0, mode)
        vals.append(v), ambs.append(a)
    v = torch.cat(vals, 1)
    if fault == "src_boundary" and len(srcs) > 1:      # the second source taken to begin one column early
        k0 = srcs[0][0].shape[1]
        v = torch.cat([v[:, :k0 - 1], v[:, k0:], torch.zeros_like(v[:, :1])], 1)
    return v, (None if mode == "emu" else torch.cat(ambs, 1))


def gmat(gy, y, oa, mode, fault=None):
    """G = gy * out_act'(y) -> (value (P, N), ambiguity)."""
    if mode == "emu":
        return (gy.float() if oa is None else gy.float() * out_grad(y, oa, mode, fault)[0]), None
    g = gy.double()
    if oa is None:
        return g, torch.zeros_like(g)
    d, e = out_grad(y, oa, mode)
    v = g * d
    return v, (torch.zeros_like(v) if mode == "exact" else g.abs() * e + U * v.abs())


# -------------------------------------------------------------------------------------------------------------------- GEMM
def gemm(a, b, da, db, rounds):
    """a (M, K) . b (N, K)^T in float64 -> (value, gate without the roundings' extra addends, A)."""
    k = a.shape[1]
    big = a.abs() @ b.abs().T
    gate = (SPLIT + rounds * U) * big + da @ b.abs().T + a.abs() @ db.T + (k + 2) * TINY
    return a @ b.T, gate, big


def _split(x):
    hi = x.bfloat16().float()
    return hi.double(), (x - hi).bfloat16().float().double()


def gemm_emu(a, b, fault=None):
    """The kernel's arithmetic in float32: RNE bf16 hi/lo split, per 16-wide k-step the passes lo*hi, hi*lo, hi*hi, each one fp32
    rounding of accumulator + 16 exact products (summed in float64: exact to well below fp32's half ulp)."""
    k = a.shape[1]
    kp = _ceil(k, 16) * 16
    a = torch.nn.functional.pad(a.float(), (0, kp - k))
    b = torch.nn.functional.pad(b.float(), (0, kp - k))
    (ah, al), (bh, bl) = _split(a), _split(b)
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
    for s in range(0, kp, 16):
        passes = [(ah, bl), (ah, bh)] if fault == "drop_lo" else [(al, bh), (ah, bl), (ah, bh)]
        for x, y in passes:
            acc = (acc.double() + x[:, s:s + 16] @ y[:, s:s + 16].T).float()
    return acc


def _k_early(t, fault):
    """Fault: the last k of a ragged 32-wide tile zeroed one k too early (t: (rows, K), contraction along dim 1)."""
    if fault == "k_early" and t.shape[1] % 32:
        t = t.clone()
        t[:, -1] = 0
    return t


# --------------------------------------------------------------------------------------------------------------- reference
def fwd(srcs, w, b, p, oa, mode="ref"):
    """sr_linear_fwd -> (y, gate), float64 (P, n_out)."""
    a, da = acat(srcs, p, mode)
    k = a.shape[1]
    pre, gate, big = gemm(a, w.double(), da, torch.zeros_like(w, dtype=torch.float64), 3 * _ceil(k, 16) + 1)
    if b is not None:
        pre = pre + b.double()
        gate = gate + U * b.double().abs()                      # the bias add rounds once, relative to at most A + |b|
    y, d, amb = out_fwd(pre, oa, mode)
    return y, (gate * d * torch.exp(gate) + amb if oa is not None else gate)


def dx(gy, y, oa, w, col0, target, p, mode="ref"):
    """sr_linear_bwd_input -> (d_src per point (P, k), gate)."""
    x, act, w0, div = target
    k = x.shape[1]
    g, dg = gmat(gy, y, oa, mode)
    wt = w.double()[:, col0:col0 + k].T.contiguous()          # (k, n_out)
    acc, gate, _ = gemm(g, wt, dg, torch.zeros_like(wt), 3 * _ceil(g.shape[1], 16))
    if act is None:
        return acc, gate
    assert div == 1, "an activated source is per point"
    d, dd = act_grad(x[:p], act, w0, mode)
    m = acc * d
    return m, gate * d.abs() + acc.abs() * dd + U * m.abs() + TINY        # + the product's own underflow floor


def dw(gy, y, oa, srcs, p, n_out, want_bias=True, pre_w=None, pre_b=None, mode="ref"):
    """sr_linear_bwd_weight -> (dW, gate, db, gate) with what the buffers held before added in; db None without ``want_bias``."""
    g, dg = gmat(gy, y, oa, mode)
    a, da = acat(srcs, p, mode)
    splits, slabs = _ceil(p, KCHUNK), _ceil(p, SLAB)
    mw, gate_w, big = gemm(g.T.contiguous(), a.T.contiguous(), dg.T.contiguous(), da.T.contiguous(), 3 * _ceil(min(p, KCHUNK), 16))
    hw = torch.zeros_like(mw) if pre_w is None else pre_w.double()
    gate_w = gate_w + (splits - 1 + int(pre_w is not None)) * U * (big + hw.abs())
    if not want_bias:
        return mw + hw, gate_w, None, None
    hb = torch.zeros(n_out, dtype=torch.float64) if pre_b is None else pre_b.double()
    rb = 41 + slabs - 1 + int(pre_b is not None)
    gate_b = rb * U * (g.abs().sum(0) + hb.abs()) + dg.sum(0) + (p + 2) * TINY
    return mw + hw, gate_w, g.sum(0) + hb, gate_b


def points_along(rays, dir_col, z):
    """fl(o + fl(d * z)) in float32, (N * S, 3): the kernel's own bits."""
    o, d = rays[:, 0:3].float().unsqueeze(1), rays[:, dir_col:dir_col + 3].float().unsqueeze(1)
    return (o + d * z.float().unsqueeze(-1)).reshape(-1, 3)


def positional_map(x, n_freqs):
    """(rows, dim) -> (value, gate) (rows, 2 * n_freqs * dim): [sin(2^0 x), cos(2^0 x), sin(2^1 x), ...] of the exact float32 argument."""
    arg = torch.stack([(x.float() * _f32(2.0 ** f)).double() for f in range(n_freqs)], 1)      # (rows, F, dim): exact in fp32
    v = torch.stack([torch.sin(arg), torch.cos(arg)], 2).reshape(x.shape[0], -1)
    return v, EPS_SINF * v.abs() + TINY


# --------------------------------------------------------------------------------------------------------------- emulation
class Emu:
    """The kernels' float32 arithmetic on the CPU, with the interface the device backend of the GPU test has."""

    def __init__(self, fault=None):
        self.fault = fault

    def fwd(self, srcs, w, b, p, oa):
        f = self.fault
        a, _ = acat(srcs, p, "emu", f)
        pre = gemm_emu(_k_early(a, f), w, f)
        if b is not None:
            pre = pre + b.float()
            if f == "bias_twice":
                pre = pre + b.float()
        return out_fwd(pre, oa, "emu", f)

    def dx(self, gy, y, oa, w, col0, target, p):
        f = self.fault
        x, act, w0, div = target
        k = x.shape[1]
        g, _ = gmat(gy, y, oa, "emu", f)
        c = 0 if f == "no_col0" else col0
        acc = gemm_emu(_k_early(g, f), w.float()[:, c:c + k].T.contiguous(), f)
        return acc if act is None else acc * act_grad(x[:p], act, w0, "emu")[0]

    def dw(self, gy, y, oa, srcs, p, n_out, want_bias=True, pre_w=None, pre_b=None):
        f = self.fault
        g, _ = gmat(gy, y, oa, "emu", f)
        a, _ = acat(srcs, p, "emu", f)
        out = torch.zeros(n_out, a.shape[1]) if pre_w is None or f == "dw_overwrite" else pre_w.float().clone()
        chunks = list(range(0, p, KCHUNK))
        for c0 in chunks[:-1] if f == "drop_chunk" and len(chunks) > 1 else chunks:
            c1 = min(c0 + KCHUNK, p)
            if f == "k_late" and c1 < p:
                c1 += 1                      # the row behind a chunk's end not masked: counted by this chunk and by the next
            out = out + gemm_emu(_k_early(g[c0:c1].T.contiguous(), f), a[c0:c1].T.contiguous(), f)
        if not want_bias:
            return out, None
        db = torch.zeros(n_out) if pre_b is None or f == "dw_overwrite" else pre_b.float().clone()
        slabs = list(range(0, p, SLAB))
        for p0 in slabs[:-1] if f == "drop_slab" and len(slabs) > 1 else slabs:
            part = []
            for ph in range(4):                                   # colsum_kernel's thread (column, row phase)
                r = g[p0 + ph:min(p0 + SLAB, p):4]
                s = [torch.zeros(n_out) for _ in range(4)]
                j = 0
                while j + 3 < r.shape[0]:
                    for e in range(4):
                        s[e] = s[e] + r[j + e]
                    j += 4
                for jj in range(j, r.shape[0]):
                    s[0] = s[0] + r[jj]
                part.append(s[0] + ((s[1] + s[2]) + s[3]))
            db = db + (((part[0] + part[1]) + part[2]) + part[3])
        return out, db


# ------------------------------------------------------------------------------------------------------------------- cases
def S(k, act=None, w0=1.0, div=1, lay="dense"):
    """One source of a case: width, activation, w0, row_div, memory layout ("dense"; "rays" = columns 8:8+k of an (n, 11) tensor;
    "off1" = columns 1:1+k of a tensor two columns wider: ld > k, rows not 16-byte aligned)."""
    return (k, act, w0, div, lay)


def case(p, n_out, srcs, oa=None, bias=True, want_bias=True, deep=False):
    return dict(p=p, n_out=n_out, srcs=tuple(srcs), oa=oa, bias=bias, want_bias=want_bias, deep=deep)


ACTS = ((None, 1.0), ("sin", 1.0), ("sin", 1.7), ("sin", 30.0), ("relu", 1.0))
ROWS = (1, 127, 128, 129, 296, 511, 512, 513, 1023, 1024, 1025, 2048 + 17)
N_OUTS = (1, 3, 127, 128, 129, 136)
KS = (1, 3, 31, 32, 33, 35, 130)
PAIRS = ((3, 64), (3, 256), (63, 4), (61, 16), (64, 5))
SKIP = (S(3), S(64, "sin", 1.7))            # the skip layer [xyz | h]: the source boundary inside a group of four, col0 = 3

CASES = (
    # rows: FWD / DX tiles (1 .. 296) and DW split-K chunks / colsum slabs (511 .. 2065 = three chunks, the last of 17; five slabs)
    [case(p, 129, SKIP) for p in ROWS]
    # columns x contraction, the activations rotating through them
    + [case(129, n, (S(k, *ACTS[(i + j) % 5]),), OUT_ACTS[(i + 2 * j) % 4], deep=True) for j, n in enumerate(N_OUTS) for i, k in enumerate(KS)]
    # every act x every out_act; softplus / sigmoid heads with pre-activations down to -15
    + [case(129, 5, (S(33, a, w),), oa, deep=True) for a, w in ACTS for oa in OUT_ACTS]
    # two sources: the boundary inside and on a group of four, col0 = 3 / 61 / 63 / 64
    + [case(p, 136, (S(k0, "relu" if k0 > 3 else None), S(k1, "sin", 30.0)), oa) for k0, k1 in PAIRS for p, oa in ((129, None), (1025, "softplus"))]
    # NeRF's colour head [h(60) | dir encoding(24) per ray], row_div 50 and 4, rows to spare, n_points no multiple of either
    + [case(p, 3, (S(60, "relu"), S(24, None, 1.0, div)), "sigmoid_rgb" if div == 50 else "sigmoid") for div in (4, 50) for p in (129, 1025)]
    + [case(129, 64, (S(61, "sin", 1.7), S(16, "relu", 1.0, 4)))]
    # DW with M = n_out = 128 and N = k0 + k1 = 128: both extents exact multiples of the tile
    + [case(129, 128, (S(64, "relu"), S(64, "sin", 1.7)))]
    # views: rays[:, 8:11] of an (n, 11) tensor, x[:, 1:] of a wider one
    + [case(129, 128, (S(3, lay="rays"), S(64, "sin", 30.0))), case(129, 136, (S(35, "sin", 1.7, lay="off1"),), "softplus"),
       case(296, 127, (S(3, lay="rays"), S(256, "relu", lay="off1")))]
    # no bias; no bias gradient
    + [case(129, 35, SKIP, "sigmoid", bias=False), case(513, 35, SKIP, "softplus", want_bias=False)]
)


def case_id(c):
    src = "+".join(f"{k}{(a or 'id')[:3]}{w0:g}" + (f"d{div}" if div > 1 else "") + ("" if lay == "dense" else lay) for k, a, w0, div, lay in c["srcs"])
    flags = ("" if c["bias"] else "-nobias") + ("" if c["want_bias"] else "-nodb") + ("-deep" if c["deep"] else "")
    return f"p{c['p']}-n{c['n_out']}-{src}-{c['oa'] or 'none'}" + flags


_BUILT = {}


def build(c):
    """The case's tensors (float32, CPU; built once, nobody writes to them): ``bases`` = the tensors the sources are views of, ``srcs`` =
    (view, act, w0, row_div), w, b (or None), gy."""
    key = case_id(c)
    if key in _BUILT:
        return _BUILT[key]
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()))
    p, n_out = c["p"], c["n_out"]
    bases, srcs = [], []
    for k, act, w0, div, lay in c["srcs"]:
        rows = _ceil(p, div) + (3 if div > 1 else 0)              # a per-ray source has rows to spare
        wide, c0 = {"dense": (k, 0), "rays": (11, 8), "off1": (k + 2, 1)}[lay]
        base = torch.randn(rows, wide, generator=g)
        if act == "relu":                                         # exact zeros and negative zeros among the inputs
            base[::5, ::3] = 0.0
            base[1::5, 1::3] = -0.0
        bases.append(base)
        srcs.append((base[:, c0:c0 + k], act, w0, div))
    ktot = sum(s[0].shape[1] for s in srcs)
    w = torch.randn(n_out, ktot, generator=g) / ktot ** 0.5
    b = torch.randn(n_out, generator=g)
    if c["deep"] and c["oa"] is not None:
        b = b + torch.linspace(-15.0, 2.0, n_out)                 # heads whose output is tiny: the per-element gate decides there
    out = types.SimpleNamespace(p=p, n_out=n_out, oa=c["oa"], bases=bases, srcs=srcs, w=w, b=b if c["bias"] else None,
                                gy=torch.randn(p, n_out, generator=g), want_bias=c["want_bias"],
                                col0=[0] + [srcs[0][0].shape[1]] * (len(srcs) - 1))
    _BUILT[key] = out
    return out


def ratio(got, want, gate):
    """|got - want| / gate per element; a NaN or a wrong shape is outside every gate."""
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    err = (got - want).abs()
    return torch.where(torch.isfinite(err), err / gate, torch.full_like(err, float("inf")))


def run_case(c, be):
    """FWD, DX of every source, DW + colsum of one case through backend ``be`` (Emu or the device) -> {kind: ratio tensor}.  DX and DW
    are handed the backend's own y, as the trainer hands them the forward's."""
    t = build(c)
    out = {}
    y = be.fwd(t.srcs, t.w, t.b, t.p, t.oa)
    out["fwd"] = ratio(y, *fwd(t.srcs, t.w, t.b, t.p, t.oa))
    y = y.detach().cpu()
    yy = y if t.oa is not None else None
    for i, (src, col0) in enumerate(zip(t.srcs, t.col0)):
        if src[1] is not None and src[3] != 1:
            continue                                              # the C entry refuses an activated per-ray source
        out[f"dx{i}"] = ratio(be.dx(t.gy, yy, t.oa, t.w, col0, src, t.p), *dx(t.gy, yy, t.oa, t.w, col0, src, t.p))
    gw, gb = be.dw(t.gy, yy, t.oa, t.srcs, t.p, t.n_out, t.want_bias)
    mw, gate_w, mb, gate_b = dw(t.gy, yy, t.oa, t.srcs, t.p, t.n_out, t.want_bias)
    out["dw"] = ratio(gw, mw, gate_w)
    if t.want_bias:
        out["db"] = ratio(gb, mb, gate_b)
    else:
        assert gb is None
    return out


def worst(ratios):
    """{kind: ratio tensor} -> {fwd, dx, dw, db: worst ratio}."""
    res = {}
    for k, r in ratios.items():
        kind = "dx" if k.startswith("dx") else k
        res[kind] = max(res.get(kind, 0.0), float(r.max()))
    return res
