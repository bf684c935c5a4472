"""Typed Python wrappers over the C ABI (one function per entry point of include/satrender.h).

Every wrapper validates device / dtype / contiguity (the library itself sees only raw pointers), enqueues on
torch's current HIP stream and returns torch tensors it allocated.  No arithmetic happens here beyond the small host-side tables
an entry is defined to take (e.g. ``lanczos_tables``).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import torch

from . import _lib

MODES = {"bf16": _lib.MODE_BF16, "f16": _lib.MODE_F16, "bf16x3": _lib.MODE_BF16X3}


class KernelTimer:
    """Brackets selected kernel launches with HIP events on torch's current stream (bench.py's roofline leg)."""

    def __init__(self):
        self.spans = []

    def span(self, name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.spans.append((name, e0, e1))
        return e0, e1

    def mean_ms(self, name):
        t = [a.elapsed_time(b) for n, a, b in self.spans if n == name]
        return sum(t) / len(t) if t else None


kernel_timer = None  # set to a KernelTimer to time the fused-MLP launches


@contextlib.contextmanager
def _timed(name):
    """A ``kernel_timer`` span around the launches of the block (nothing when no timer is set)."""
    if kernel_timer is None:
        yield
        return
    e0, e1 = kernel_timer.span(name)
    e0.record()
    yield
    e1.record()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk(t, name, dtype=torch.float32, allow_none=False):
    if t is None:
        if allow_none:
            return None
        raise ValueError(f"{name} is required")
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (got {t.device}); satnerf_amd has no CPU path")
    _same_device(t, name)
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype} (got {t.dtype})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def _same_device(t, name):
    """Launches go to torch's CURRENT stream, i.e. to the current device: a tensor living on another GPU would be touched by the
    wrong device's kernel."""
    if t.device.index != torch.cuda.current_device():
        raise ValueError(f"{name} lives on {t.device} but the current device is cuda:{torch.cuda.current_device()} "
                         "(wrap the call in torch.cuda.device(...) or torch.cuda.set_device)")


def _scratch_bytes(entry, *args):
    """What a ``*_scratch`` entry point answers for these integer sizes (host only)."""
    nbytes = C.c_int64(0)
    _lib.call(entry, *(int(a) for a in args), C.byref(nbytes))
    return nbytes.value


def _rows(t, name, min_cols):
    """A 2-D fp32 view whose rows may be strided (e.g. rays[:, 3:6]): returns (tensor, row stride in elements)."""
    if t.dim() != 2 or t.shape[1] < min_cols or t.dtype != torch.float32 or not t.is_cuda or t.stride(1) != 1:
        raise ValueError(f"{name} must be a GPU fp32 (N,>={min_cols}) tensor with unit inner stride")
    _same_device(t, name)
    return t, t.stride(0) if t.shape[0] > 1 else t.shape[1]


def pack_stream(flat, idx, scale, want_lo, f16=False):
    """Gather + scale + convert the weight stream: bf16 hi (and lo) planes, or fp16 (``f16``: the SR_MODE_F16 forward stream)."""
    n = idx.numel()
    hi = torch.empty(n, dtype=torch.int16, device=flat.device)
    lo = torch.empty(n, dtype=torch.int16, device=flat.device) if want_lo else None
    _lib.call("sr_pack_stream", _p(_chk(flat, "flat")), _p(_chk(idx, "idx", torch.int32)), _p(_chk(scale, "scale")), n, _p(hi), _p(lo),
              n if f16 else 0, _stream())
    return hi, lo


def pack_stream_into(flat, idx, scale, hi, lo, f16=False):
    _lib.call("sr_pack_stream", _p(_chk(flat, "flat")), _p(_chk(idx, "idx", torch.int32)), _p(_chk(scale, "scale")), idx.numel(), _p(hi), _p(lo),
              idx.numel() if f16 else 0, _stream())


def gather_scale_into(flat, idx, scale, out):
    _lib.call("sr_gather_scale_f32", _p(_chk(flat, "flat")), _p(_chk(idx, "idx", torch.int32)), _p(_chk(scale, "scale")), idx.numel(), _p(out),
              _stream())


def gather_scale(flat, idx, scale):
    out = torch.empty(idx.numel(), dtype=torch.float32, device=flat.device)
    _lib.call("sr_gather_scale_f32", _p(_chk(flat, "flat")), _p(_chk(idx, "idx", torch.int32)), _p(_chk(scale, "scale")), idx.numel(), _p(out),
              _stream())
    return out


def ray_sample(rays, u, n_samples):
    rays, stride = _rows(rays, "rays", 8)
    n = rays.shape[0]
    _chk(u, "u")
    if tuple(u.shape) != (n, n_samples):
        raise ValueError(f"u must be ({n},{n_samples}), got {tuple(u.shape)}")
    z = torch.empty(n, n_samples, dtype=torch.float32, device=rays.device)
    _lib.call("sr_ray_sample_fwd", _p(rays), stride, _p(u), n, n_samples, _p(z), _stream())
    return z


def sky(sun, w1, b1, w2, b2):
    sun, stride = _rows(sun, "sun", 3)
    n, hidden = sun.shape[0], w1.shape[0]
    out = torch.empty(n, 3, dtype=torch.float32, device=sun.device)
    _lib.call("sr_sky_fwd", _p(sun), stride, n, hidden, _p(_chk(w1, "w1")), _p(_chk(b1, "b1")), _p(_chk(w2, "w2")), _p(_chk(b2, "b2")), _p(out),
              _stream())
    return out


def _mlp_inputs(org, direction, sun, z, temb, ts, n_points, n_samples):
    """The sr_mlp_inputs block of a point launch, its tensors validated (``org`` / ``direction`` / ``sun`` may be strided rows)."""
    org, so = _rows(org, "org", 3)
    sun, ss = _rows(sun, "sun", 3)
    sd = 0
    if direction is not None:
        direction, sd = _rows(direction, "dir", 3)
    if z is not None:
        _chk(z, "z")
    _chk(temb, "temb")
    if ts is not None:
        _chk(ts, "ts", torch.int64)
    return _lib.MlpInputs(_p(org), so, _p(direction), sd, _p(sun), ss, _p(z), _p(temb), _p(ts), n_points, n_samples)


def _render_args(rays, ts, temb, n_samples, sky, z, u, noise, noise_std, seed, step_counter, tick, bank_chunks=0, n=None):
    """The sr_render_args block of a render launch over ``n`` rays (default: the rows of ``rays``), its tensors validated; ``sky`` =
    (w1, b1, w2, b2) or None.  Returns (args, n, n_samples, an allocator of fp32 tensors on the rays' device)."""
    rays, stride = _rows(rays, "rays", 11)
    n, s = rays.shape[0] if n is None else n, int(n_samples)
    _chk(ts, "ts", torch.int64), _chk(temb, "temb")
    for t, nm in ((z, "z"), (u, "u"), (noise, "noise")):
        if t is not None and tuple(_chk(t, nm).shape) != (n, s):
            raise ValueError(f"{nm} must be ({n},{s}), got {tuple(t.shape)}")
    if tick and (step_counter is None or step_counter.numel() < 4):
        raise ValueError("tick=True needs step_counter = a zero-initialised float32 block of 4")
    w = [None] * 4 if sky is None else [_chk(t, nm) for t, nm in zip(sky, ("w1", "b1", "w2", "b2"))]
    args = _lib.RenderArgs(_p(rays), stride, _p(ts), _p(temb), n, s, _p(z), _p(u), int(seed) & 0xFFFFFFFFFFFFFFFF,
                           _p(_chk(step_counter, "step_counter", allow_none=True)), int(tick), _p(noise), float(noise_std),
                           0 if sky is None else w[0].shape[0], *map(_p, w), int(bank_chunks))
    return args, n, s, lambda *shape: torch.empty(*shape, dtype=torch.float32, device=rays.device)


def _render_outputs(out, z=None):
    """The sr_render_outputs block of a wrapper's result dict: an absent or None entry is not written, nor are given depths ``z``."""
    return _lib.RenderOutputs(None if z is not None else _p(out.get("z")),
                              *(_p(out.get(k)) for k in ("albedo", "sigma", "sun_v", "beta", "sky", "weights", "transparency", "depth", "rgb")))


def satnerf_mlp(org, direction, sun, z, temb, ts, n_points, n_samples, feat, tau, mode, stream_hi, stream_lo, l0, acts=None, fmt=16):
    """Fused MLP over n_points sample points; returns (albedo (P,3), sigma (P), sun_v (P), beta (P)).  ``acts`` = training
    workspace (``acts_workspace(..., fmt)``) the activations are saved to in format ``fmt`` (16 | 8)."""
    inp = _mlp_inputs(org, direction, sun, z, temb, ts, n_points, n_samples)
    dev = org.device
    albedo = torch.empty(n_points, 3, dtype=torch.float32, device=dev)
    sigma = torch.empty(n_points, dtype=torch.float32, device=dev)
    sun_v = torch.empty(n_points, dtype=torch.float32, device=dev)
    beta = torch.empty(n_points, dtype=torch.float32, device=dev)
    with _timed("mlp_fwd"):
        _lib.call("sr_satnerf_mlp_fwd", C.byref(inp), feat, tau, MODES[mode], _p(stream_hi), _p(stream_lo), _p(_chk(l0, "l0")), _p(albedo), _p(sigma),
                  _p(sun_v), _p(beta), _p(acts), int(fmt), _stream())
    return albedo, sigma, sun_v, beta


def render_fused_ok(feat, mode, n_samples):
    """True when sr_satnerf_render_fwd covers (feat, mode) and ``n_samples`` divides the points a workgroup owns."""
    per_block = _lib.lib().sr_render_points_per_block(int(feat), MODES[mode])
    return per_block > 0 and n_samples >= 2 and per_block % n_samples == 0


def render_fwd(rays, ts, temb, n_samples, feat, tau, mode, stream_hi, stream_lo, l0, sky_w1, sky_b1, sky_w2, sky_b2, z=None, u=None, noise=None,
               noise_std=0.0, seed=0, step_counter=None, tick=False, want_z=True, bank_chunks=0, want_sigma=False):
    """One launch: stratified sampling (or given depths ``z``) -> fused MLP -> sky head + compositing (sr_satnerf_render_fwd).
    Depths: ``z`` (N,S) given, else stratified with ``u`` (N,S), else jitter drawn in the kernel (``seed``, ``step_counter``, ``tick``).
    ``bank_chunks`` > 0: ``rays`` / ``ts`` are a bank of bank_chunks x N rows and the launch renders chunk step_counter[0] % bank_chunks.
    Returns dict(z, albedo (N,S,3), sun_v (N,S), beta (N,S), sky (N,3), weights, transparency (N,S), depth (N), rgb (N,3)), and
    ``sigma`` (N,S) with ``want_sigma``."""
    n = None
    if bank_chunks:
        if rays.shape[0] % bank_chunks or ts.numel() != rays.shape[0] or step_counter is None:
            raise ValueError("bank mode: rays / ts must hold bank_chunks x N rows and step_counter is required")
        n = rays.shape[0] // bank_chunks
    args, n, s, e = _render_args(rays, ts, temb, n_samples, (sky_w1, sky_b1, sky_w2, sky_b2), z, u, noise, noise_std, seed, step_counter, bool(tick),
                                 bank_chunks, n)
    out = {"z": z if z is not None else (e(n, s) if want_z else None), "albedo": e(n, s, 3), "sun_v": e(n, s), "beta": e(n, s), "sky": e(n, 3),
           "weights": e(n, s), "transparency": e(n, s), "depth": e(n), "rgb": e(n, 3)}
    if want_sigma:
        out["sigma"] = e(n, s)
    outs = _render_outputs(out, z)
    with _timed("mlp_fwd"):
        _lib.call("sr_satnerf_render_fwd", C.byref(args), feat, tau, MODES[mode], _p(stream_hi), _p(stream_lo), _p(_chk(l0, "l0")), C.byref(outs), _stream())
    return out


def render_depth(rays, ts, temb, n_samples, feat, tau, mode, stream_hi, stream_lo, l0, sky=None, z=None, u=None, noise=None, noise_std=0.0, seed=0,
                 step_counter=None, tick=False, want_z=True, want_sigma=False):
    """The depth-only render pass in one launch (sr_satnerf_render_depth): ``render_fwd``'s sampling and inputs, the trunk and the sigma
    row of the same packed stream, sigma-only compositing -- no colour, sun, uncertainty or sky weight is read in the ``bf16`` / ``f16``
    modes.  ``sky`` = (w1, b1, w2, b2) or None: only the configurations the full kernel serves (``bf16x3``, SATNERF_FWD_V1=1) need it.
    ``n_samples`` must divide the points of a workgroup (``render_fused_ok``); otherwise the C entry's error is raised.
    Returns dict(z (N,S) or None, sigma (N,S) or None, weights, transparency (N,S), depth (N)): ``render_fwd``'s values bit for bit."""
    args, n, s, e = _render_args(rays, ts, temb, n_samples, sky, z, u, noise, noise_std, seed, step_counter, bool(tick))
    out = {"z": z if z is not None else (e(n, s) if want_z else None), "sigma": e(n, s) if want_sigma else None, "weights": e(n, s),
           "transparency": e(n, s), "depth": e(n)}
    if n == 0:
        return out
    outs = _render_outputs(out, z)
    with _timed("mlp_fwd"):
        _lib.call("sr_satnerf_render_depth", C.byref(args), feat, tau, MODES[mode], _p(stream_hi), _p(stream_lo), _p(_chk(l0, "l0")), C.byref(outs),
                  _stream())
    return out


def satnerf_sigma(org, direction, sun, z, temb, ts, n_points, n_samples, feat, tau, mode, stream_hi, stream_lo, l0):
    """sigma (P,) of the fused MLP over n_points sample points (sr_satnerf_mlp_sigma): ``satnerf_mlp``'s arguments and its sigma bit for
    bit, from the trunk-and-sigma core -- the heads are not evaluated."""
    inp = _mlp_inputs(org, direction, sun, z, temb, ts, n_points, n_samples)
    sigma = torch.empty(n_points, dtype=torch.float32, device=org.device)
    if n_points == 0:
        return sigma
    with _timed("mlp_fwd"):
        _lib.call("sr_satnerf_mlp_sigma", C.byref(inp), feat, tau, MODES[mode], _p(stream_hi), _p(stream_lo), _p(_chk(l0, "l0")), _p(sigma), _stream())
    return sigma


def render_train(rays, ts, temb, n_samples, feat, tau, mode, stream_hi, stream_lo, l0, sky_w1, sky_b1, sky_w2, sky_b2, target, acts, u=None,
                 noise=None, noise_std=0.0, seed=0, step_counter=None, sched=None, beta_min=0.05, want_z=False, tick=0, gather=None):
    """The training forward in ONE launch (sr_satnerf_render_train): stratified depths (``u`` (N,S) given, else drawn in the kernel from
    ``seed`` / ``step_counter``) -> fused MLP saving the 8-bit activations into ``acts`` -> sky head, compositing, colour loss and the
    compositing backward per ray.  Returns dict(albedo (N,S,3), sigma, sun_v, beta (N,S), sky (N,3), z (N,S) or None, loss (partial sums),
    rgb (N,3), d_sigma, d_sun, g_beta (N,S), d_albedo (N,S,3), d_sky (N,3)) -- what ``ray_setup`` + ``satnerf_mlp`` + ``render_loss``
    return, bit for bit.  ``tick`` = 2: the launch opens the step (advances ``step_counter`` and draws for the advanced value).
    ``gather`` = dict(idx, cursor, batches, out=(rays (N,11), rgbs (N,3), ts (N))): ``rays`` / ``ts`` / ``target`` are the resident bank and
    the launch samples batch cursor[0] of the epoch's shuffled ``idx`` itself, writing the batch rows to ``out``."""
    args, n, s, e = _render_args(rays, ts, temb, n_samples, (sky_w1, sky_b1, sky_w2, sky_b2), None, u, noise, noise_std, seed, step_counter, tick,
                                 n=None if gather is None else gather["out"][0].shape[0])
    if gather is not None:
        o_rays, o_rgbs, o_ts = gather["out"]
        if (args.ray_stride != 11 or tuple(_chk(o_rays, "out rays").shape) != (n, 11) or tuple(_chk(o_rgbs, "out rgbs").shape) != (n, 3)
                or tuple(_chk(o_ts, "out ts", torch.int64).shape) != (n,) or _chk(gather["idx"], "idx", torch.int64).numel() < int(gather["batches"]) * n
                or target.shape[0] != rays.shape[0] or ts.shape[0] != rays.shape[0] or u is not None or noise is not None):
            raise ValueError("gather: the bank (rays (R,11), ts (R), target (R,3)), idx (>= batches x N) and out = ((N,11), (N,3), (N,)) do not fit")
    per_block = _lib.lib().sr_render_points_per_block(int(feat), MODES[mode])
    if per_block <= 0 or s > 64 or per_block % s:
        raise ValueError(f"no fused training forward for feat={feat}, mode={mode}, n_samples={s}")
    out = {"z": e(n, s) if want_z else None, "albedo": e(n, s, 3), "sigma": e(n, s), "sun_v": e(n, s), "beta": e(n, s), "sky": e(n, 3)}
    outs = _render_outputs(out)  # the launch writes what follows through sr_train_args
    out.update({"loss": e((n * s + per_block - 1) // per_block), "rgb": e(n, 3), "d_sigma": e(n, s), "d_albedo": e(n, s, 3), "d_sun": e(n, s),
                "g_beta": e(n, s), "d_sky": e(n, 3)})
    g = gather or {}
    tr = _lib.TrainArgs(_p(_chk(target, "target")), _p(_chk(sched, "sched", allow_none=True)), float(beta_min), _p(out["loss"]), _p(out["rgb"]),
                        _p(out["d_sigma"]), _p(out["d_albedo"]), _p(out["d_sun"]), _p(out["g_beta"]), _p(out["d_sky"]),
                        _p(g.get("idx")), _p(_chk(g.get("cursor"), "cursor", allow_none=True)), int(g.get("batches", 0)),
                        *([_p(t) for t in g["out"]] if gather is not None else [None, None, None]))
    with _timed("mlp_fwd"):
        _lib.call("sr_satnerf_render_train", C.byref(args), feat, tau, MODES[mode], _p(stream_hi), _p(stream_lo), _p(_chk(l0, "l0")), C.byref(outs),
                  C.byref(tr), _p(acts), 8, _stream())
    return out


def composite(z, sigma, noise, noise_std, albedo, sun_v, sky_rgb, clamp_rgb=True):
    """Compositing forward: (weights (N,S), transparency (N,S), depth (N,), rgb (N,3)).  ``albedo`` None = sigma-only (rgb is zero), as
    composite_bwd takes it; ``sun_v`` / ``sky_rgb`` are given together or not at all (irradiance 1)."""
    n, s = z.shape
    dev = z.device
    _chk(z, "z"), _chk(sigma, "sigma")
    weights = torch.empty(n, s, dtype=torch.float32, device=dev)
    transp = torch.empty(n, s, dtype=torch.float32, device=dev)
    depth = torch.empty(n, dtype=torch.float32, device=dev)
    rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
    _lib.call("sr_composite_fwd", _p(z), _p(sigma), _p(_chk(noise, "noise", allow_none=True)), float(noise_std), _p(_chk(albedo, "albedo", allow_none=True)),
              _p(_chk(sun_v, "sun_v", allow_none=True)), _p(_chk(sky_rgb, "sky", allow_none=True)), n, s, int(clamp_rgb), _p(weights), _p(transp),
              _p(depth), _p(rgb), _stream())
    return weights, transp, depth, rgb


def composite_bwd(z, sigma, noise, noise_std, albedo, sun_v, sky_rgb, weights, transp, g_rgb, g_depth, g_weights, g_transp, clamp_rgb=True):
    n, s = z.shape
    dev = z.device
    d_sigma = torch.empty(n, s, dtype=torch.float32, device=dev)
    d_albedo = torch.empty(n, s, 3, dtype=torch.float32, device=dev)
    d_sun = torch.empty(n, s, dtype=torch.float32, device=dev)
    d_sky = torch.empty(n, 3, dtype=torch.float32, device=dev)
    opt = lambda t, nm: _p(_chk(t, nm, allow_none=True))  # noqa: E731
    _lib.call("sr_composite_bwd", _p(z), _p(sigma), opt(noise, "noise"), float(noise_std), _p(albedo), opt(sun_v, "sun_v"), opt(sky_rgb, "sky"),
              _p(weights), _p(transp), None, n, s, int(clamp_rgb), opt(g_rgb, "g_rgb"), opt(g_depth, "g_depth"), opt(g_weights, "g_weights"),
              opt(g_transp, "g_transparency"), _p(d_sigma), _p(d_albedo), _p(d_sun), _p(d_sky), _stream())
    return d_sigma, d_albedo, d_sun, d_sky


# ----------------------------------------------------------------------------------- layer-by-layer path (any width)
ACTS = {None: _lib.ACT_NONE, "none": _lib.ACT_NONE, "sin": _lib.ACT_SIN, "relu": _lib.ACT_RELU}
OUT_ACTS = {None: _lib.OUT_NONE, "none": _lib.OUT_NONE, "softplus": _lib.OUT_SOFTPLUS, "sigmoid": _lib.OUT_SIGMOID, "sigmoid_rgb": _lib.OUT_SIGMOID_RGB}


def _linear_srcs(srcs, n_points):
    """srcs: 1 or 2 tuples (x (rows, k) fp32 with unit inner stride, act, w0, row_div) -> ctypes array (keeps the tensors alive)."""
    if not 1 <= len(srcs) <= 2:
        raise ValueError("a linear layer takes one or two concatenated sources")
    arr = (_lib.LinearSrc * len(srcs))()
    for a, (x, act, w0, row_div) in zip(arr, srcs):
        if act not in ACTS:
            raise ValueError(f"unknown activation {act!r} (one of {sorted(k for k in ACTS if k)})")
        x, ld = _rows(x, "linear source", 1)
        if x.shape[0] * row_div < n_points:
            raise ValueError(f"linear source has {x.shape[0]} rows x row_div {row_div} < {n_points} points")
        a.x, a.ld, a.k, a.act, a.w0, a.row_div = x.data_ptr(), ld, x.shape[1], ACTS[act], float(w0), int(row_div)
    return arr


def linear_fwd(srcs, weight, bias, n_points, out_act=None):
    """One nn.Linear on the concatenation of ``srcs`` (activation applied on load) -> (P, n_out) fp32, see sr_linear_fwd."""
    if out_act not in OUT_ACTS:
        raise ValueError(f"unknown output activation {out_act!r} (one of {sorted(k for k in OUT_ACTS if k)})")
    arr = _linear_srcs(srcs, n_points)
    n_out = weight.shape[0]
    if weight.shape[1] != sum(x.shape[1] for x, *_ in srcs):
        raise ValueError(f"weight is {tuple(weight.shape)} but the sources have {sum(x.shape[1] for x, *_ in srcs)} columns")
    y = torch.empty(n_points, n_out, dtype=torch.float32, device=weight.device)
    _lib.call("sr_linear_fwd", arr, len(srcs), _p(_chk(weight, "weight")), _p(_chk(bias, "bias", allow_none=True)), n_points, n_out, OUT_ACTS[out_act],
              _p(y), n_out, _stream())
    return y


def linear_bwd_input(gy, y, out_act, weight, col0, target, n_points):
    """Gradient w.r.t. one source (pre-activation): (P, k); ``target`` = (x, act, w0, row_div) of that source."""
    arr = _linear_srcs([target], n_points if target[3] == 1 else target[0].shape[0] * target[3])
    k = target[0].shape[1]
    d = torch.empty(n_points, k, dtype=torch.float32, device=gy.device)
    _lib.call("sr_linear_bwd_input", _p(_chk(gy, "gy")), gy.shape[1], _p(_chk(y, "y", allow_none=True)), 0 if y is None else y.shape[1], OUT_ACTS[out_act],
              _p(_chk(weight, "weight")), weight.shape[1], col0, arr, n_points, weight.shape[0], _p(d), k, _stream())
    return d


def linear_bwd_weight(gy, y, out_act, srcs, n_points, n_out, want_bias=True):
    arr = _linear_srcs(srcs, n_points)
    k = sum(x.shape[1] for x, *_ in srcs)
    dw = torch.zeros(n_out, k, dtype=torch.float32, device=gy.device)
    db = torch.zeros(n_out, dtype=torch.float32, device=gy.device) if want_bias else None
    _lib.call("sr_linear_bwd_weight", _p(_chk(gy, "gy")), gy.shape[1], _p(_chk(y, "y", allow_none=True)), 0 if y is None else y.shape[1], OUT_ACTS[out_act],
              arr, len(srcs), n_points, n_out, _p(dw), _p(db), _stream())
    return dw, db


def positional_map(x, n_freqs):
    """``Mapping.forward`` (models/nerf.py:53-69): (rows, dim) -> (rows, 2*n_freqs*dim)."""
    x, ld = _rows(x, "x", 1)
    out = torch.empty(x.shape[0], 2 * n_freqs * x.shape[1], dtype=torch.float32, device=x.device)
    _lib.call("sr_positional_map", _p(x), ld, x.shape[1], x.shape[0], n_freqs, _p(out), _stream())
    return out


def points_along(rays, dir_col, z):
    """xyz (N*S, 3) = rays[:, 0:3] + rays[:, dir_col:dir_col+3] * z (rendering.py:81)."""
    rays, stride = _rows(rays, "rays", dir_col + 3)
    n, s = z.shape
    xyz = torch.empty(n * s, 3, dtype=torch.float32, device=rays.device)
    _lib.call("sr_points_along", _p(rays), stride, dir_col, _p(_chk(z, "z")), n, s, _p(xyz), _stream())
    return xyz


# ----------------------------------------------------------------------------------- fused classic NeRF (csrc/nerf_fwd.inc)
def nerf_fused_ok(model, mode):
    """True when the one-launch classic-NeRF forward serves ``model`` in numeric mode ``mode``: single-pass bf16 at the shape of
    models/__init__.py:8 (a width the library has a stream for, 8 layers, skip at 4, mapping sizes [10, 4])."""
    return (mode == "bf16" and model.layers == 8 and list(model.skips) == [4] and list(model.mapping_sizes) == [10, 4]
            and _lib.lib().sr_nerf_stream_elems(int(model.feat)) > 0)


def nerf_render_ok(n_samples):
    """True when sr_nerf_render_fwd takes ``n_samples`` samples per ray (a workgroup composites whole rays)."""
    return 2 <= int(n_samples) <= _lib.lib().sr_nerf_render_max_samples()


def _nerf_stream(stream, feat=256):
    _chk(stream, "stream", torch.int16)
    if stream.numel() != _lib.lib().sr_nerf_stream_elems(feat):
        raise ValueError(f"stream holds {stream.numel()} elements, sr_nerf_stream_elems({feat}) = {_lib.lib().sr_nerf_stream_elems(feat)}")
    return stream


def nerf_mlp(xyz, dirs, row_div, stream):
    """Fused classic ``NeRF.forward`` (models/nerf.py:184-227) in bf16: xyz (P,3) per point, dirs (rows,3) read at row p // row_div;
    ``stream`` = ``NeRF.packed('bf16')``.  Returns rgb (P,3), sigma (P,)."""
    xyz, sx = _rows(xyz, "xyz", 3)
    dirs, sd = _rows(dirs, "dirs", 3)
    p, row_div = xyz.shape[0], int(row_div)
    if row_div < 1 or dirs.shape[0] * row_div < p:
        raise ValueError(f"dirs has {dirs.shape[0]} rows x row_div {row_div} < {p} points")
    _nerf_stream(stream)
    rgb = torch.empty(p, 3, dtype=torch.float32, device=xyz.device)
    sigma = torch.empty(p, dtype=torch.float32, device=xyz.device)
    if p:
        _lib.call("sr_nerf_mlp_fwd", _p(xyz), sx, _p(dirs), sd, row_div, p, 256, _p(stream), _p(rgb), _p(sigma), _stream())
    return rgb, sigma


def nerf_render_fwd(rays, n_samples, stream, u=None, z=None, noise=None, noise_std=0.0, want_z=False):
    """One pass of the classic render in ONE launch (sr_nerf_render_fwd): depths (stratified from ``u`` (N,S), or ``z`` (N,S) as given)
    -> points -> fused NeRF -> classic compositing (no sun, no sky, no clamp).  ``noise`` (N,S) is added to sigma times ``noise_std``.
    Returns dict(rgb (N,3), depth (N,), weights, transparency (N,S), z (N,S) = the given ``z``, the depths drawn if ``want_z``, else None)."""
    rays, stride = _rows(rays, "rays", 8)
    n, s, dev = rays.shape[0], int(n_samples), rays.device
    if (u is None) == (z is None):
        raise ValueError("exactly one of u (stratified depths) and z (given depths) is required")
    if not nerf_render_ok(s):
        raise ValueError(f"n_samples={s} unsupported (2..{_lib.lib().sr_nerf_render_max_samples()})")
    for t, nm in ((z, "z"), (u, "u"), (noise, "noise")):
        if t is not None and tuple(_chk(t, nm).shape) != (n, s):
            raise ValueError(f"{nm} must be ({n},{s}), got {tuple(t.shape)}")
    _nerf_stream(stream)
    e = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
    out = {"rgb": e(n, 3), "depth": e(n), "weights": e(n, s), "transparency": e(n, s), "z": z if z is not None else (e(n, s) if want_z else None)}
    if n:
        _lib.call("sr_nerf_render_fwd", _p(rays), stride, n, s, _p(u), _p(z), _p(noise), float(noise_std), 256, _p(stream),
                  _p(out["z"]) if z is None else None, _p(out["rgb"]), _p(out["depth"]), _p(out["weights"]), _p(out["transparency"]), _stream())
    return out


IMAGE_COLUMNS = {"rgb": (0, 3), "depth": (3, 4), "acc": (4, 5), "sun": (5, 6), "albedo": (6, 9), "beta": (9, 10), "sky": (10, 13)}


def composite_image(z, sigma, noise, noise_std, albedo, sun_v, beta, sky_rgb):
    """Compositing reduced to the per-pixel images of eval_satnerf.save_nerf_output_to_images: (N,13), see IMAGE_COLUMNS."""
    n, s = z.shape
    image = torch.empty(n, 13, dtype=torch.float32, device=z.device)
    _lib.call("sr_composite_image", _p(_chk(z, "z")), _p(_chk(sigma, "sigma")), _p(_chk(noise, "noise", allow_none=True)), float(noise_std),
              _p(_chk(albedo, "albedo")), _p(_chk(sun_v, "sun_v")), _p(_chk(beta, "beta")), _p(_chk(sky_rgb, "sky")), n, s, _p(image), _stream())
    return image


def latlonalt_from_depth(rays, depth, center, scene_range):
    """(lat, lon, alt) fp64 device tensors of the points rays_o + rays_d * depth, de-normalised by ``scene_range`` / ``center``."""
    import ctypes

    rays, stride = _rows(rays, "rays", 6)
    n = rays.shape[0]
    if depth.reshape(-1).shape[0] != n:
        raise ValueError("depth must have one value per ray")
    depth = _chk(depth.reshape(-1).contiguous().float(), "depth")
    c = (ctypes.c_double * 3)(*[float(v) for v in center])
    out = torch.empty(3, n, dtype=torch.float64, device=rays.device)
    _lib.call("sr_latlonalt_from_depth", _p(rays), stride, _p(depth), n, ctypes.addressof(c), float(scene_range), out[0].data_ptr(),
              out[1].data_ptr(), out[2].data_ptr(), _stream())
    return out[0], out[1], out[2]


RPC_KEYS = ("row_num", "row_den", "col_num", "col_den")
RPC_SCALARS = ("row_offset", "col_offset", "lat_offset", "lon_offset", "alt_offset", "row_scale", "col_scale", "lat_scale", "lon_scale", "alt_scale")


def rpc_rays(rpc, width, height, min_alt, max_alt, center, scene_range, sun_elevation_deg, sun_azimuth_deg, device, want_cache=False,
             out=None):
    """RPC ray generation of one image on the GPU (sr_rpc_rays): ``rpc`` = dict in rpcm's "rpcm" format (20-term lists row_num,
    row_den, col_num, col_den + the ten offsets / scales).  Returns (rays (H*W, 11) fp32, cache (H*W, 8) fp32 or None); ``out`` = a
    contiguous (H*W, 11) fp32 tensor on ``device`` to write the rays into (e.g. one image's rows of a dataset's ray tensor)."""
    buf = rpc_buffer(rpc)
    ctr = (C.c_double * 3)(*[float(v) for v in center])
    n = int(width) * int(height)
    dev = torch.device(device)
    with torch.cuda.device(dev):
        rays = torch.empty(n, 11, dtype=torch.float32, device=dev) if out is None else _chk(out, "out")
        if tuple(rays.shape) != (n, 11):
            raise ValueError(f"out must be ({n}, 11), got {tuple(rays.shape)}")
        cache = torch.empty(n, 8, dtype=torch.float32, device=dev) if want_cache else None
        _lib.call("sr_rpc_rays", C.addressof(buf), int(width), int(height), float(min_alt), float(max_alt), C.addressof(ctr),
                  float(scene_range), float(sun_elevation_deg), float(sun_azimuth_deg), _p(rays), _p(cache), _stream())
    return rays, cache


def rpc_scene_bounds(rpc, width, height, min_alt, max_alt, device, out=None, n_bad=None):
    """sr_rpc_scene_bounds: the ECEF bounds of one image's rays, near and far points.  Returns (bounds (6,) fp32 = [xmin, xmax, ymin,
    ymax, zmin, zmax], n_bad int64 with one element = the pixels with a non-finite coordinate, which count in no bound) on ``device``;
    ``out`` / ``n_bad`` = tensors of that size to write into (e.g. row k of a per-image table).  Nothing is read back."""
    buf = rpc_buffer(rpc)
    dev = torch.device(device)
    with torch.cuda.device(dev):
        out = torch.empty(6, dtype=torch.float32, device=dev) if out is None else _chk(out, "out")
        n_bad = torch.empty(1, dtype=torch.int64, device=dev) if n_bad is None else _chk(n_bad, "n_bad", torch.int64)
        if out.numel() != 6 or n_bad.numel() != 1:
            raise ValueError(f"out must hold 6 floats and n_bad one int64, got {tuple(out.shape)} and {tuple(n_bad.shape)}")
        _lib.call("sr_rpc_scene_bounds", C.addressof(buf), int(width), int(height), float(min_alt), float(max_alt), _p(out), _p(n_bad),
                  _stream())
    return out, n_bad


def rpc_buffer(rpc):
    """The 90 HOST doubles of an "rpcm"-format RPC dict in the C ABI's order (include/satrender.h, sr_rpc_rays)."""
    vals = []
    for k in RPC_KEYS:
        c = [float(v) for v in rpc[k]]
        if len(c) != 20:
            raise ValueError(f"rpc[{k!r}] must hold the 20 RPC00B coefficients, got {len(c)}")
        vals += c
    vals += [float(rpc[k]) for k in RPC_SCALARS]
    return (C.c_double * 90)(*vals)


def _colrow(colrow):
    colrow = _chk(colrow, "colrow", torch.float64)
    if colrow.dim() != 2 or colrow.shape[1] != 2:
        raise ValueError(f"colrow must be (n, 2) = (col, row) pairs, got {tuple(colrow.shape)}")
    return colrow


def _pts3d(pts3d):
    pts3d = _chk(pts3d, "pts3d", torch.float64)
    if pts3d.dim() != 2 or pts3d.shape[1] != 3:
        raise ValueError(f"pts3d must be (n_pts, 3) ECEF points, got {tuple(pts3d.shape)}")
    return pts3d


def _index(idx, n, name="pts3d_idx"):
    idx = _chk(idx, name, torch.int64)
    if idx.dim() != 1 or idx.numel() != n:
        raise ValueError(f"{name} must be ({n},), got {tuple(idx.shape)}")
    return idx


def rpc_rays_at(rpc, colrow, min_alt, max_alt, center, scene_range, sun_elevation_deg, sun_azimuth_deg, out=None):
    """sr_rpc_rays_at: the (n, 11) fp32 normalised rays of one image at n (col, row) points (``colrow``: (n, 2) fp64 device tensor)."""
    colrow = _colrow(colrow)
    n = colrow.shape[0]
    out = torch.empty(n, 11, dtype=torch.float32, device=colrow.device) if out is None else _chk(out, "out")
    if tuple(out.shape) != (n, 11):
        raise ValueError(f"out must be ({n}, 11), got {tuple(out.shape)}")
    buf, ctr = rpc_buffer(rpc), (C.c_double * 3)(*[float(v) for v in center])
    _lib.call("sr_rpc_rays_at", C.addressof(buf), _p(colrow), n, float(min_alt), float(max_alt), C.addressof(ctr), float(scene_range),
              float(sun_elevation_deg), float(sun_azimuth_deg), _p(out), _stream())
    return out


def reprojection_errors(rpc, colrow, pts3d_idx, pts3d, out=None):
    """sr_reprojection_errors: (n,) fp32 pixel distance between each keypoint and the RPC projection of its tie point."""
    colrow, pts3d = _colrow(colrow), _pts3d(pts3d)
    n = colrow.shape[0]
    pts3d_idx = _index(pts3d_idx, n)
    out = torch.empty(n, dtype=torch.float32, device=colrow.device) if out is None else _chk(out, "out")
    if out.numel() != n:
        raise ValueError(f"out must hold {n} floats")
    buf = rpc_buffer(rpc)
    _lib.call("sr_reprojection_errors", C.addressof(buf), _p(colrow), _p(pts3d_idx), n, _p(pts3d), pts3d.shape[0], _p(out), _stream())
    return out


def keypoint_weights_scratch(n_pts, n_cams):
    """Bytes of scratch sr_keypoint_weights needs (host only)."""
    return _scratch_bytes("sr_keypoint_weights_scratch", n_pts, n_cams)


def keypoint_weights(pts3d_idx, cam, err, n_pts, n_cams, scratch=None):
    """sr_keypoint_weights over all observations: returns (e (n_pts,), w (n_pts,), e_mean (1,)) fp32 device tensors.  Nothing is
    read back."""
    err = _chk(err, "err")
    n = err.numel()
    pts3d_idx, cam = _index(pts3d_idx, n), _index(cam, n, "cam")
    dev = err.device
    scratch = _metric_scratch(scratch, keypoint_weights_scratch(n_pts, n_cams), dev)
    e = torch.empty(int(n_pts), dtype=torch.float32, device=dev)
    w = torch.empty_like(e)
    e_mean = torch.empty(1, dtype=torch.float32, device=dev)
    _lib.call("sr_keypoint_weights", _p(pts3d_idx), _p(cam), _p(err), n, int(n_pts), int(n_cams), _p(scratch),
              scratch.numel() * scratch.element_size(), _p(e), _p(w), _p(e_mean), _stream())
    return e, w, e_mean


def tie_point_depths(rays, pts3d, pts3d_idx, center, scene_range, w=None, out=None):
    """sr_tie_point_depths: (n, 2) fp32 [target depth, w[idx]] of the n rays (columns 0..2 = normalised origins)."""
    rays, pts3d = _chk(rays, "rays"), _pts3d(pts3d)
    if rays.dim() != 2 or rays.shape[1] != 11:
        raise ValueError(f"rays must be (n, 11), got {tuple(rays.shape)}")
    n = rays.shape[0]
    pts3d_idx = _index(pts3d_idx, n)
    if w is not None and (_chk(w, "w").numel() != pts3d.shape[0]):
        raise ValueError(f"w must hold one weight per tie point ({pts3d.shape[0]})")
    out = torch.empty(n, 2, dtype=torch.float32, device=rays.device) if out is None else _chk(out, "out")
    if tuple(out.shape) != (n, 2):
        raise ValueError(f"out must be ({n}, 2), got {tuple(out.shape)}")
    ctr = (C.c_double * 3)(*[float(v) for v in center])
    _lib.call("sr_tie_point_depths", _p(rays), _p(pts3d), _p(pts3d_idx), n, pts3d.shape[0], C.addressof(ctr), float(scene_range), _p(w),
              _p(out), _stream())
    return out


def sample_pdf(bins, weights, u, eps=1e-5):
    n, nb = bins.shape
    _chk(bins, "bins"), _chk(weights, "weights"), _chk(u, "u")
    if tuple(weights.shape) != (n, nb - 1) or u.shape[0] != n:
        raise ValueError(f"sample_pdf: weights must be ({n},{nb - 1}) and u ({n},I)")
    out = torch.empty(n, u.shape[1], dtype=torch.float32, device=bins.device)
    _lib.call("sr_sample_pdf", _p(bins), _p(weights), _p(u), n, nb, u.shape[1], float(eps), _p(out), _stream())
    return out


def sample_pdf_merge(z_coarse, weights_coarse, u, eps=1e-5):
    n, s = z_coarse.shape
    i = u.shape[1]
    _chk(z_coarse, "z_coarse"), _chk(weights_coarse, "weights_coarse"), _chk(u, "u")
    if tuple(weights_coarse.shape) != (n, s) or u.shape[0] != n:
        raise ValueError("sample_pdf_merge: shape mismatch")
    z_fine = torch.empty(n, s + i, dtype=torch.float32, device=z_coarse.device)
    _lib.call("sr_sample_pdf_merge", _p(z_coarse), _p(weights_coarse), _p(u), n, s, i, float(eps), _p(z_fine), _stream())
    return z_fine


# ------------------------------------------------------------------------------------------------ backward
def graph_capture(graph):
    """``torch.cuda.graph(graph)``; under ``torch.distributed`` the capture is thread-local, so the process group's watchdog
    thread (which polls events of earlier collectives) cannot invalidate a capture in progress on this thread."""
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        return torch.cuda.graph(graph, capture_error_mode="thread_local")
    return torch.cuda.graph(graph)


def default_fmt(mode):
    """Workspace format of a numeric mode: the throughput mode trains on 8-bit saved state, the parity mode on 16-bit."""
    return 8 if mode in ("bf16", "f16") else 16


def _ws_empty(n, dtype, device, slot):
    """Workspace allocation; SATNERF_WS_PAD=<bytes> shifts workspace `slot` by slot * pad bytes (placement experiments)."""
    pad = int(os.environ.get("SATNERF_WS_PAD", "0")) * slot
    if not pad:
        return torch.empty(n, dtype=dtype, device=device)
    item = torch.empty((), dtype=dtype).element_size()
    return torch.empty(n + pad // item, dtype=dtype, device=device)[pad // item:]


def acts_workspace(n_points, feat, device, fmt=16):
    per_tile = _lib.lib().sr_act_elems_per_tile(feat, int(fmt))
    if per_tile <= 0:
        raise ValueError(f"unsupported workspace (feat={feat}, fmt={fmt})")
    return _ws_empty(_lib.lib().sr_workspace_tiles(n_points) * per_tile, torch.int16, device, 1)


def satnerf_mlp_bwd(feat, tau, n_points, bwd_stream, acts, albedo, sigma, sun_v, beta, g_albedo, g_sigma, g_sun_v, g_beta, want_dt=True, fmt=16):
    """dX chain: returns (dpre workspace, d_t (P,tau) or None); ``fmt`` = format of ``acts`` and of the returned workspace."""
    dev = albedo.device
    n_elems = _lib.lib().sr_dpre_workspace_elems(n_points, feat, int(fmt))  # (8-bit: + the table of exponent maxima behind the last tile)
    if n_elems <= 0:
        raise ValueError(f"unsupported workspace (feat={feat}, fmt={fmt})")
    dpre = _ws_empty(n_elems, torch.int16, dev, 2)
    d_t = torch.empty(n_points, tau, dtype=torch.float32, device=dev) if want_dt else None
    opt = lambda t, nm: _p(_chk(t, nm, allow_none=True))  # noqa: E731
    with _timed("mlp_bwd"):
        _lib.call("sr_satnerf_mlp_bwd", feat, tau, n_points, _p(bwd_stream), _p(acts), _p(_chk(albedo, "albedo")), _p(_chk(sigma, "sigma")),
                  _p(_chk(sun_v, "sun_v")), _p(_chk(beta, "beta")), opt(g_albedo, "g_albedo"), opt(g_sigma, "g_sigma"), opt(g_sun_v, "g_sun_v"),
                  opt(g_beta, "g_beta"), _p(dpre), _p(d_t), int(fmt), _stream())
    return dpre, d_t


_plan_cache = {}


def wgrad_plan(blocks, n_points, n_wg=0, fmt=16):
    """Split-K plan of the weight-gradient job table for ``n_points`` points (sr_wgrad_plan; ``fmt`` = workspace format of the kernel
    that will run it): returns (planned device table, total slices, span of a stream-K plan or 0).  Cached per (table, n_points, fmt): the copy to the device
    must not happen inside a graph capture."""
    key = (blocks.data_ptr(), int(n_points), int(n_wg), str(blocks.device), int(fmt))
    ent = _plan_cache.get(key)
    if ent is None:
        import ctypes

        host = _chk(blocks, "blocks", torch.int32).cpu().contiguous().clone()
        n_slices = ctypes.c_int(0)
        with torch.cuda.device(blocks.device):
            _lib.call("sr_wgrad_plan", host.data_ptr(), host.shape[0], n_points, n_wg, int(fmt), ctypes.addressof(n_slices))
        if len(_plan_cache) > 64:
            _plan_cache.clear()
        # (int 11 of the first row: the span of a stream-K plan, 0 otherwise -- the launch has to know which build of the kernel to run)
        ent = _plan_cache[key] = (host.to(blocks.device), int(n_slices.value), blocks, int(host[0, 11]))  # keeps `blocks` alive: data_ptr stays unique
    return ent[0], ent[1], ent[3]


def wgrad_partials(feat, tau, n_points, dpre, acts, blocks, fmt=16, loads=None, n_wg=0):
    """Weight-gradient GEMMs only: returns (fp32 split-K slices, planned job table); reduce with grad_tail / unpack_grads.
    ``fmt`` = format of both workspaces; the 8-bit kernel also needs the per-block load table ``loads`` (packing.wgrad8_loads).
    ``n_wg`` = workgroups the plan is made for (0: the device's CU count)."""
    plan, n_slices, span = wgrad_plan(blocks, n_points, n_wg=n_wg, fmt=fmt)
    block_floats = 256 * 256 + 256 * 32  # csrc/mlp_layout.h kWgBlockFloats
    partial = _ws_empty(n_slices * block_floats, torch.float32, dpre.device, 3)
    with _timed("wgrad"):
        if int(fmt) == 8:
            _lib.call("sr_satnerf_wgrad8", feat, tau, n_points, _p(dpre), dpre.numel(), _p(acts), _p(plan), _p(_chk(loads, "loads", torch.int32)), plan.shape[0],
                      n_slices, span, _p(partial), _stream())
        else:
            _lib.call("sr_satnerf_wgrad", feat, tau, n_points, _p(dpre), _p(acts), _p(plan), plan.shape[0], n_slices, _p(partial), _stream())
    return partial, plan


def satnerf_wgrad(feat, tau, n_points, dpre, acts, blocks, gidx, gscale, grad_flat, accumulate=True, fmt=16, loads=None):
    """Weight-gradient GEMMs + split-K reduction + scatter into the flat gradient buffer."""
    partial, plan = wgrad_partials(feat, tau, n_points, dpre, acts, blocks, fmt, loads)
    _lib.call("sr_unpack_grads", _p(partial), _p(_chk(gidx, "gidx", torch.int32)), _p(_chk(gscale, "gscale")), gidx.numel(), _p(plan),
              _p(_chk(grad_flat, "grad_flat")), int(accumulate), _stream())


def sky_bwd(sun, w1, b1, w2, sky_rgb, d_sky, g_w1, g_b1, g_w2, g_b2):
    sun, stride = _rows(sun, "sun", 3)
    _lib.call("sr_sky_bwd", _p(sun), stride, sun.shape[0], w1.shape[0], _p(w1), _p(b1), _p(w2), _p(_chk(sky_rgb, "sky")), _p(_chk(d_sky, "d_sky")),
              _p(g_w1), _p(g_b1), _p(g_w2), _p(g_b2), _stream())


def embedding_bwd(d_t, ts, n_rays, n_samples, tau, g_emb):
    _lib.call("sr_embedding_bwd", _p(_chk(d_t, "d_t")), _p(_chk(ts, "ts", torch.int64)), n_rays, n_samples, tau, _p(_chk(g_emb, "g_emb")), _stream())


def satnerf_loss(rgb, weights, beta, target, beta_min=0.05, grad_scale=1.0, sched=None):
    """Fused SatNerfLoss forward + gradient: returns (loss partial sums (ceil(N/4),) -- the loss is their sum --, g_rgb (N,3),
    g_weights (N,S), g_beta (N,S))."""
    n, s = weights.shape
    dev = rgb.device
    loss = torch.empty((n + 3) // 4, dtype=torch.float32, device=dev)
    g_rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
    g_w = torch.empty(n, s, dtype=torch.float32, device=dev)
    g_b = torch.empty(n, s, dtype=torch.float32, device=dev)
    _lib.call("sr_satnerf_loss", _p(_chk(rgb, "rgb")), _p(_chk(weights, "weights")), _p(_chk(beta, "beta")), _p(_chk(target, "target")), n, s,
              float(beta_min), float(grad_scale), _p(_chk(sched, "sched", allow_none=True)), _p(loss), _p(g_rgb), _p(g_w), _p(g_b), _stream())
    return loss, g_rgb, g_w, g_b


def adam_step(params, grads, exp_avg, exp_avg_sq, step, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, zero_grad=True):
    """``step`` is the 1-based step count (bias corrections are computed on the host in fp64)."""
    _lib.call("sr_adam_step", _p(_chk(params, "params")), _p(_chk(grads, "grads")), _p(_chk(exp_avg, "exp_avg")), _p(_chk(exp_avg_sq, "exp_avg_sq")),
              params.numel(), float(lr), float(betas[0]), float(betas[1]), float(eps), float(grad_scale), int(step), int(zero_grad), _stream())


def pack_all(flat, idx, scale, hi, lo, f32_idx, f32_scale, f32_out, tick=None, n_f16=0):
    """``n_f16``: the first n_f16 stream elements (the forward stream) are written as fp16 (SR_MODE_F16), the rest as bf16."""
    _lib.call("sr_pack_all", _p(_chk(flat, "flat")), _p(_chk(idx, "idx", torch.int32)), _p(_chk(scale, "scale")), idx.numel(), _p(hi), _p(lo),
              _p(_chk(f32_idx, "f32_idx", torch.int32)), _p(_chk(f32_scale, "f32_scale")), f32_idx.numel(), _p(f32_out), _p(tick), int(n_f16),
              _stream())


def sc_loss(z, sigma, noise, noise_std, sun_v, lambda_sc):
    """Solar-correction terms of the pass along the sun direction: (loss_parts, d_sun_v (N,S))."""
    n, s = z.shape
    parts = torch.empty((n + 3) // 4, dtype=torch.float32, device=z.device)
    d_sun = torch.empty(n, s, dtype=torch.float32, device=z.device)
    _lib.call("sr_sc_loss", _p(_chk(z, "z")), _p(_chk(sigma, "sigma")), _p(_chk(noise, "noise", allow_none=True)), float(noise_std),
              _p(_chk(sun_v, "sun_v")), n, s, float(lambda_sc), _p(parts), _p(d_sun), _stream())
    return parts, d_sun


def depth_loss(depth, depths, lambda_ds, use_weights=True):
    """metrics.DepthLoss (coarse) value parts + gradient w.r.t. the rendered depth: (loss_parts, g_depth (N,))."""
    depths, stride = _rows(depths, "depths", 2 if use_weights else 1)
    n = depth.shape[0]
    parts = torch.empty((n + 255) // 256, dtype=torch.float32, device=depth.device)
    g = torch.empty(n, dtype=torch.float32, device=depth.device)
    _lib.call("sr_depth_loss", _p(_chk(depth, "depth")), _p(depths), stride, int(use_weights), n, float(lambda_ds), _p(parts), _p(g), _stream())
    return parts, g


def ray_setup(rays, u, n_samples, w1, b1, w2, b2, seed=0, step_counter=None, tick=False):
    """Fused sr_ray_sample_fwd + sr_sky_fwd: returns (z (N,S), sky (N,3)).  ``u`` = (N,S) uniform jitter, or None to draw it inside
    the kernel (Philox keyed by ``seed``, stepping with the device counter ``step_counter[0]``; ``tick``: the launch advances the
    counter itself -- ``step_counter`` is then a zero-initialised 4-float block)."""
    rays, stride = _rows(rays, "rays", 11)
    n = rays.shape[0]
    z = torch.empty(n, n_samples, dtype=torch.float32, device=rays.device)
    sky_rgb = torch.empty(n, 3, dtype=torch.float32, device=rays.device)
    w = (_p(_chk(w1, "w1")), _p(_chk(b1, "b1")), _p(_chk(w2, "w2")), _p(_chk(b2, "b2")))
    if u is None:
        if tick and (step_counter is None or step_counter.numel() < 4):
            raise ValueError("tick=True needs step_counter = a zero-initialised float32 block of 4")
        _lib.call("sr_ray_setup_rng", _p(rays), stride, int(seed) & 0xFFFFFFFFFFFFFFFF, _p(_chk(step_counter, "step_counter", allow_none=True)),
                  int(bool(tick)), n, n_samples, w1.shape[0], *w, _p(z), _p(sky_rgb), _stream())
    else:
        _lib.call("sr_ray_setup", _p(rays), stride, _p(_chk(u, "u")), n, n_samples, w1.shape[0], *w, _p(z), _p(sky_rgb), _stream())
    return z, sky_rgb


def render_loss(z, sigma, noise, noise_std, albedo, sun_v, beta, sky_rgb, target, beta_min=0.05, sched=None):
    """Fused compositing forward + SatNerf loss + compositing backward (S <= 64).
    Returns (loss partial sums, rgb (N,3), d_sigma (N,S), d_albedo (N,S,3), d_sun (N,S), g_beta (N,S), d_sky (N,3))."""
    n, s = z.shape
    dev = z.device
    e = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
    loss, rgb, d_sigma, d_albedo, d_sun, g_beta, d_sky = e((n + 3) // 4), e(n, 3), e(n, s), e(n, s, 3), e(n, s), e(n, s), e(n, 3)
    _lib.call("sr_render_loss", _p(_chk(z, "z")), _p(_chk(sigma, "sigma")), _p(_chk(noise, "noise", allow_none=True)), float(noise_std),
              _p(_chk(albedo, "albedo")), _p(_chk(sun_v, "sun_v")), _p(_chk(beta, "beta")), _p(_chk(sky_rgb, "sky")), _p(_chk(target, "target")), n, s,
              float(beta_min), _p(_chk(sched, "sched", allow_none=True)), _p(loss), _p(rgb), _p(d_sigma), _p(d_albedo), _p(d_sun), _p(g_beta), _p(d_sky),
              _stream())
    return loss, rgb, d_sigma, d_albedo, d_sun, g_beta, d_sky


def gather_batch(rays, rgbs, ts, idx, out=None, cursor=None, batches=0):
    """Rows ``idx`` of the ray bank -> (rays (B,11), ts (B,), rgbs (B,3)), one launch.  With ``cursor`` (zeros(4) float32) ``idx``
    holds a whole epoch of ``batches`` x B indices: the launch takes batch cursor[0] and advances the cursor (captured steps)."""
    n = idx.numel()
    if cursor is not None:
        if batches < 1 or n % batches or cursor.numel() < 4:
            raise ValueError("cursor mode: idx must hold batches x B indices and cursor 4 floats")
        n //= batches
    if rays.shape[1] != 11 or rgbs.shape[1] != 3:
        raise ValueError("gather_batch expects (N,11) rays and (N,3) rgbs")
    if out is None:
        out = (torch.empty(n, 11, dtype=torch.float32, device=rays.device), torch.empty(n, dtype=torch.int64, device=rays.device),
               torch.empty(n, 3, dtype=torch.float32, device=rays.device))
    _lib.call("sr_gather_batch", _p(_chk(rays, "rays")), _p(_chk(rgbs, "rgbs")), _p(_chk(ts, "ts", torch.int64)), _p(_chk(idx, "idx", torch.int64)), n,
              _p(_chk(out[0], "out_rays")), _p(_chk(out[2], "out_rgbs")), _p(_chk(out[1], "out_ts", torch.int64)),
              _p(_chk(cursor, "cursor", allow_none=True)), int(batches), _stream())
    return out


def gather_setup(rays, rgbs, ts, idx, out, n_samples, w1, b1, w2, b2, z, sky_rgb, seed, step_counter, step_offset=1, cursor=None, batches=0):
    """``gather_batch`` + ``ray_setup`` (in-kernel jitter) in one launch: rows -> ``out`` = (rays, ts, rgbs), depths -> ``z`` (B,S),
    sky colour -> ``sky_rgb`` (B,3); the jitter step is step_counter[0] + step_offset."""
    n = idx.numel()
    if cursor is not None:
        if batches < 1 or n % batches or cursor.numel() < 4:
            raise ValueError("cursor mode: idx must hold batches x B indices and cursor 4 floats")
        n //= batches
    if out[0].shape[0] != n or tuple(z.shape) != (n, n_samples) or tuple(sky_rgb.shape) != (n, 3):
        raise ValueError("gather_setup: output shapes do not match the batch")
    _lib.call("sr_gather_setup", _p(_chk(rays, "rays")), _p(_chk(rgbs, "rgbs")), _p(_chk(ts, "ts", torch.int64)), _p(_chk(idx, "idx", torch.int64)), n,
              _p(_chk(out[0], "out_rays")), _p(_chk(out[2], "out_rgbs")), _p(_chk(out[1], "out_ts", torch.int64)),
              _p(_chk(cursor, "cursor", allow_none=True)), int(batches), int(n_samples), w1.shape[0], _p(_chk(w1, "w1")), _p(_chk(b1, "b1")),
              _p(_chk(w2, "w2")), _p(_chk(b2, "b2")), _p(_chk(z, "z")), _p(_chk(sky_rgb, "sky")), int(seed) & 0xFFFFFFFFFFFFFFFF,
              _p(_chk(step_counter, "step_counter", allow_none=True)), int(step_offset), _stream())


def _grad_tail_args(partial, plan, gidx, gscale, grad_flat, sun, w1, b1, w2, sky_rgb, d_sky, g_w1, g_b1, g_w2, g_b2, d_t, ts, n_rays, n_samples, tau,
                    g_emb):
    """The sr_grad_tail_args of the four tail wrappers (their first 21 arguments); it holds addresses only: the tensors are the caller's."""
    sun, stride = _rows(sun, "sun", 3)
    return _lib.GradTailArgs(
        partial=_p(partial), gidx=_p(_chk(gidx, "gidx", torch.int32)), gscale=_p(_chk(gscale, "gscale")), n_params=gidx.numel(), blocks=_p(plan),
        n_blocks=plan.shape[0], grad=_p(_chk(grad_flat, "grad_flat")), accumulate=1, sun=_p(sun), sun_stride=stride, n_rays=n_rays,
        hidden=w1.shape[0], w1=_p(w1), b1=_p(b1), w2=_p(w2), sky=_p(_chk(sky_rgb, "sky")), d_sky=_p(_chk(d_sky, "d_sky")), g_w1=_p(g_w1),
        g_b1=_p(g_b1), g_w2=_p(g_w2), g_b2=_p(g_b2), d_t=_p(_chk(d_t, "d_t")), ts=_p(_chk(ts, "ts", torch.int64)), n_samples=n_samples, tau=tau,
        g_emb=_p(_chk(g_emb, "g_emb")))


def _tail_adam_args(n_params, params, exp_avg, exp_avg_sq, late_idx, state, lr, betas, eps, grad_scale, pack):
    """The sr_tail_adam_args of the two tail + Adam wrappers; the struct keeps its PackScatter alive."""
    ps = C.pointer(_pack_scatter_struct(pack, n_params)) if pack is not None else None
    return _lib.TailAdamArgs(
        params=_p(_chk(params, "params")), exp_avg=_p(_chk(exp_avg, "exp_avg")), exp_avg_sq=_p(_chk(exp_avg_sq, "exp_avg_sq")),
        late_idx=_p(_chk(late_idx, "late_idx", torch.int32)), n_late=late_idx.numel(), state=_p(_chk(state, "state")), lr=float(lr),
        beta1=float(betas[0]), beta2=float(betas[1]), eps=float(eps), grad_scale=float(grad_scale), pack=ps)


def grad_tail(partial, plan, gidx, gscale, grad_flat, sun, w1, b1, w2, sky_rgb, d_sky, g_w1, g_b1, g_w2, g_b2, d_t, ts, n_rays,
              n_samples, tau, g_emb):
    args = _grad_tail_args(partial, plan, gidx, gscale, grad_flat, sun, w1, b1, w2, sky_rgb, d_sky, g_w1, g_b1, g_w2, g_b2, d_t, ts, n_rays,
                           n_samples, tau, g_emb)
    _lib.call("sr_grad_tail", C.byref(args), _stream())


def grad_tail_adam(partial, plan, gidx, gscale, grad_flat, sun, w1, b1, w2, sky_rgb, d_sky, g_w1, g_b1, g_w2, g_b2, d_t, ts, n_rays, n_samples, tau,
                   g_emb, params, exp_avg, exp_avg_sq, late_idx, state, lr=-1.0, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, pack=None):
    """``grad_tail`` + ``adam_step_graph`` in one launch (sr_grad_tail_adam): ``params`` / ``exp_avg`` / ``exp_avg_sq`` are the flat buffers
    aligned with ``grad_flat`` (they may extend past it: ``late_idx`` addresses the embedding rows behind the model's parameters).
    ``pack`` (``SatNeRF.pack_scatter``): the launch also writes every updated parameter into the weight streams (no sr_pack_all next step)."""
    args = _grad_tail_args(partial, plan, gidx, gscale, grad_flat, sun, w1, b1, w2, sky_rgb, d_sky, g_w1, g_b1, g_w2, g_b2, d_t, ts, n_rays,
                           n_samples, tau, g_emb)
    adam = _tail_adam_args(gidx.numel(), params, exp_avg, exp_avg_sq, late_idx, state, lr, betas, eps, grad_scale, pack)
    _lib.call("sr_grad_tail_adam", C.byref(args), C.byref(adam), _stream())


# ---- fixed-order sky and embedding gradients (include/satrender.h: the *_det entry points) ---------------------------------------------
def late_grad_scratch_bytes(n_rays, hidden, tau):
    """Size in bytes of the scratch of the ``*_det`` launches (sr_late_grad_scratch_bytes, host only)."""
    n = int(_lib.lib().sr_late_grad_scratch_bytes(int(n_rays), int(hidden), int(tau)))
    if n < 0:
        raise ValueError(f"late_grad_scratch_bytes: n_rays={n_rays}, hidden={hidden}, tau={tau}")
    return n


def late_grad_scratch(n_rays, hidden, tau, device):
    """The scratch of the ``*_det`` launches for batches of up to ``n_rays`` rays: a zeroed float32 buffer (word 0 is the arrival counter, which
    every launch leaves at zero) that may be reused for every step."""
    return torch.zeros(late_grad_scratch_bytes(n_rays, hidden, tau) // 4, dtype=torch.float32, device=device)


def _late_scratch(scratch, need=None):
    """(pointer, size in bytes) of a ``*_det`` launch's scratch; ``need``: the bytes the launch asks for when the caller knows them (the
    library checks in any case)."""
    scratch = _chk(scratch, "scratch")
    if need is not None and scratch.numel() * 4 < need:
        raise ValueError(f"scratch holds {scratch.numel() * 4} bytes, the launch needs {need} (late_grad_scratch)")
    return _p(scratch), scratch.numel() * 4


def sky_bwd_det(sun, w1, b1, w2, sky_rgb, d_sky, g_w1, g_b1, g_w2, g_b2, scratch):
    """``sky_bwd`` with the per-block sums stored in ``scratch`` and added up in block order by the last block (sr_sky_bwd_det)."""
    sun, stride = _rows(sun, "sun", 3)
    _lib.call("sr_sky_bwd_det", _p(sun), stride, sun.shape[0], w1.shape[0], _p(w1), _p(b1), _p(w2), _p(_chk(sky_rgb, "sky")), _p(_chk(d_sky, "d_sky")),
              _p(g_w1), _p(g_b1), _p(g_w2), _p(g_b2), *_late_scratch(scratch), _stream())


def embedding_bwd_det(d_t, ts, n_rays, n_samples, tau, g_emb, scratch):
    """``embedding_bwd`` with the per-ray sums stored in ``scratch`` and added up in ray order by the last block (sr_embedding_bwd_det)."""
    _lib.call("sr_embedding_bwd_det", _p(_chk(d_t, "d_t")), _p(_chk(ts, "ts", torch.int64)), n_rays, n_samples, tau, _p(_chk(g_emb, "g_emb")),
              *_late_scratch(scratch), _stream())


def grad_tail_det(partial, plan, gidx, gscale, grad_flat, sun, w1, b1, w2, sky_rgb, d_sky, g_w1, g_b1, g_w2, g_b2, d_t, ts, n_rays,
                  n_samples, tau, g_emb, scratch):
    """``grad_tail`` whose sky and embedding gradients are summed in a fixed order (sr_grad_tail_det); ``scratch``: ``late_grad_scratch``."""
    args = _grad_tail_args(partial, plan, gidx, gscale, grad_flat, sun, w1, b1, w2, sky_rgb, d_sky, g_w1, g_b1, g_w2, g_b2, d_t, ts, n_rays,
                           n_samples, tau, g_emb)
    _lib.call("sr_grad_tail_det", C.byref(args), *_late_scratch(scratch, late_grad_scratch_bytes(n_rays, w1.shape[0], tau)), _stream())


def grad_tail_adam_det(partial, plan, gidx, gscale, grad_flat, sun, w1, b1, w2, sky_rgb, d_sky, g_w1, g_b1, g_w2, g_b2, d_t, ts, n_rays, n_samples,
                       tau, g_emb, params, exp_avg, exp_avg_sq, late_idx, state, scratch, lr=-1.0, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0,
                       pack=None):
    """``grad_tail_adam`` whose sky and embedding gradients are summed in a fixed order before the last block updates the ``late_idx``
    parameters (sr_grad_tail_adam_det); ``scratch``: ``late_grad_scratch``.  The arrival counter is ``state[3]``, as in ``grad_tail_adam``."""
    args = _grad_tail_args(partial, plan, gidx, gscale, grad_flat, sun, w1, b1, w2, sky_rgb, d_sky, g_w1, g_b1, g_w2, g_b2, d_t, ts, n_rays,
                           n_samples, tau, g_emb)
    adam = _tail_adam_args(gidx.numel(), params, exp_avg, exp_avg_sq, late_idx, state, lr, betas, eps, grad_scale, pack)
    need = late_grad_scratch_bytes(n_rays, w1.shape[0], tau)
    _lib.call("sr_grad_tail_adam_det", C.byref(args), C.byref(adam), *_late_scratch(scratch, need), _stream())


def _pack_scatter_struct(pack, n_model):
    if pack["map"].shape != (n_model, 2):
        raise ValueError("pack map does not match the parameter count")
    return _lib.PackScatter(_p(_chk(pack["map"], "pack map", torch.int32)), _p(pack["hi"]), _p(pack["lo"]), _p(_chk(pack["l0"], "pack l0")),
                            int(pack["n_f16"]), (C.c_float * 4)(*[float(x) for x in pack["scales"]]))


def adam_step_pack(params, grads, exp_avg, exp_avg_sq, state, pack=None, lr=-1.0, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, zero_grad=True):
    """``adam_step_graph`` that also writes the first ``pack['map'].shape[0]`` parameters (the coarse model's) into the weight streams
    (sr_adam_step_pack): the update launch of a data-parallel step, issued after the gradient all-reduce."""
    ps = _pack_scatter_struct(pack, pack["map"].shape[0]) if pack is not None else None
    _lib.call("sr_adam_step_pack", _p(_chk(params, "params")), _p(_chk(grads, "grads")), _p(_chk(exp_avg, "exp_avg")), _p(_chk(exp_avg_sq, "exp_avg_sq")),
              params.numel(), float(lr), float(betas[0]), float(betas[1]), float(eps), float(grad_scale), _p(_chk(state, "state")), int(zero_grad),
              0 if pack is None else pack["map"].shape[0], C.byref(ps) if ps is not None else None, _stream())


def adam_step_graph(params, grads, exp_avg, exp_avg_sq, state, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, zero_grad=True):
    _lib.call("sr_adam_step_graph", _p(_chk(params, "params")), _p(_chk(grads, "grads")), _p(_chk(exp_avg, "exp_avg")), _p(_chk(exp_avg_sq, "exp_avg_sq")),
              params.numel(), float(lr), float(betas[0]), float(betas[1]), float(eps), float(grad_scale), _p(_chk(state, "state")), int(zero_grad),
              _stream())


# ---- DSM extraction (csrc/dsm.hip) ----------------------------------------------------------------------------------------------------
def utm_zone(lat, lon):
    """(zone number, band letter) of one point by the utm package's rules (sr_utm_zone, host only); raises unless -80 <= lat <= 84."""
    zone, letter = C.c_int(0), C.c_int(0)
    _lib.call("sr_utm_zone", float(lat), float(lon), C.byref(zone), C.byref(letter))
    return zone.value, chr(letter.value)


def utm_from_latlon(lats, lons, zone):
    """(east, north) fp64 device tensors of fp64 device lat / lon (degrees) in UTM zone ``zone`` (1..60)."""
    lats, lons = _chk(lats.contiguous(), "lats", torch.float64), _chk(lons.contiguous(), "lons", torch.float64)
    if lats.dim() != 1 or lats.shape != lons.shape:
        raise ValueError(f"lats / lons must be two (N,) tensors, got {tuple(lats.shape)} / {tuple(lons.shape)}")
    out = torch.empty(2, lats.shape[0], dtype=torch.float64, device=lats.device)
    _lib.call("sr_utm_from_latlon", _p(lats), _p(lons), lats.shape[0], int(zone), out[0].data_ptr(), out[1].data_ptr(), _stream())
    return out[0], out[1]


def depth_to_utm(rays, depth, center, scene_range, zone=0):
    """(east, north, alt) fp64 device tensors of the points rays_o + rays_d * depth, and a (2,) int32 device tensor {zone number,
    letter code} of ray 0's point (zone > 0 overrides the number; number 0 = ray 0's point is unusable)."""
    rays, stride = _rows(rays, "rays", 6)
    n = rays.shape[0]
    if depth.reshape(-1).shape[0] != n:
        raise ValueError("depth must have one value per ray")
    depth = _chk(depth.reshape(-1).contiguous(), "depth")
    c = (C.c_double * 3)(*[float(v) for v in center])
    out = torch.empty(3, n, dtype=torch.float64, device=rays.device)
    zone_out = torch.zeros(2, dtype=torch.int32, device=rays.device)
    _lib.call("sr_depth_to_utm", _p(rays), stride, _p(depth), n, C.addressof(c), float(scene_range), int(zone), out[0].data_ptr(),
              out[1].data_ptr(), out[2].data_ptr(), _p(zone_out), _stream())
    return out[0], out[1], out[2], zone_out


def dsm_bounds(east, north, alt, out=None):
    """(4,) fp64 device tensor {min east, max east, min north, max north} over the usable points (NaN if none); ``out`` may be given."""
    east, north, alt = (_chk(t, k, torch.float64) for t, k in ((east, "east"), (north, "north"), (alt, "alt")))
    if not (east.dim() == 1 and east.shape == north.shape == alt.shape):
        raise ValueError("east / north / alt must be three (N,) tensors")
    out = torch.empty(4, dtype=torch.float64, device=east.device) if out is None else _chk(out, "out", torch.float64)
    _lib.call("sr_dsm_bounds", _p(east), _p(north), _p(alt), east.shape[0], _p(out), _stream())
    return out


def dsm_rasterize(east, north, alt, xoff, yoff, resolution, xsize, ysize, radius=1, sigma=float("inf")):
    """(dsm, weight) fp32 (ysize, xsize) device tensors: the splat rasteriser of sr_dsm_rasterize."""
    east, north, alt = (_chk(t, k, torch.float64) for t, k in ((east, "east"), (north, "north"), (alt, "alt")))
    if not (east.dim() == 1 and east.shape == north.shape == alt.shape):
        raise ValueError("east / north / alt must be three (N,) tensors")
    if xsize < 1 or ysize < 1:
        raise ValueError(f"empty DSM grid ({ysize} x {xsize})")
    acc = torch.empty(ysize, xsize, 2, dtype=torch.int64, device=east.device)
    dsm = torch.empty(ysize, xsize, dtype=torch.float32, device=east.device)
    weight = torch.empty_like(dsm)
    _lib.call("sr_dsm_rasterize", _p(east), _p(north), _p(alt), east.shape[0], float(xoff), float(yoff), float(resolution), int(xsize),
              int(ysize), int(radius), float(sigma), _p(acc), _p(dsm), _p(weight), _stream())
    return dsm, weight


# ---- nadir DSM rays (csrc/ortho.hip) -------------------------------------------------------------------------------------------------
def utm_to_latlon(easts, norths, zone):
    """(lat, lon) fp64 device tensors (degrees) of fp64 device east / north (metres) in UTM zone ``zone`` (1..60): sr_utm_to_latlon."""
    easts, norths = _chk(easts.contiguous(), "easts", torch.float64), _chk(norths.contiguous(), "norths", torch.float64)
    if easts.dim() != 1 or easts.shape != norths.shape:
        raise ValueError(f"easts / norths must be two (N,) tensors, got {tuple(easts.shape)} / {tuple(norths.shape)}")
    out = torch.empty(2, easts.shape[0], dtype=torch.float64, device=easts.device)
    _lib.call("sr_utm_to_latlon", _p(easts), _p(norths), easts.shape[0], int(zone), out[0].data_ptr(), out[1].data_ptr(), _stream())
    return out[0], out[1]


def ortho_rays(xoff, yoff, resolution, xsize, ysize, zone, min_alt, max_alt, center, scene_range, sun_d, device="cuda", out=None,
               want_latlon=False):
    """sr_ortho_rays: one vertical ray per cell of the (ysize, xsize) DSM grid, row-major with row 0 at the top.  Returns (rays, latlon):
    rays = ``out`` (a (ysize * xsize, >=11) fp32 tensor on ``device`` with unit inner stride, columns 0..10 written) or a new
    (ysize * xsize, 11) tensor; latlon = (ysize * xsize, 2) fp64 (lat, lon) degrees, or None."""
    n = int(xsize) * int(ysize)
    dev = torch.device(device)
    ctr = (C.c_double * 3)(*[float(v) for v in center])
    sun = (C.c_float * 3)(*[float(v) for v in sun_d])
    with torch.cuda.device(dev):
        if out is None:
            rays, stride = torch.empty(max(n, 0), 11, dtype=torch.float32, device=dev), 11
        else:
            rays, stride = _rows(out, "out", 11)
            if rays.shape[0] != n:
                raise ValueError(f"out must hold {n} rows (ysize * xsize), got {tuple(rays.shape)}")
        latlon = torch.empty(max(n, 0), 2, dtype=torch.float64, device=dev) if want_latlon else None
        _lib.call("sr_ortho_rays", float(xoff), float(yoff), float(resolution), int(xsize), int(ysize), int(zone), float(min_alt),
                  float(max_alt), C.addressof(ctr), float(scene_range), sun, _p(rays), int(stride), _p(latlon), _stream())
    return rays, latlon


# ---- geometric sun visibility (csrc/sun_rays.hip) ------------------------------------------------------------------------------------
def sun_rays(rays, depth, center, scene_range, max_alt, sun_d=None, bias_abs=0.0, bias_rel=0.0, out=None, want_latlonalt=False):
    """sr_sun_rays: per primary ray (``rays`` (N, >=11), ``depth`` (N,)) the ray from its surface point towards the sun (``sun_d``: 3
    floats for the whole call, or None for each ray's own columns 8:11), near = bias_abs + bias_rel * (far - near) of the primary ray.
    Returns (sun_rays, valid, latlonalt): sun_rays = ``out`` (an (N, >=11) fp32 tensor with unit inner stride, columns 0..10 written)
    or a new (N, 11) tensor; valid (N,) uint8; latlonalt (3, N) fp64 (lat, lon degrees, alt metres), or None."""
    rays, stride = _rows(rays, "rays", 11)
    n = rays.shape[0]
    depth = _chk(depth, "depth")
    if depth.dim() != 1 or depth.shape[0] != n:
        raise ValueError(f"depth must be ({n},), one value per ray, got {tuple(depth.shape)}")
    ctr = (C.c_double * 3)(*[float(v) for v in center])
    sun = None if sun_d is None else (C.c_float * 3)(*[float(v) for v in sun_d])
    if out is None:
        sr, so = torch.empty(n, 11, dtype=torch.float32, device=rays.device), 11
    else:
        sr, so = _rows(out, "out", 11)
        if sr.shape[0] != n:
            raise ValueError(f"out must hold {n} rows, one per ray, got {tuple(sr.shape)}")
        if n and sr.untyped_storage().data_ptr() == rays.untyped_storage().data_ptr():
            raise ValueError("out must not share its storage with rays (the kernel reads one and writes the other)")
    valid = torch.empty(n, dtype=torch.uint8, device=rays.device)
    lla = torch.empty(3, n, dtype=torch.float64, device=rays.device) if want_latlonalt else None
    _lib.call("sr_sun_rays", _p(rays), int(stride), _p(depth), n, C.addressof(ctr), float(scene_range), float(max_alt), sun, float(bias_abs),
              float(bias_rel), _p(sr), int(so), _p(valid), _p(lla), _stream())
    return sr, valid, lla


def sun_shade(albedo, sky, vis, out=None):
    """sr_sun_shade: rgb (N, 3) = clamp(albedo * (vis + (1 - vis) * sky), 0, 1) in fp32 per pixel, NaN where ``vis`` is NaN.  ``albedo``
    / ``sky`` (N, >=3) rows (e.g. the columns of ``render_image_outputs``), ``vis`` (N,) or (N, 1); ``out``: an (N, >=3) fp32 tensor whose
    columns 0..2 are written."""
    albedo, sa = _rows(albedo, "albedo", 3)
    sky, ss = _rows(sky, "sky", 3)
    n = albedo.shape[0]
    if sky.shape[0] != n or vis.numel() != n or vis.dim() > 2:
        raise ValueError(f"albedo, sky and vis must hold one row per pixel, got {tuple(albedo.shape)}, {tuple(sky.shape)}, {tuple(vis.shape)}")
    vis = _chk(vis.reshape(-1), "vis")
    if out is None:
        rgb, so = torch.empty(n, 3, dtype=torch.float32, device=albedo.device), 3
    else:
        rgb, so = _rows(out, "out", 3)
        if rgb.shape[0] != n:
            raise ValueError(f"out must hold {n} rows, one per pixel, got {tuple(rgb.shape)}")
    _lib.call("sr_sun_shade", _p(albedo), int(sa), _p(sky), int(ss), _p(vis), n, _p(rgb), int(so), _stream())
    return rgb[:, :3]


# ---- ray casting against a DSM raster (csrc/heightfield.hip) -------------------------------------------------------------------------
def _heightfield(hgt):
    hgt = _chk(hgt, "hgt")
    if hgt.dim() != 2 or hgt.numel() == 0:
        raise ValueError(f"hgt must be a non-empty (ysize, xsize) raster, got {tuple(hgt.shape)}")
    return hgt, int(hgt.shape[1]), int(hgt.shape[0])


def heightfield_blockmax(hgt):
    """sr_heightfield_blockmax: (blockmax (ceil(ysize / 16), ceil(xsize / 16)) fp32, gmax (1,) fp32) of an (ysize, xsize) fp32 device
    raster: the maxima of the finite cells of its 16 x 16 blocks and of the whole raster, -inf where there is no finite cell."""
    hgt, xsize, ysize = _heightfield(hgt)
    blockmax = torch.empty(-(-ysize // 16), -(-xsize // 16), dtype=torch.float32, device=hgt.device)
    gmax = torch.empty(1, dtype=torch.float32, device=hgt.device)
    _lib.call("sr_heightfield_blockmax", _p(hgt), xsize, ysize, _p(blockmax), _p(gmax), _stream())
    return blockmax, gmax


def _heightfield_maxima(hgt, accelerate, maxima, always=False):
    if maxima is None:
        return heightfield_blockmax(hgt) if accelerate or always else (None, None)
    blockmax, gmax = maxima
    blockmax, gmax = _chk(blockmax, "blockmax"), _chk(gmax, "gmax")
    if tuple(blockmax.shape) != (-(-hgt.shape[0] // 16), -(-hgt.shape[1] // 16)) or gmax.numel() != 1:
        raise ValueError(f"maxima must be heightfield_blockmax's pair for a {tuple(hgt.shape)} raster, got {tuple(blockmax.shape)} and "
                         f"{tuple(gmax.shape)}")
    return blockmax, gmax


def heightfield_cast(hgt, resolution, rays=None, center=None, scene_range=None, zone=None, xoff=None, yoff=None, seg_a=None, seg_b=None,
                     accelerate=True, maxima=None, want_s=False, want_seg=False):
    """sr_heightfield_cast: the first column of the (ysize, xsize) fp32 device raster ``hgt`` that each ray enters.  The rays are either
    ``rays`` (N, >=8) fp32 in the scene frame (with ``center``, ``scene_range``, ``zone`` 1..60 and the raster's ``xoff`` / ``yoff``) or
    the grid-frame segments ``seg_a`` / ``seg_b`` (N, 3) fp64.  ``maxima``: heightfield_blockmax's pair when it is at hand (computed here
    otherwise, for ``accelerate``).  Returns (depth (N,) fp32, NaN on a miss; cell (N,) int32, -1 on a miss; s (N,) fp64 or None; seg
    (N, 6) fp64 = the UTM (E, N, alt) of both ends of the walked segment, or None)."""
    hgt, xsize, ysize = _heightfield(hgt)
    if (rays is None) == (seg_a is None and seg_b is None):
        raise ValueError("give either rays (scene frame) or seg_a and seg_b (grid frame)")
    ctr = None
    if rays is not None:
        rays, stride = _rows(rays, "rays", 8)
        n = rays.shape[0]
        if center is None or scene_range is None or zone is None or xoff is None or yoff is None:
            raise ValueError("rays in the scene frame need center, scene_range, zone, xoff and yoff")
        ctr = (C.c_double * 3)(*[float(v) for v in center])
        frame = (C.addressof(ctr), float(scene_range), int(zone), float(xoff), float(yoff))
    else:
        seg_a, seg_b = _chk(seg_a, "seg_a", torch.float64), _chk(seg_b, "seg_b", torch.float64)
        if seg_a.dim() != 2 or seg_a.shape[1] != 3 or seg_a.shape != seg_b.shape:
            raise ValueError(f"seg_a / seg_b must be two (N, 3) tensors, got {tuple(seg_a.shape)} / {tuple(seg_b.shape)}")
        if want_seg:
            raise ValueError("want_seg belongs to rays in the scene frame: segments are walked as given")
        n, stride, frame = seg_a.shape[0], 0, (None, 1.0, 0, 0.0, 0.0)
    blockmax, gmax = _heightfield_maxima(hgt, accelerate, maxima)
    dev = hgt.device
    depth = torch.empty(n, dtype=torch.float32, device=dev)
    cell = torch.empty(n, dtype=torch.int32, device=dev)
    s = torch.empty(n, dtype=torch.float64, device=dev) if want_s else None
    seg = torch.empty(n, 6, dtype=torch.float64, device=dev) if rays is not None else None  # the entry's scratch in the ray form
    if n == 0:  # an empty tensor has no address to tell the two forms apart by
        return depth, cell, s, seg if want_seg else None
    _lib.call("sr_heightfield_cast", _p(hgt), xsize, ysize, float(resolution), _p(blockmax), _p(gmax), int(bool(accelerate)), _p(rays),
              int(stride), *frame, _p(seg_a), _p(seg_b), n, _p(depth), _p(cell), _p(s), _p(seg), _stream())
    return depth, cell, s, seg if want_seg else None


def heightfield_shadow(hgt, resolution, sun_d, bias=0.0, accelerate=True, maxima=None):
    """sr_heightfield_shadow: the (ysize, xsize) fp32 mask of the raster ``hgt`` under the sun direction ``sun_d`` (3 floats: east, north,
    up; up > 0): 1 lit, 0 shadowed, NaN where the cell holds no surface.  ``bias`` >= 0 metres lifts the start of every ray."""
    hgt, xsize, ysize = _heightfield(hgt)
    sun = (C.c_double * 3)(*[float(v) for v in sun_d])
    blockmax, gmax = _heightfield_maxima(hgt, accelerate, maxima, always=True)
    out = torch.empty_like(hgt)
    _lib.call("sr_heightfield_shadow", _p(hgt), xsize, ysize, float(resolution), _p(blockmax), _p(gmax), int(bool(accelerate)),
              C.addressof(sun), float(bias), _p(out), _stream())
    return out


# ---- orthorectification onto a DSM raster (csrc/orthorectify.hip) ------------------------------------------------------------------
ORTHO_MODES = {"nearest": 0, "bilinear": 1, "bicubic": 2}
ORTHO_STAGES = {"all": 0, "project": 1, "sample": 2}


def orthorectify_scratch(xsize, ysize):
    """Bytes of scratch sr_orthorectify needs for an (ysize, xsize) raster (host only)."""
    return _scratch_bytes("sr_orthorectify_scratch", xsize, ysize)


def orthorectify(hgt, resolution, xoff, yoff, zone, rpc, image, mode="bilinear", bias=0.0, accelerate=True, maxima=None, scratch=None,
                 color=None, status=None, colrow=None, sum=None, count=None, stage="all"):
    """sr_orthorectify: one view brought onto the (ysize, xsize) fp32 device raster ``hgt`` placed at ``xoff`` / ``yoff`` in UTM ``zone``
    (1..60).  ``rpc``: an "rpcm"-format dict; ``image``: (H, W, C) device tensor, uint8 (values / 255) or fp32, C in 1..4, unit channel
    stride.  Returns (color (ysize, xsize, C) fp32, NaN where the cell is not visible; status (ysize, xsize) uint8: 0 empty, 1 visible,
    2 occluded, 3 outside the image; colrow (ysize, xsize, 2) fp64).  ``sum`` (ysize, xsize, C) fp64 and ``count`` (ysize, xsize) int32:
    accumulators every visible cell adds its colour and 1 to, both or neither.  ``maxima``: heightfield_blockmax's pair when at hand.
    ``scratch``: a contiguous device tensor of at least orthorectify_scratch bytes.  ``stage``: "all", or "project" / "sample" for one of
    the two launches ("sample" reads the ``colrow`` and ``scratch`` a "project" call left).  Nothing is read back."""
    if mode not in ORTHO_MODES:
        raise ValueError(f"mode must be one of {sorted(ORTHO_MODES)}, got {mode!r}")
    if stage not in ORTHO_STAGES:
        raise ValueError(f"stage must be one of {sorted(ORTHO_STAGES)}, got {stage!r}")
    hgt, xsize, ysize = _heightfield(hgt)
    if not (torch.is_tensor(image) and image.is_cuda):
        raise ValueError("image must live on the GPU; satnerf_amd has no CPU path")
    _same_device(image, "image")
    if image.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"image must be uint8 or float32 (got {image.dtype})")
    if image.dim() != 3 or image.numel() == 0 or not 1 <= image.shape[2] <= 4:
        raise ValueError(f"image must be a non-empty (H, W, C) tensor with C in 1..4, got {tuple(image.shape)}")
    height, width, channels = (int(v) for v in image.shape)
    pix_stride = image.stride(1) if width > 1 else channels  # the stride of a dimension of size 1 says nothing
    row_stride = image.stride(0) if height > 1 else width * pix_stride
    if (image.stride(2) != 1 and channels > 1) or pix_stride < channels or row_stride < (width - 1) * pix_stride + channels:
        raise ValueError(f"image must have unit channel stride and rows and pixels that do not overlap, got strides {image.stride()}")
    if not (float(bias) >= 0 and float(bias) != float("inf")):
        raise ValueError(f"bias must be finite and >= 0 metres, got {bias}")
    if (sum is None) != (count is None):
        raise ValueError("give both accumulators, sum and count, or neither")
    buf = rpc_buffer(rpc)
    dev = hgt.device
    blockmax, gmax = _heightfield_maxima(hgt, accelerate, maxima, always=True)
    scratch = _metric_scratch(scratch, orthorectify_scratch(xsize, ysize), dev)

    def out(t, name, shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=dev) if t is None else _chk(t, name, dtype)
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
        return t

    color = out(color, "color", (ysize, xsize, channels), torch.float32)
    status = out(status, "status", (ysize, xsize), torch.uint8)
    colrow = out(colrow, "colrow", (ysize, xsize, 2), torch.float64)
    if sum is not None:
        sum, count = out(sum, "sum", (ysize, xsize, channels), torch.float64), out(count, "count", (ysize, xsize), torch.int32)
    _lib.call("sr_orthorectify", _p(hgt), xsize, ysize, float(resolution), float(xoff), float(yoff), int(zone), _p(blockmax), _p(gmax),
              int(bool(accelerate)), C.addressof(buf), _p(image), 0 if image.dtype == torch.uint8 else 1, width, height, channels,
              int(row_stride), int(pix_stride), ORTHO_MODES[mode], float(bias), ORTHO_STAGES[stage], _p(scratch),
              scratch.numel() * scratch.element_size(), _p(color), _p(status), _p(colrow), _p(sum), _p(count), _stream())
    return color, status, colrow


# ---- cloud fusion (csrc/cloud_grid.hip) --------------------------------------------------------------------------------------------
CLOUD_RULES ={"nearest": 0, "floor": 1}
CLOUD_MODES = {"min": 0, "max": 1, "avg": 2, "med": 3}


def cloud_grid_scratch(n, map_w, map_h):
    """Bytes of scratch sr_cloud_grid needs for n points on a map_h x map_w grid (host only)."""
    return _scratch_bytes("sr_cloud_grid_scratch", n, map_w, map_h)


def cloud_grid(east, north, alt, x0, y0, definition, map_w, map_h, rule="nearest", mode="med", scratch=None, out=None, count=None,
               stages=0):
    """(out, count): the (map_h, map_w) fp64 raster of the per-cell ``mode`` ("min" / "max" / "avg" / "med") of the altitudes of the
    (N,) fp64 device cloud east / north / alt (NaN where no point landed) and the int32 points per cell (sr_cloud_grid).  ``rule``
    "nearest" is eval_s2p.project_cloud_into_utm_grid's cell with (x0, y0) = (bb[0], bb[2]), "floor" the DSM grid's with (x0, y0) =
    (xoff, yoff).  ``scratch``: a contiguous device tensor of at least cloud_grid_scratch bytes.  Nothing is read back."""
    east, north, alt = (_chk(t, k, torch.float64) for t, k in ((east, "east"), (north, "north"), (alt, "alt")))
    if not (east.dim() == 1 and east.shape == north.shape == alt.shape):
        raise ValueError("east / north / alt must be three (N,) tensors")
    if rule not in CLOUD_RULES:
        raise ValueError(f"rule must be one of {sorted(CLOUD_RULES)}, got {rule!r}")
    if mode not in CLOUD_MODES:
        raise ValueError(f"mode must be one of {sorted(CLOUD_MODES)}, got {mode!r}")
    map_w, map_h = int(map_w), int(map_h)
    if map_w < 1 or map_h < 1:
        raise ValueError(f"empty grid ({map_h} x {map_w})")
    dev = east.device
    scratch = _metric_scratch(scratch, cloud_grid_scratch(east.shape[0], map_w, map_h), dev)
    out = torch.empty(map_h, map_w, dtype=torch.float64, device=dev) if out is None else _chk(out, "out", torch.float64)
    count = torch.empty(map_h, map_w, dtype=torch.int32, device=dev) if count is None else _chk(count, "count", torch.int32)
    if out.shape != (map_h, map_w) or count.shape != (map_h, map_w):
        raise ValueError(f"out / count must be ({map_h}, {map_w})")
    _lib.call("sr_cloud_grid", _p(east), _p(north), _p(alt), east.shape[0], float(x0), float(y0), float(definition), map_w, map_h,
              CLOUD_RULES[rule], CLOUD_MODES[mode], _p(scratch), scratch.numel() * scratch.element_size(), _p(out), _p(count), int(stages),
              _stream())
    return out, count


# ---- DSM registration (csrc/dsm_register.hip) --------------------------------------------------------------------------------------
def _raster(t, name):
    t = _chk(t, name, torch.float64)
    if t.dim() != 2:
        raise ValueError(f"{name} must be an (H, W) raster, got shape {tuple(t.shape)}")
    return t


def dsm_register_plan(u_shape, v_shape, irange=5):
    """(scratch bytes, levels) of sr_dsm_compute_shift for these shapes (host only)."""
    nbytes, levels = C.c_int64(0), C.c_int(0)
    _lib.call("sr_dsm_register_scratch", int(u_shape[0]), int(u_shape[1]), int(v_shape[0]), int(v_shape[1]), int(irange), C.byref(nbytes),
              C.byref(levels))
    return nbytes.value, levels.value


def dsm_downsample2x(img):
    """((H+1)//2, (W+1)//2) fp64 device tensor: the reference's downsample2x_ of an fp64 (H, W) device raster."""
    img = _raster(img, "img")
    out = torch.empty((img.shape[0] + 1) // 2, (img.shape[1] + 1) // 2, dtype=torch.float64, device=img.device)
    _lib.call("sr_dsm_downsample2x", _p(img), img.shape[0], img.shape[1], _p(out), _stream())
    return out


def dsm_compute_shift(u, v, irange=5, scaling=True, out=None, scratch=None, maps=False):
    """Enqueue sr_dsm_compute_shift on fp64 (H, W) device rasters u (reference) and v (secondary).  ``out`` is a (9,) int64 device
    tensor (allocated if None): coef (8 fp64) in out[:8], shift (2 int32) in out[8]; ``scratch`` a uint8 device tensor of at least
    dsm_register_plan's bytes.  With maps=True also returns the per-level NCC maps (levels, n, n) fp64 and starts (levels, 2) int32.
    Returns (out, ncc, starts); nothing is read back."""
    u, v = _raster(u, "u"), _raster(v, "v")
    _same_device(v, "v")
    nbytes, levels = dsm_register_plan(u.shape, v.shape, irange)
    scratch = _metric_scratch(scratch, nbytes, u.device)
    out = torch.empty(9, dtype=torch.int64, device=u.device) if out is None else _chk(out, "out", torch.int64)
    n = 2 * int(irange) + 1
    ncc = torch.empty(levels, n, n, dtype=torch.float64, device=u.device) if maps else None
    starts = torch.empty(levels, 2, dtype=torch.int32, device=u.device) if maps else None
    _lib.call("sr_dsm_compute_shift", _p(u), u.shape[0], u.shape[1], _p(v), v.shape[0], v.shape[1], int(irange), int(bool(scaling)),
              _p(scratch), scratch.numel() * scratch.element_size(), out[8:].data_ptr(), out[:8].data_ptr(), _p(ncc), _p(starts),
              _stream())
    return out, ncc, starts


def dsm_apply_shift(v, shift, coef, out=None):
    """(H, W) fp32 device tensor: a v[j + dy, i + dx] + b over v's extent, (dx, dy) / (a, b) read on the device from ``shift`` (2
    int32) and ``coef`` (>= 2 fp64)."""
    v = _raster(v, "v")
    shift, coef = _chk(shift, "shift", torch.int32), _chk(coef, "coef", torch.float64)
    if shift.numel() < 2 or coef.numel() < 2:
        raise ValueError("shift needs 2 int32 and coef at least 2 fp64")
    out = torch.empty(v.shape, dtype=torch.float32, device=v.device) if out is None else _chk(out, "out")
    if out.shape != v.shape:
        raise ValueError(f"out must be {tuple(v.shape)}")
    _lib.call("sr_dsm_apply_shift", _p(v), v.shape[0], v.shape[1], _p(shift), _p(coef), _p(out), _stream())
    return out


# ---- tie-point interpolation (csrc/tie_points.hip) --------------------------------------------------------------------------------
def idw_grid_scratch(k, n_neighbors):
    """Bytes of scratch sr_idw_interpolate needs for k points and n_neighbors (host only)."""
    return _scratch_bytes("sr_idw_grid_scratch", k, n_neighbors)


def idw_interpolate(pts2d, z, n_neighbors, query=None, height=0, width=0, want_indices=False, want_visited=False, out=None, scratch=None):
    """sr_idw_interpolate: (Q,) fp64 IDW of the n_neighbors nearest of the k points ``pts2d`` ((k, 2) fp64 (col, row)) carrying ``z`` ((k,)
    fp32), at the (Q, 2) fp64 ``query`` points or, with query None, at every pixel of the height x width raster (Q = h w, row-major).
    ``want_indices`` adds the (Q, n_neighbors) int32 chosen indices, ``want_visited`` the (Q,) int32 points each query examined (returned
    in that order after the values).  Nothing is read back."""
    pts2d, z = _chk(pts2d, "pts2d", torch.float64), _chk(z, "z")
    if pts2d.dim() != 2 or pts2d.shape[1] != 2 or z.dim() != 1 or z.shape[0] != pts2d.shape[0]:
        raise ValueError(f"pts2d must be (k, 2) and z (k,), got {tuple(pts2d.shape)} and {tuple(z.shape)}")
    _same_device(z, "z")
    k, n = pts2d.shape[0], int(n_neighbors)
    if query is not None:
        query = _chk(query, "query", torch.float64)
        if query.dim() != 2 or query.shape[1] != 2:
            raise ValueError(f"query must be (Q, 2) = (col, row) pairs, got {tuple(query.shape)}")
        nq = query.shape[0]
    else:
        nq = int(height) * int(width)
    dev = pts2d.device
    scratch = _metric_scratch(scratch, idw_grid_scratch(k, n), dev)
    out = torch.empty(nq, dtype=torch.float64, device=dev) if out is None else _chk(out, "out", torch.float64)
    if out.numel() != nq:
        raise ValueError(f"out must hold {nq} doubles")
    idx = torch.empty(nq, n, dtype=torch.int32, device=dev) if want_indices else None
    seen = torch.empty(nq, dtype=torch.int32, device=dev) if want_visited else None
    _lib.call("sr_idw_interpolate", _p(pts2d), _p(z), k, _p(query), nq if query is not None else 0, int(height), int(width), n, _p(scratch),
              scratch.numel() * scratch.element_size(), _p(out), _p(idx), _p(seen), _stream())
    extra = [t for t in (idx, seen) if t is not None]
    return (out, *extra) if extra else out


def gaussian_filter_f64(image, taps0, taps1, out=None, tmp=None):
    """sr_gaussian_filter_f64: the (h, w) fp64 device raster filtered along axis 0 with the 1-D fp64 device ``taps0`` (2 r + 1 values),
    then along axis 1 with ``taps1``, reflect borders; None skips an axis.  Returns a new (h, w) fp64 tensor (or ``out``)."""
    image = _chk(image, "image", torch.float64)
    if image.dim() != 2:
        raise ValueError(f"image must be (h, w), got {tuple(image.shape)}")
    radii = []
    for t, name in ((taps0, "taps0"), (taps1, "taps1")):
        if t is not None and (_chk(t, name, torch.float64).dim() != 1 or t.numel() % 2 != 1):
            raise ValueError(f"{name} must hold 2 r + 1 taps")
        radii.append(-1 if t is None else t.numel() // 2)
    out = torch.empty_like(image) if out is None else _chk(out, "out", torch.float64)
    if out.shape != image.shape:
        raise ValueError(f"out must be {tuple(image.shape)}")
    if taps0 is not None and taps1 is not None:
        tmp = torch.empty_like(image) if tmp is None else _chk(tmp, "tmp", torch.float64)
        if tmp.shape != image.shape:
            raise ValueError(f"tmp must be {tuple(image.shape)}")
    _lib.call("sr_gaussian_filter_f64", _p(image), image.shape[0], image.shape[1], _p(taps0), radii[0], _p(taps1), radii[1], _p(tmp), _p(out),
              _stream())
    return out


# ---- image metrics (csrc/image_metrics.hip) ---------------------------------------------------------------------------------------
def image_metrics_scratch(n=0, planes=0, h=0, w=0):
    """Bytes of scratch sr_image_sse over n elements and sr_ssim_sum over (planes, h, w) need (host only)."""
    return _scratch_bytes("sr_image_metrics_scratch", n, planes, h, w)


def _metric_scratch(scratch, nbytes, dev):
    if scratch is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if not (scratch.is_cuda and scratch.is_contiguous() and scratch.numel() * scratch.element_size() >= nbytes):
        raise ValueError(f"scratch must be a contiguous device tensor of >= {nbytes} bytes")
    _same_device(scratch, "scratch")
    return scratch


def image_sse(pred, gt, mask=None, mask_div=1, out=None, scratch=None):
    """(2,) fp64 device tensor {sum of (pred - gt)^2, count} over contiguous fp32 device tensors of one shape; ``mask`` (optional, bool or
    uint8, numel = pred.numel() / mask_div) selects element i by mask[i // mask_div].  Nothing is read back."""
    pred, gt = _chk(pred, "pred"), _chk(gt, "gt")
    if pred.shape != gt.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape")
    n = pred.numel()
    if mask is not None:
        if mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"mask must be bool or uint8 (got {mask.dtype})")
        mask = _chk(mask, "mask", mask.dtype)
        if int(mask_div) < 1 or mask.numel() * int(mask_div) != n:
            raise ValueError(f"mask holds {mask.numel()} entries, which times mask_div {mask_div} is not the {n} elements")
    out = torch.empty(2, dtype=torch.float64, device=pred.device) if out is None else _chk(out, "out", torch.float64)
    scratch = _metric_scratch(scratch, image_metrics_scratch(n=n), pred.device)
    _lib.call("sr_image_sse", _p(pred), _p(gt), n, _p(mask), int(mask_div), _p(scratch), scratch.numel() * scratch.element_size(), _p(out),
              _stream())
    return out


def ssim_sum(img1, img2, out=None, scratch=None):
    """(2,) fp64 device tensor {sum of the SSIM map (window 3), B*C*H*W} over two contiguous fp32 (B, C, H, W) device tensors.  Nothing
    is read back."""
    img1, img2 = _chk(img1, "img1"), _chk(img2, "img2")
    if img1.dim() != 4 or img1.shape != img2.shape:
        raise ValueError(f"img1 / img2 must be two (B, C, H, W) tensors of one shape, got {tuple(img1.shape)} / {tuple(img2.shape)}")
    b, c, h, w = img1.shape
    out = torch.empty(2, dtype=torch.float64, device=img1.device) if out is None else _chk(out, "out", torch.float64)
    scratch = _metric_scratch(scratch, image_metrics_scratch(planes=b * c, h=h, w=w), img1.device)
    _lib.call("sr_ssim_sum", _p(img1), _p(img2), b * c, h, w, _p(scratch), scratch.numel() * scratch.element_size(), _p(out), _stream())
    return out


# ---- a dataset's colours (csrc/image_colors.hip) ------------------------------------------------------------------------------------
def _image_u8(image_u8, bands, layout):
    """(h, w, (row, pixel, channel) byte strides) of a contiguous uint8 device image of ``bands`` bands, (H, W, bands) ("hwc") or
    (bands, H, W) ("chw"); layout None reads it off the shape."""
    b, word = bands, {3: "three", 4: "four"}[bands]
    image_u8 = _chk(image_u8, "image_u8", torch.uint8)
    if image_u8.dim() != 3:
        raise ValueError(f"image_u8 must be (H, W, {b}) or ({b}, H, W), got {tuple(image_u8.shape)}")
    if layout is None:
        first, last = image_u8.shape[0] == b, image_u8.shape[2] == b
        if first and last:
            raise ValueError(f"image_u8 {tuple(image_u8.shape)} reads as (H, W, {b}) and as ({b}, H, W): pass layout='hwc' or layout='chw'")
        if not (first or last):
            raise ValueError(f"image_u8 must have {word} bands, (H, W, {b}) or ({b}, H, W), got {tuple(image_u8.shape)}")
        layout = "chw" if first else "hwc"
    if layout not in ("hwc", "chw"):
        raise ValueError(f"layout must be 'hwc' or 'chw', got {layout!r}")
    if image_u8.shape[0 if layout == "chw" else 2] != b:
        raise ValueError(f"image_u8 {tuple(image_u8.shape)} does not have {word} bands in layout {layout!r}")
    h, w = (image_u8.shape[1], image_u8.shape[2]) if layout == "chw" else (image_u8.shape[0], image_u8.shape[1])
    if h < 1 or w < 1:
        raise ValueError(f"image_u8 must be at least 1 x 1, got {h} x {w}")
    return h, w, ((w, 1, h * w) if layout == "chw" else (b * w, b, 1))


def image_colors(image_u8, out_h, out_w, out=None, layout=None):
    """sr_image_colors: the (out_h * out_w, 3) fp32 colour rows of one 8-bit image, ``u8 / 255`` and -- unless (out_h, out_w) is the
    image's own size -- the bicubic resize of the reference's loader (datasets/satellite.py:67-80).  ``image_u8``: a contiguous uint8
    device tensor, (H, W, 3) (``layout="hwc"``) or (3, H, W) (``"chw"``); the layout is read off the shape, and a 3 x W x 3 image needs
    it said.  ``out`` = an (out_h * out_w, 3) fp32 tensor with contiguous rows to write into (e.g. one image's rows of a dataset's
    colour tensor).  Nothing is launched for an empty output."""
    h, w, strides = _image_u8(image_u8, 3, layout)
    out_h, out_w = int(out_h), int(out_w)
    if out_h < 0 or out_w < 0:
        raise ValueError(f"out_h and out_w must be >= 0, got {out_h} and {out_w}")
    n = out_h * out_w
    out = torch.empty(n, 3, dtype=torch.float32, device=image_u8.device) if out is None else _chk(out, "out")
    if tuple(out.shape) != (n, 3):
        raise ValueError(f"out must be ({n}, 3), got {tuple(out.shape)}")
    _lib.call("sr_image_colors", _p(image_u8), h, w, strides[0], strides[1], strides[2], out_h, out_w, _p(out), _stream())
    return out


# ---- a Blender scene's colours and rays (csrc/blender.hip) ----------------------------------------------------------------------------
_lanczos_host, _lanczos_dev = {}, {}


def lanczos_tables(n_in, n_out):
    """(bounds (n_out, 2) int32 = [xmin, count], coef (n_out, ksize) int32): Pillow's 8-bit Lanczos coefficients of one axis resized
    n_in -> n_out, as include/satrender.h defines them (fp64 on the host, 22-bit fixed point, rows zero-padded).  Read-only numpy
    arrays, cached per (n_in, n_out); ``sr_blender_colors`` takes ``coef`` and recomputes the bounds itself."""
    import numpy as np

    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"n_in and n_out must be >= 1, got {n_in} and {n_out}")
    hit = _lanczos_host.get((n_in, n_out))
    if hit is not None:
        return hit
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = 2 * int(np.ceil(support)) + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)  # astype truncates toward zero, as a C cast does
    count = np.minimum((center + support + 0.5).astype(np.int64), n_in) - xmin
    x = np.arange(ksize, dtype=np.float64)[None, :]
    arg = (x + xmin[:, None] - center[:, None] + 0.5) / fs

    def sinc(v):
        pv = np.pi * np.where(v == 0.0, 1.0, v)
        return np.where(v == 0.0, 1.0, np.sin(pv) / pv)

    w = np.where((arg >= -3.0) & (arg < 3.0) & (x < count[:, None]), sinc(arg) * sinc(arg / 3.0), 0.0)
    total = np.zeros(n_out)
    for j in range(ksize):  # the running sum in index order (a padded tap adds an exact zero)
        total = total + w[:, j]
    w = np.where(total[:, None] != 0.0, w / np.where(total == 0.0, 1.0, total)[:, None], w)
    coef = np.where(w < 0, w * 4194304.0 - 0.5, w * 4194304.0 + 0.5).astype(np.int64).astype(np.int32)
    bounds = np.stack([xmin, count], 1).astype(np.int32)
    coef.setflags(write=False), bounds.setflags(write=False)
    _lanczos_host[(n_in, n_out)] = bounds, coef
    return bounds, coef


def _lanczos_device(n_in, n_out, dev):
    """The coefficient table of lanczos_tables on ``dev`` (uploaded once per device) and its ksize."""
    key = (int(n_in), int(n_out), dev.index)
    t = _lanczos_dev.get(key)
    if t is None:
        t = _lanczos_dev[key] = torch.from_numpy(lanczos_tables(n_in, n_out)[1].copy()).to(dev)
    return t, t.shape[1]


def blender_colors_scratch(src_h, src_w, out_h, out_w):
    """Bytes of scratch sr_blender_colors needs for this resize (host only): the (src_h, out_w, 4) intermediate when both passes run."""
    return _scratch_bytes("sr_blender_colors_scratch", src_h, src_w, out_h, out_w)


def blender_colors(image_u8, out_h, out_w, out=None, layout=None, want_rgba=False):
    """sr_blender_colors: one 8-bit RGBA image resized to (out_h, out_w) as Pillow's ``Image.resize(..., Image.LANCZOS)`` does, byte for
    byte, and blended onto white as the reference's BlenderDataset does (datasets/blender.py:136-139).  ``image_u8``: a contiguous uint8
    device tensor, (H, W, 4) (``layout="hwc"``) or (4, H, W) (``"chw"``); the layout is read off the shape, and a 4 x W x 4 image needs it
    said.  Returns (rgbs (out_h * out_w, 3) fp32, valid_mask (out_h * out_w,) bool = alpha > 0), and with ``want_rgba`` also the resized
    image, (out_h, out_w, 4) uint8.  ``out`` = an (out_h * out_w, 3) fp32 tensor with contiguous rows to write the colours into.  Nothing
    is launched for an empty output."""
    h, w, strides = _image_u8(image_u8, 4, layout)
    out_h, out_w = int(out_h), int(out_w)
    if out_h < 0 or out_w < 0:
        raise ValueError(f"out_h and out_w must be >= 0, got {out_h} and {out_w}")
    n, dev = out_h * out_w, image_u8.device
    out = torch.empty(n, 3, dtype=torch.float32, device=dev) if out is None else _chk(out, "out")
    if tuple(out.shape) != (n, 3):
        raise ValueError(f"out must be ({n}, 3), got {tuple(out.shape)}")
    mask = torch.empty(n, dtype=torch.bool, device=dev)
    rgba = torch.empty(out_h, out_w, 4, dtype=torch.uint8, device=dev) if want_rgba else None
    coef_w, ksize_w = _lanczos_device(w, out_w, dev) if n and out_w != w else (None, 0)
    coef_h, ksize_h = _lanczos_device(h, out_h, dev) if n and out_h != h else (None, 0)
    nbytes = blender_colors_scratch(h, w, out_h, out_w)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    _lib.call("sr_blender_colors", _p(image_u8), h, w, strides[0], strides[1], strides[2], out_h, out_w, _p(coef_w), ksize_w, _p(coef_h),
              ksize_h, _p(scratch), nbytes, _p(out), _p(mask), _p(rgba), 0, _stream())
    return (out, mask, rgba) if want_rgba else (out, mask)


def blender_perturb(image_u8, lut=None, rects=None, fills=None, layout=None, out=None):
    """sr_blender_perturb: the reference's ``add_perturbation`` (datasets/blender.py:61-79) of one 8-bit RGBA image on the device, from
    host-side parameters (``data.blender_perturbation`` draws them).  ``image_u8``: a contiguous uint8 device tensor, (H, W, 4) or
    (4, H, W), the layout resolved as ``blender_colors`` resolves it.  ``lut``: (4, 256) uint8 on the host, band k's byte v becomes
    ``lut[k, v]``; ``rects``: (n, 4) integers [x0, y0, x1, y1], both corners included, anywhere (clipped to the image), n <= 16, with
    ``fills`` (n, 4) uint8 RGBA, applied in order after the table, so a later rectangle wins.  Either part may be None.  ``out``: a
    tensor like ``image_u8`` to write into -- ``image_u8`` itself works in place -- or None for a new one; it is returned.  The
    parameters travel in the kernel's arguments: nothing is uploaded and nothing waits."""
    import numpy as np

    h, w, strides = _image_u8(image_u8, 4, layout)
    if out is None:
        out = torch.empty_like(image_u8)
    elif out is not image_u8:
        out = _chk(out, "out", torch.uint8)
        if out.shape != image_u8.shape or out.device != image_u8.device:
            raise ValueError(f"out must be {tuple(image_u8.shape)} on {image_u8.device}, got {tuple(out.shape)} on {out.device}")
    if lut is not None:
        lut = np.ascontiguousarray(lut.cpu().numpy() if torch.is_tensor(lut) else lut)
        if lut.dtype != np.uint8 or lut.shape != (4, 256):
            raise ValueError(f"lut must be (4, 256) uint8, got {lut.shape} {lut.dtype}")
    if (rects is None) != (fills is None):
        raise ValueError("rects and fills come together")
    n = 0
    if rects is not None:
        rects, fills = np.asarray(rects), np.asarray(fills)
        n = rects.shape[0]
        if rects.ndim != 2 or rects.shape[1] != 4 or rects.dtype.kind not in "iu" or n > 16:
            raise ValueError(f"rects must be (n, 4) integers with n <= 16, got {rects.shape} {rects.dtype}")
        if fills.shape != (n, 4) or fills.dtype != np.uint8:
            raise ValueError(f"fills must be ({n}, 4) uint8, got {fills.shape} {fills.dtype}")
        if n and (rects.min() < -2 ** 31 or rects.max() >= 2 ** 31):
            raise ValueError("rects must fit 32-bit integers")
        rects, fills = np.ascontiguousarray(rects, dtype=np.int32), np.ascontiguousarray(fills)
    host = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    _lib.call("sr_blender_perturb", _p(image_u8), _p(out), h, w, strides[0], strides[1], strides[2], host(lut), host(rects), host(fills), n,
              _stream())
    return out


def pinhole_rays(h, w, fx, fy, cx, cy, c2w, near, far, out=None):
    """sr_pinhole_rays: the (h * w, 8) fp32 rows [o, d, near, far] of a pinhole camera, get_ray_directions + get_rays of the reference
    (datasets/blender.py:12-59): pixel (r, c) looks along ((c - cx) / fx, -(r - cy) / fy, -1) rotated by c2w[:, :3] and normalised, from
    c2w[:, 3].  ``c2w``: 12 host values, (3, 4) row-major; it and the scalars are rounded to fp32 first, as the reference's tensors hold
    them.  ``out`` = an (h * w, 8) fp32 device tensor with contiguous rows to write into; without it the rows go to the current device."""
    import numpy as np

    h, w = int(h), int(w)
    if h < 0 or w < 0:
        raise ValueError(f"h and w must be >= 0, got {h} and {w}")
    m = np.ascontiguousarray(np.asarray(c2w.cpu() if torch.is_tensor(c2w) else c2w, dtype=np.float32))
    if m.shape != (3, 4):
        raise ValueError(f"c2w must be (3, 4), got {m.shape}")
    n = h * w
    out = torch.empty(n, 8, dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device())) if out is None else _chk(out, "out")
    if tuple(out.shape) != (n, 8):
        raise ValueError(f"out must be ({n}, 8), got {tuple(out.shape)}")
    _lib.call("sr_pinhole_rays", h, w, float(np.float32(fx)), float(np.float32(fy)), float(np.float32(cx)), float(np.float32(cy)),
              m.ctypes.data_as(C.POINTER(C.c_float)), float(np.float32(near)), float(np.float32(far)), _p(out), _stream())
    return out


# ---- evaluation image products (csrc/image_products.hip) ----------------------------------------------------------------------------
def _strided_image(t, name, dims):
    """An fp32 device image read in place through its element strides (a column of the (N, 13) image buffer, a crop window): returns
    the strides with those of one-element dimensions set to 1 (torch leaves them arbitrary; they are never stepped along)."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (got {t.device if torch.is_tensor(t) else type(t).__name__}); satnerf_amd has no CPU path")
    _same_device(t, name)
    if t.dtype != torch.float32 or t.dim() != dims:
        raise ValueError(f"{name} must be a {dims}-D fp32 tensor, got {tuple(t.shape)} {t.dtype}")
    strides = [1 if n <= 1 else s for n, s in zip(t.shape, t.stride())]
    if min(strides) < 1:
        raise ValueError(f"{name} must have positive strides, got {tuple(t.stride())}")
    return strides


def nearest_fill_scratch(h, w):
    """Bytes of scratch sr_nearest_fill needs for an (h, w) image (host only)."""
    return _scratch_bytes("sr_nearest_fill_scratch", h, w)


def nearest_fill(image, want_index=False, out=None, scratch=None):
    """sr_nearest_fill: the (h, w) fp32 image with every NaN replaced by the nearest non-NaN pixel's bits (squared Euclidean pixel
    distance, ties to the smallest row, then column), the reference's griddata(method="nearest") hole fill.  ``image`` is read through
    its strides.  Returns a new dense (h, w) tensor (or ``out``), and with ``want_index`` also the (h, w) int32 flat index r' * w + c' of
    each pixel's source, -1 where the image has no valid pixel."""
    rs, cs = _strided_image(image, "image", 2)
    h, w = image.shape
    out = torch.empty(h, w, dtype=torch.float32, device=image.device) if out is None else _chk(out, "out")
    if tuple(out.shape) != (h, w):
        raise ValueError(f"out must be ({h}, {w}), got {tuple(out.shape)}")
    if h * w:  # the row pass reads source pixels while other workgroups write out
        first, last = image.data_ptr(), image.data_ptr() + 4 * ((h - 1) * rs + (w - 1) * cs + 1)
        if out.data_ptr() < last and first < out.data_ptr() + 4 * h * w:
            raise ValueError("out must not overlap image")
    index = torch.empty(h, w, dtype=torch.int32, device=image.device) if want_index else None
    scratch = _metric_scratch(scratch, nearest_fill_scratch(h, w), image.device)
    _lib.call("sr_nearest_fill", _p(image), h, w, rs, cs, _p(scratch), scratch.numel() * scratch.element_size(), _p(out), _p(index), _stream())
    return (out, index) if want_index else out


def colorize_denominator(vmin, vmax):
    """The divisor the reference's ``ma - mi + 1e-8`` becomes when both bounds are Python floats: an fp64 sum, rounded to fp32 where it
    meets the fp32 image."""
    import numpy as np

    return float(np.float32(float(vmax) - float(vmin) + 1e-8))


def colorize(image, lut=None, nan_to_zero=False, vmin=None, vmax=None, want_index=False, strip=None, strip_col0=0, want_chw=False,
             scratch=None):
    """sr_colorize over the (rows, cols) fp32 image (read through its strides; pass a slice for a crop window): the byte index
    ``(uint8)(255 * ((x - mi) / d))`` of the reference's depth colouring and ``lut[index]``.  ``vmin`` / ``vmax``: Python floats, or None
    for the window's own minimum / maximum.  ``nan_to_zero``: visualize_depth's np.nan_to_num first.  Outputs: ``want_index`` -> (rows,
    cols) uint8; ``strip`` -> the colours are written into this (rows, total_cols, 3) uint8 tensor from column ``strip_col0``;
    ``want_chw`` -> (3, rows, cols) fp32 = byte / 255.  ``lut``: (256, 3) uint8 device tensor, needed for the coloured outputs.  Returns
    {"index", "strip", "chw"} with the outputs asked for."""
    import numpy as np

    rs, cs = _strided_image(image, "image", 2)
    rows, cols = image.shape
    dev = image.device
    if lut is not None and tuple(_chk(lut, "lut", torch.uint8).shape) != (256, 3):
        raise ValueError(f"lut must be (256, 3) uint8, got {tuple(lut.shape)}")
    if lut is None and (strip is not None or want_chw):
        raise ValueError("a coloured output needs a lut")
    if not (want_index or want_chw or strip is not None):
        raise ValueError("no output requested")
    if strip is not None:
        if _chk(strip, "strip", torch.uint8).dim() != 3 or strip.shape[0] != rows or strip.shape[2] != 3:
            raise ValueError(f"strip must be ({rows}, total_cols, 3) uint8, got {tuple(strip.shape)}")
        if not 0 <= int(strip_col0) <= strip.shape[1] - cols:
            raise ValueError(f"columns {strip_col0}..{int(strip_col0) + cols} do not fit a strip of {strip.shape[1]} columns")
    bounds = (vmin is not None) | ((vmax is not None) << 1)
    lo = float(np.float32(vmin)) if vmin is not None else 0.0
    hi = float(np.float32(vmax)) if vmax is not None else 0.0
    denom = colorize_denominator(vmin, vmax) if bounds == 3 else 0.0
    index = torch.empty(rows, cols, dtype=torch.uint8, device=dev) if want_index else None
    chw = torch.empty(3, rows, cols, dtype=torch.float32, device=dev) if want_chw else None
    nbytes = _scratch_bytes("sr_colorize_scratch", bounds)
    scratch = _metric_scratch(scratch, nbytes, dev) if nbytes else None
    _lib.call("sr_colorize", _p(image), rows, cols, rs, cs, int(bool(nan_to_zero)), bounds, lo, hi, denom, _p(lut), _p(index), _p(strip),
              0 if strip is None else strip.shape[1], int(strip_col0), _p(chw), _p(scratch), nbytes, _stream())
    return {"index": index, "strip": strip, "chw": chw}


def unit_to_u8(image, strip, strip_col0=0):
    """sr_unit_to_u8: ``(uint8)(x * 255)`` of the (rows, cols, C) fp32 image (C = 1 or 3, read through its strides) into columns
    ``strip_col0 ..`` of ``strip``, a contiguous (rows, total_cols, C) uint8 device tensor."""
    rs, cs, ks = _strided_image(image, "image", 3)
    rows, cols, ch = image.shape
    if ch not in (1, 3):
        raise ValueError(f"image must have 1 or 3 channels, got {ch}")
    if _chk(strip, "strip", torch.uint8).dim() != 3 or strip.shape[0] != rows or strip.shape[2] != ch:
        raise ValueError(f"strip must be ({rows}, total_cols, {ch}) uint8, got {tuple(strip.shape)}")
    if not 0 <= int(strip_col0) <= strip.shape[1] - cols:
        raise ValueError(f"columns {strip_col0}..{int(strip_col0) + cols} do not fit a strip of {strip.shape[1]} columns")
    _lib.call("sr_unit_to_u8", _p(image), rows, cols, ch, rs, cs, ks, _p(strip), strip.shape[1], int(strip_col0), _stream())
    return strip
