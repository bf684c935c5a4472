"""float64 restatement of the per-ray stage between the training forward and the backward: compositing, the Sat-NeRF / warm-up loss,
the solar-correction and depth losses, the head gradients (d_sigma, d_albedo, d_sun_v, g_beta, d_sky) and the 13 evaluation columns --
what csrc/ray_device.h (composite_ray, render_loss_ray), csrc/ray_ops.hip (composite_bwd_kernel, composite_image_kernel) and
csrc/train_ops.hip (satnerf_loss_kernel, sc_loss_kernel, depth_loss_kernel) compute.  Written from oracle/satnerf_oracle.py
(alpha_composite, satnerf_inference, satnerf_loss, snerf_loss, solar_correction_loss, depth_loss, image_outputs) and their closed-form
derivatives; tests/test_ray_reference_host.py pins every value to the oracle and every gradient to torch.autograd through it.
Runs on whatever device its inputs live on.

MODELLED (reproduced bit for bit in float32, because the kernels compute them unfused and everything later depends on them
discontinuously or with unbounded gain):
  delta_j = fl(z[j+1] - z[j]), 1e10f for the last sample;   dens_j = fl(sigma_j + fl(noise_j * noise_std));
  x_j = fl(delta_j * relu(dens_j));   alpha_j = fl(1 - E_j);   f_j = fl(fl(1 - alpha_j) + 1e-10f);
  the constants the kernels round once: 1/n, 0.5f/3, 1/3.0f, lambda/3.
ASSUMED (not a documented property of the hardware, stated as wgrad_reference.py states EPS_SIN): the device's expf returns a float32
  within one ulp of the true value (the HIP math API's stated accuracy), expf(-0) = 1 exactly and expf(-x) <= 1.  Together with the
  half ulp of rounding the float64 value to float32 that is EPS_EXP = 1.5 * 2^-23, relative.  logf: the same, EPS_LOG.
  alpha and f are ROUNDED functions of E: an E one ulp off either leaves them unchanged or moves them by a whole step of their grid.
  So the ambiguity is not EPS_EXP * E pushed through a derivative of the rounding but the interval itself: E_lo / E_hi = E (1 -/+
  EPS_EXP) rounded to float32 are run through the modelled float32 chain (it is monotone), and amb_alpha_j, amb_f_j, amb_E_j are the
  larger distance of the centre value from either end.
NOT MODELLED: the order and rounding of every float32 sum, product, scan and division behind those intermediates.

THE GATE of an output element y:   |y_dev - y_ref| <= (1 + 2^-10) [ 2^-24 sum_terms C_t |t|  +  amb_y  +  floor_y ] + 2^-126
* 2^-24 sum C_t |t| (``V.r``): every formula below is written once over the number type ``V``, which carries beside the float64 value
  the first-order bound of its float32 rounding error in units of 2^-24 (half an ulp relative): one unit of |result| per operation,
  the operands' own bounds scaled by the partial derivative's magnitude.  Expanded, that IS the sum over the terms t of y's fully
  expanded expression of |t| times the count C_t of roundings on t's path -- the convention of late_grads_reference.py (a sum's error
  is relative to its terms, not its value), with the count taken per term.  The counts that are not one-per-operation are written
  next to the line they belong to: a lane reduction or scan is LEVELS = 6 adds deep for every term, a ray of more than 64 samples adds
  one accumulation per segment (``_levels``), the transmittance T_j is a product of j factors = j roundings in ANY order of
  multiplication (+ one per segment carry), the suffix sum keeps its own term's rounding although the term is subtracted again
  (after = suf - tail: the kernels compute it so, and with f = 1e-10 under it that residue is the largest error of a saturated sample).
  An fma rounds once where the count assumes twice, a correctly rounded division once.
* amb_y = (1 + R) sum_j |dy/dalpha_j| amb_alpha_j + |dy/df_j| amb_f_j + |dy/dE_j| amb_E_j: the expf ambiguity through the reference's own
  float64 Jacobian (torch.autograd over the formulas below; a ray's outputs depend on that ray alone, so one batched backward pass per
  output column gives every ray's row).  dy/dE_j is the direct dependence (the factor exp(-x_j) of d_sigma_j).  R = sum_j amb_f_j / f_j
  of the ray bounds the second-order remainder of the products of f.
* floor_y (``V.a``): every float32 product or quotient that leaves the normal range is off by at most 2^-126 absolutely (flushed or
  denormal); that enters at each product (T_j: 2 * 2^-126) and is carried on with the same partial derivatives, so a floor under a division
  by f = 1e-10 is multiplied by 1e10 as it is on the device.
* 1 + 2^-10: the first-order counts reach a few hundred, so the neglected second-order rounding terms stay below 2^-16 of the bound.
Every constant above comes from the arithmetic; none was chosen by looking at a kernel's error.

WHAT THE GATES DO NOT DECIDE: a colour channel whose unclamped value lies within its own gate of 0 or 1 (the clamp's pass-through gate
may fall either way), and a sample whose f moves by more than 2^-17 f over the expf ambiguity (1 - E near a rounding step at small E).
``make_inputs`` builds inputs with neither; ``coverage`` reports both so that the tests can assert it.

Worst ratio |error| / gate of the float32 emulation (tests/test_ray_reference_host.py, sequential cumprod / cumsum) and of the MI355X
kernels (tests/test_hip_ray_reference.py), per output, are recorded in those modules' headers.

``fault=`` plants one named arithmetic fault (FAULTS) into the formulas; only the host self-test sets it, on the float32 emulation."""
import numpy as np
import torch

U = 2.0 ** -24            # half a float32 ulp, relative: one rounding
TINY = 2.0 ** -126        # smallest normal float32: absolute error of a result that underflows
EPS_EXP = 1.5 * 2.0 ** -23  # ASSUMED: expf within 1 ulp (2^-23 relative at worst) + half an ulp (2^-24) for rounding the float64 value
EPS_LOG = EPS_EXP           # ASSUMED: logf likewise
LEVELS = 6                # a 64-lane butterfly or Hillis-Steele scan: six adds on every term's path
SECOND = 1.0 + 2.0 ** -10
AMB_F_MAX = 2.0 ** -17    # see WHAT THE GATES DO NOT DECIDE

FAULTS = ("last_delta", "no_floor", "inclusive_T", "suffix_incl", "carry_fwd", "carry_rev", "gate_sigma", "no_clamp_gate", "no_1m_sun",
          "no_1m_sky", "db_missing", "db_sign", "warm_log", "mean_3n", "depth_no_w", "sc_no_w")


def c32(x, mode="ref"):
    """A constant as the float32 the kernel holds (mode "exact": as the oracle holds it)."""
    return float(x) if mode == "exact" else float(np.float32(x))


def _levels(s):
    """Adds on a term's path through a per-lane accumulation over ceil(S / 64) segments followed by the 6-level lane reduction."""
    return LEVELS + (s + 63) // 64


# ------------------------------------------------------------------------------------------------------------ the number type
class V:
    """float64 value ``v`` + rounding bound ``r`` (units of 2^-24) + absolute floor ``a``; with a float32 ``v`` it is the plain float32
    emulation (no bounds kept, every operation one torch float32 operation, sums sequential)."""
    __slots__ = ("v", "r", "a")

    def __init__(self, v, r=None, a=None):
        self.v = v
        self.r = r
        self.a = a
        if v.dtype == torch.float64 and r is None:
            self.r, self.a = torch.zeros_like(v), torch.zeros_like(v)

    @property
    def emu(self):
        return self.v.dtype == torch.float32

    @staticmethod
    def exact(t, like=None):
        """Data the kernel reads: no error.  ``like``: take its mode (float64 reference / float32 emulation)."""
        if isinstance(t, V):
            return t
        dt = torch.float32 if (like is not None and like.emu) else torch.float64
        return V(t.detach().to(dt))

    def _lift(self, o):
        if isinstance(o, V):
            return o
        if torch.is_tensor(o):
            return V.exact(o, self)
        return V(torch.full_like(self.v.detach(), o))     # a constant the caller has already rounded as the kernel holds it

    def _new(self, v, r, a):
        return V(v) if self.emu else V(v, r, a)

    def __add__(self, o):
        o = self._lift(o)
        v = self.v + o.v
        if self.emu:
            return V(v)
        return V(v, self.r + o.r + v.detach().abs(), self.a + o.a)      # one rounding of the sum

    __radd__ = __add__

    def __neg__(self):
        return self._new(-self.v, self.r, self.a)

    def __sub__(self, o):
        return self + (-self._lift(o))

    def __rsub__(self, o):
        return self._lift(o) + (-self)

    def __mul__(self, o):
        o = self._lift(o)
        v = self.v * o.v
        if self.emu:
            return V(v)
        x, y, p = self.v.detach().abs(), o.v.detach().abs(), v.detach().abs()
        return V(v, self.r * y + x * o.r + p, self.a * y + x * o.a + TINY * (p != 0))   # one rounding; may underflow

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._lift(o)
        v = self.v / o.v
        if self.emu:
            return V(v)
        y, q = o.v.detach().abs(), v.detach().abs()
        return V(v, self.r / y + q * o.r / y + q, self.a / y + q * o.a / y + TINY * (q != 0))   # correctly rounded: one rounding

    def __rtruediv__(self, o):
        return self._lift(o) / self

    def log(self):
        v = torch.log(self.v)
        if self.emu:
            return V(v)
        y = self.v.detach().abs()
        return V(v, self.r / y + (EPS_LOG / U) * v.detach().abs(), self.a / y)    # logf: EPS_LOG relative (assumed)

    def clamp01(self):
        return self._new(self.v.clamp(0.0, 1.0), self.r, self.a)               # 1-Lipschitz, exact

    def where(self, mask, other=0.0):
        o = self._lift(other)
        v = torch.where(mask, self.v, o.v)
        if self.emu:
            return V(v)
        return V(v, torch.where(mask, self.r, o.r), torch.where(mask, self.a, o.a))

    def sum(self, dim, levels):
        """A reduction whose every term passes ``levels`` adds (lane tree, segment accumulation)."""
        if self.emu:
            return V(torch.cumsum(self.v, dim).select(dim, -1))               # sequential float32
        return V(self.v.sum(dim), (self.r + levels * self.v.detach().abs()).sum(dim), self.a.sum(dim))

    def suffix(self, levels):
        """Inclusive suffix sum along the last dimension."""
        rc = lambda t: torch.flip(torch.cumsum(torch.flip(t, (-1,)), -1), (-1,))  # noqa: E731
        if self.emu:
            return V(rc(self.v))
        return V(rc(self.v), rc(self.r + levels * self.v.detach().abs()), rc(self.a))

    def map(self, fn):
        """A re-indexing (slice, unsqueeze, cat with itself ...) applied to value and bounds alike."""
        return V(fn(self.v)) if self.emu else V(fn(self.v), fn(self.r), fn(self.a))

    def gate(self, amb=None):
        g = U * self.r + self.a
        if amb is not None:
            g = g + amb
        return SECOND * g + TINY


def vcat(parts, dim=-1):
    if parts[0].emu:
        return V(torch.cat([p.v for p in parts], dim))
    return V(torch.cat([p.v for p in parts], dim), torch.cat([p.r for p in parts], dim), torch.cat([p.a for p in parts], dim))


# ------------------------------------------------------------------------------------------ sigma -> alpha -> transmittance
class Chain:
    """delta, dens (plain tensors, exact in every mode), E, alpha, f, T, w (V) of a batch of rays, and the expf ambiguity of the three
    leaves.  mode: "ref" = the modelled float32 intermediates in float64 with bounds; "exact" = the oracle's formulas in float64, nothing
    rounded (pins the formulas to the oracle); "emu" = float32 throughout."""

    def __init__(self, z, sigma, noise, noise_std, mode="ref", fault=None):
        self.mode, self.fault = mode, fault
        n, s = z.shape
        self.n, self.s = n, s
        f32 = mode != "exact"
        dt = torch.float32 if f32 else torch.float64
        z, sigma = z.detach().to(dt), sigma.detach().to(dt)
        big = torch.full_like(z[:, :1], 1e10)
        if fault == "last_delta" and s > 1:
            big = z[:, -1:] - z[:, -2:-1]
        delta = torch.cat([z[:, 1:] - z[:, :-1], big], -1)
        dens = sigma if noise is None else sigma + noise.detach().to(dt) * torch.tensor(noise_std, dtype=dt, device=z.device)
        x = delta * torch.relu(dens)
        one = torch.ones((), dtype=dt, device=z.device)
        tiny = torch.tensor(1e-10, dtype=dt, device=z.device)

        def tail(e):   # alpha, f from E, in the mode's arithmetic
            alpha = one - e
            return alpha, ((one - alpha) if fault == "no_floor" else (one - alpha) + tiny)

        self.z, self.sigma, self.delta, self.dens, self.x = z, sigma, delta, dens, x
        self.leaves, self.ambs, self.R = None, None, 0.0
        if mode == "emu":
            e = torch.exp(-x)
            alpha, f = tail(e)
            self.E, self.alpha, self.f = V(e), V(alpha), V(f)
        elif mode == "exact":
            e = torch.exp(-x)
            alpha, f = tail(e)
            self.E, self.alpha, self.f = V(e), V(alpha), V(f)
        else:
            e64 = torch.exp(-x.double())
            zero_x = x == 0
            ends = []
            for k in (1.0, 1.0 - EPS_EXP, 1.0 + EPS_EXP):
                e = torch.where(zero_x, torch.ones_like(x), (e64 * k).float().clamp(max=1.0))   # expf(-0) = 1, expf <= 1 (assumed)
                ends.append((e,) + tail(e))
            (e, alpha, f), lo, hi = ends
            amb = [torch.maximum((c - l).abs(), (h - c).abs()).double() for c, l, h in zip(ends[0], lo, hi)]
            amb[0] = amb[0] + TINY * (~zero_x)                                     # E below the normal range: flushed or denormal
            self.leaves = [t.double().requires_grad_(True) for t in (e, alpha, f)]
            self.ambs = amb
            self.E, self.alpha, self.f = (V(t) for t in self.leaves)
            self.R = (amb[2] / f.double()).sum(-1)
        self.T = self._transmittance()
        self.w = self.alpha * self.T
        self.nseg = (s + 63) // 64

    def _transmittance(self):
        f, s = self.f, self.s
        if self.f.emu or self.mode == "exact":
            incl = torch.cumprod(f.v, -1)
            if self.fault == "carry_fwd" and s > 64:
                incl = torch.cat([torch.cumprod(f.v[:, a:a + 64], -1) for a in range(0, s, 64)], -1)
                excl = torch.cat([torch.cat([torch.ones_like(incl[:, :1]), incl[:, a:min(a + 64, s) - 1]], -1) for a in range(0, s, 64)], -1)
                return V(excl)
            if self.fault == "inclusive_T":
                return V(incl)
            return V(torch.cat([torch.ones_like(incl[:, :1]), incl[:, :-1]], -1))
        # reference: exclusive product as exp(sum log f) (f >= 1e-10 > 0), differentiable without a special case at underflow
        lg = torch.log(f.v)
        excl = torch.cumsum(lg, -1) - lg
        t = torch.exp(excl)
        j = torch.arange(s, dtype=torch.float64, device=t.device)
        count = j + torch.div(j, 64, rounding_mode="floor")        # j multiplications in any order + one per segment carry
        td = t.detach()
        return V(t, count * td, 2 * TINY * (j > 0) * torch.ones_like(td))   # a product chain below the normal range: off by <= 2^-126, twice (scan, carry)

    def amb(self, y):
        """(1 + R) sum_j |dy/dleaf_j| amb_leaf_j for every element of ``y`` (N, ...), a float64 tensor computed from this chain's leaves."""
        if self.leaves is None or not y.requires_grad:
            return torch.zeros_like(y.detach())
        n = y.shape[0]
        flat = y.reshape(n, -1)
        m = flat.shape[1]
        out = torch.zeros(n, m, dtype=torch.float64, device=y.device)
        eye = torch.eye(m, dtype=torch.float64, device=y.device)
        grads = torch.autograd.grad(flat.sum(0), self.leaves, grad_outputs=eye, is_grads_batched=True, retain_graph=True, allow_unused=True)
        for g, a in zip(grads, self.ambs):
            if g is not None:
                out += (g.abs() * a.unsqueeze(0)).sum(-1).transpose(0, 1)      # g: (m, N, S)
        return (out * (1.0 + self.R).unsqueeze(-1)).reshape(y.shape)


def _irradiance(ch, sun_v, sky):
    """sun_v + (1 - sun_v) sky per sample and channel (N, S, 3); 1 without a sun head."""
    if sun_v is None:
        return None
    sv, k = V.exact(sun_v, ch.E).map(lambda t: t.unsqueeze(-1)), V.exact(sky, ch.E).map(lambda t: t.unsqueeze(1))
    return sv + (1.0 - sv) * k


def _colour(ch, w, albedo, irr):
    """sum_j w_j albedo_jc irr_jc (N, 3), unclamped."""
    t = w.map(lambda x: x.unsqueeze(-1)) * V.exact(albedo, ch.E)
    if irr is not None:
        t = t * irr
    return t.sum(1, _levels(ch.s))


def composite(z, sigma, noise, noise_std, albedo=None, sun_v=None, sky=None, clamp=True, mode="ref", fault=None):
    """sr_composite_fwd: weights, transp (N, S), depth (N,), rgb (N, 3) -- zeros without an albedo -- and the unclamped colour ``c``."""
    ch = Chain(z, sigma, noise, noise_std, mode, fault)
    out = {"chain": ch, "weights": ch.w, "transp": ch.T, "depth": (ch.w * V.exact(ch.z, ch.E)).sum(-1, _levels(ch.s))}
    if albedo is None:
        c = V.exact(torch.zeros(ch.n, 3, device=z.device), ch.E)
    else:
        c = _colour(ch, ch.w, albedo, _irradiance(ch, sun_v, sky))
    out["c"], out["rgb"] = c, (c.clamp01() if clamp else c)
    return out


def _pass_gate(c):
    return (c.v.detach() >= 0) & (c.v.detach() <= 1)


def _backward(ch, w, T, G0, gr, albedo, sun_v, sky, irr, g_T=None):
    """The closed-form compositing backward both kernels run.  G0 (N, S): the part of G_j = dL/dw_j that is not colour; gr (N, 3): the
    gradient arriving at the unclamped colour (already gated), or None."""
    fault, s = ch.fault, ch.s
    G = G0
    a = V.exact(albedo, ch.E) if albedo is not None else None
    if gr is not None:
        g3 = gr.map(lambda t: t.unsqueeze(1))
        t = g3 * a
        if irr is not None:
            t = t * irr
        col = t.map(lambda x: x[..., 0]) + t.map(lambda x: x[..., 1]) + t.map(lambda x: x[..., 2])
        G = col if G0 is None else G0 + col
    tail = G * w
    if g_T is not None:
        tail = tail + V.exact(g_T, ch.E) * T
    suf = tail.suffix(_levels(s) + 1)            # 6-level reverse scan + one add per later segment's carry + the carry's own add
    if fault == "carry_rev" and s > 64:          # each segment's suffix sum on its own
        suf = vcat([tail.map(lambda t, a0=a0: t[:, a0:a0 + 64]).suffix(LEVELS) for a0 in range(0, s, 64)])
    after = suf if fault == "suffix_incl" else suf - tail
    dalpha = G * T - after / ch.f
    on = (ch.sigma if fault == "gate_sigma" else ch.dens) > 0
    out = {"d_sigma": (dalpha * V.exact(ch.delta, ch.E) * ch.E).where(on)}
    if gr is not None:
        q = w.map(lambda t: t.unsqueeze(-1)) * g3
        out["d_albedo"] = q * irr if irr is not None else q
        di = q * a
        if sun_v is not None:
            k1 = V.exact(sky, ch.E).map(lambda t: t.unsqueeze(1))
            k1 = k1 * 0.0 + 1.0 if fault == "no_1m_sky" else 1.0 - k1
            t = di * k1
            out["d_sun"] = t.map(lambda x: x[..., 0]) + t.map(lambda x: x[..., 1]) + t.map(lambda x: x[..., 2])
            sv1 = V.exact(sun_v, ch.E).map(lambda t: t.unsqueeze(-1))
            sv1 = sv1 * 0.0 + 1.0 if fault == "no_1m_sun" else 1.0 - sv1
            out["d_sky"] = (di * sv1).sum(1, _levels(s))
    zero = lambda *shape: V.exact(torch.zeros(*shape, device=ch.z.device), ch.E)  # noqa: E731
    out.setdefault("d_albedo", zero(ch.n, s, 3))
    out.setdefault("d_sun", zero(ch.n, s))
    out.setdefault("d_sky", zero(ch.n, 3))
    return out


def composite_grads(z, sigma, noise, noise_std, albedo=None, sun_v=None, sky=None, clamp=True, g_rgb=None, g_depth=None, g_w=None, g_T=None,
                    weights=None, transp=None, mode="ref", fault=None):
    """sr_composite_bwd: d_sigma, d_albedo, d_sun, d_sky from the four arriving gradients, each optional.  ``weights`` / ``transp``: the
    forward's outputs as the kernel reads them from memory (exact data); None = this reference's own."""
    ch = Chain(z, sigma, noise, noise_std, mode, fault)
    w = ch.w if weights is None else V.exact(weights, ch.E)
    T = ch.T if transp is None else V.exact(transp, ch.E)
    irr = _irradiance(ch, sun_v, sky)
    gr, c = None, None
    if g_rgb is not None and albedo is not None:
        gr = V.exact(g_rgb, ch.E)
        if clamp:
            c = _colour(ch, w, albedo, irr)            # the kernel recomputes the unclamped colour from the weights it reads
            if fault != "no_clamp_gate":
                gr = gr.where(_pass_gate(c))
    G0 = None
    if g_w is not None:
        G0 = V.exact(g_w, ch.E)
    if g_depth is not None:
        t = V.exact(g_depth, ch.E).map(lambda x: x.unsqueeze(-1)) * V.exact(ch.z, ch.E)
        G0 = t if G0 is None else G0 + t
    if G0 is None:
        G0 = V.exact(torch.zeros_like(ch.z), ch.E)
    out = _backward(ch, w, T, G0, gr, albedo, sun_v, sky, irr, g_T)
    out["chain"], out["c"] = ch, c
    return out


def _loss_core(b, sq, n, warm, fault, mode, grad_scale=None):
    """Per ray: contribution to the batch-mean loss, the factor kk of d loss / d rgb = (rgb - target) kk, and d loss / d beta_r."""
    inv_n = c32(1.0 / (3 * n if fault == "mean_3n" else n), mode)
    third, sixth = c32(1.0 / 3.0, mode), c32(0.5 / 3.0, mode)
    ib2 = V.exact(torch.full_like(sq.v.detach(), 2.0), sq) if warm else 1.0 / (b * b)     # SNerfLoss: beta^2 = 1/2 and no log term
    contrib = sq * ib2 * sixth * inv_n
    if not warm or fault == "warm_log":
        contrib = contrib + 0.5 * b.log() * inv_n
    kk = ib2 * third * inv_n
    if warm:
        db = None
    else:
        first = -sq * ib2 / b * third
        db = (first if fault == "db_missing" else first - 0.5 / b if fault == "db_sign" else first + 0.5 / b) * inv_n
    if grad_scale is not None:
        kk = kk * c32(grad_scale, mode)
        db = None if db is None else db * c32(grad_scale, mode)
    return contrib, kk, db


def _total(contrib, warm, ch=None):
    """The batch loss (the float64 sum of loss_parts) with its gate: each ray's contribution passes at most 3 adds inside its block,
    ray 0's the + 1.5 as well."""
    c = contrib.v.detach().double()
    val = c.sum() + (0.0 if warm else 1.5)
    if contrib.emu:
        return val, None
    amb = ch.amb(contrib.v) if ch is not None else torch.zeros_like(c)
    g = (U * (contrib.r + 3 * c.abs()) + contrib.a + amb).sum() + (0.0 if warm else U * (4 * 1.5 + c[0].abs()))   # + 1.5, then 3 adds of <= 1.5 + ...
    return val, SECOND * g + TINY


def render_loss(z, sigma, noise, noise_std, albedo, sun_v, beta, sky, target, beta_min=0.05, warm=False, mode="ref", fault=None):
    """sr_render_loss (S <= 64): loss, rgb, d_sigma, d_albedo, d_sun, g_beta, d_sky."""
    ch = Chain(z, sigma, noise, noise_std, mode, fault)
    n, s = ch.n, ch.s
    irr = _irradiance(ch, sun_v, sky)
    c = _colour(ch, ch.w, albedo, irr)
    bj = V.exact(beta, ch.E)
    b = (ch.w * bj).sum(-1, _levels(s)) + c32(beta_min, mode)
    rgb = c.clamp01()
    e = rgb - V.exact(target, ch.E)
    e2 = e * e
    sq = e2.map(lambda t: t[:, 0]) + e2.map(lambda t: t[:, 1]) + e2.map(lambda t: t[:, 2])
    contrib, kk, db = _loss_core(b, sq, n, warm, fault, mode)
    gr = e * kk.map(lambda t: t.unsqueeze(-1))
    if fault != "no_clamp_gate":
        gr = gr.where(_pass_gate(c))
    if db is None:
        G0, g_beta = None, V.exact(torch.zeros_like(ch.z), ch.E)
    else:
        db1 = db.map(lambda t: t.unsqueeze(-1))
        G0, g_beta = db1 * bj, db1 * ch.w
    out = _backward(ch, ch.w, ch.T, G0, gr, albedo, sun_v, sky, irr)
    out.update(chain=ch, c=c, rgb=rgb, g_beta=g_beta, contrib=contrib, b=b)
    out["loss"], out["loss_gate"] = _total(contrib, warm, ch)
    return out


def satnerf_loss(rgb, weights, beta, target, beta_min=0.05, grad_scale=1.0, warm=False, mode="ref", fault=None):
    """sr_satnerf_loss, the separate kernel: loss, g_rgb (N, 3), g_weights, g_beta (N, S); its inputs are data."""
    like = V(torch.zeros((), dtype=torch.float32 if mode == "emu" else torch.float64))
    w, bj = V.exact(weights, like), V.exact(beta, like)
    n, s = weights.shape
    b = (w * bj).sum(-1, _levels(s)) + c32(beta_min, mode)
    d = V.exact(rgb, like) - V.exact(target, like)
    d2 = d * d
    sq = d2.map(lambda t: t[:, 0]) + d2.map(lambda t: t[:, 1]) + d2.map(lambda t: t[:, 2])
    contrib, kk, db = _loss_core(b, sq, n, warm, fault, mode, grad_scale)
    zero = V.exact(torch.zeros_like(weights), like)
    out = {"g_rgb": d * kk.map(lambda t: t.unsqueeze(-1)), "contrib": contrib,
           "g_weights": zero if db is None else db.map(lambda t: t.unsqueeze(-1)) * bj,
           "g_beta": zero if db is None else db.map(lambda t: t.unsqueeze(-1)) * w}
    out["loss"], out["loss_gate"] = _total(contrib, warm)
    return out


def sc_loss(z, sigma, noise, noise_std, sun_v, lambda_sc, mode="ref", fault=None):
    """sr_sc_loss (train_ops.hip: term2 = sum_j (T_j - sun_j)^2, term3 = 1 - sum_j w_j sun_j, T and w detached): loss, d_sun (N, S)."""
    ch = Chain(z, sigma, noise, noise_std, mode, fault)
    lam = torch.full((ch.n, 1), c32(c32(lambda_sc, mode) / 3.0, mode), dtype=torch.float64, device=z.device)
    coef = V.exact(lam, ch.E) * c32(1.0 / ch.n, mode)       # lam * inv_n: one rounding
    sv = V.exact(sun_v, ch.E)
    e = ch.T - sv
    inner = -2.0 * e if fault == "sc_no_w" else -2.0 * e - ch.w
    t2, t3 = (e * e).sum(-1, _levels(ch.s)), (ch.w * sv).sum(-1, _levels(ch.s))
    contrib = coef.map(lambda t: t[:, 0]) * (t2 + 1.0 - t3)
    out = {"chain": ch, "d_sun": coef * inner, "contrib": contrib}
    out["loss"], out["loss_gate"] = _total(contrib, True, ch)
    return out


def depth_loss(depth, depths, lambda_ds, use_weights=True, mode="ref", fault=None):
    """sr_depth_loss: lambda_ds / 3 * mean(w (depth - target)^2) with depths (N, stride) = [target, weight, ...]: loss, g_depth (N,).
    A ray's contribution passes the 6-level wave sum and 3 adds over the block's four waves."""
    like = V(torch.zeros((), dtype=torch.float32 if mode == "emu" else torch.float64))
    n = depth.shape[0]
    lam, inv_n = c32(c32(lambda_ds, mode) / 3.0, mode), c32(1.0 / n, mode)
    diff = V.exact(depth, like) - V.exact(depths[:, 0], like)
    w = V.exact(depths[:, 1] if (use_weights and fault != "depth_no_w") else torch.ones_like(depths[:, 0]), like)
    contrib = lam * w * diff * diff * inv_n
    out = {"g_depth": 2.0 * lam * w * diff * inv_n, "contrib": contrib}
    c = contrib.v.double()
    out["loss"] = c.sum()
    out["loss_gate"] = None if contrib.emu else SECOND * (U * (contrib.r + (LEVELS + 3) * c.abs()) + contrib.a).sum() + TINY
    return out


def composite_image(z, sigma, noise, noise_std, albedo, sun_v, beta, sky, mode="ref", fault=None):
    """sr_composite_image: (N, 13) = rgb(3) clamped, depth, acc, sum w sun, sum w albedo (3), sum w beta, acc * sky (3)."""
    ch = Chain(z, sigma, noise, noise_std, mode, fault)
    lv = _levels(ch.s)
    c = _colour(ch, ch.w, albedo, _irradiance(ch, sun_v, sky))
    acc = ch.w.sum(-1, lv)
    w3 = ch.w.map(lambda t: t.unsqueeze(-1))
    cols = [c.clamp01(), (ch.w * V.exact(ch.z, ch.E)).sum(-1, lv).map(lambda t: t.unsqueeze(-1)), acc.map(lambda t: t.unsqueeze(-1)),
            (ch.w * V.exact(sun_v, ch.E)).sum(-1, lv).map(lambda t: t.unsqueeze(-1)), (w3 * V.exact(albedo, ch.E)).sum(1, lv),
            (ch.w * V.exact(beta, ch.E)).sum(-1, lv).map(lambda t: t.unsqueeze(-1)), acc.map(lambda t: t.unsqueeze(-1)) * V.exact(sky, ch.E)]
    return {"chain": ch, "image": vcat(cols), "c": c}


# ------------------------------------------------------------------------------------------------------------------ comparing
def ratio(got, want, ch=None):
    """|got - want| / gate per element (0 where both the error and the gate's variable part vanish) -> (worst, tensor)."""
    amb = ch.amb(want.v) if ch is not None else None
    gate = want.gate(amb)
    err = (got.detach().double().to(want.v.device).reshape(want.v.shape) - want.v.detach()).abs()
    r = torch.where(torch.isfinite(err), err / gate, torch.full_like(err, float("inf")))     # a NaN from the device is outside every gate
    return (float(r.max()) if r.numel() else 0.0), r


def undecided_clamp(c, ch=None):
    """Colour channels whose unclamped value lies within its own gate of 0 or 1 (exact zeros of an all-zero ray excepted: no error)."""
    if c is None or c.emu:
        return 0
    amb = ch.amb(c.v) if ch is not None else None
    g, v = c.gate(amb), c.v.detach()
    exact0 = (v == 0) & (c.r == 0)
    return int((((v.abs() <= g) | ((v - 1).abs() <= g)) & ~exact0).sum())


# --------------------------------------------------------------------------------------------------------------------- inputs
def make_inputs(n, s, seed, noise=True, noise_std=0.3, smooth=False):
    """One input set (float32, CPU).  Per sample x = delta relu(dens) is drawn from four kinds: dens <= 0; 1e-7 <= x < 1e-4; a moderate
    x <= 2.5; 25 <= x <= 60 = saturated, f at its 1e-10 floor; nothing in between, where 1 - E crosses float32 rounding steps that are
    large against f (header).  Four saturated samples take the transmittance below float32's range, so a ray has none before its own
    index j0 (spread over [0, S) by the golden ratio: some rays stay alive across every 64-sample segment boundary, which is what the
    segment carries need) and many behind it: 30 / 15 / 55 / 0 % in front (the moderate x scaled so that their sum stays near 20),
    30 / 12 / 18 / 40 % behind.  The last sample (delta = 1e10) is dens <= 0 or dens >= 1.
    Rays of n >= 9: ray 0 has every dens <= 0; ray 1 is opaque at its first sample; rays 1..3 carry an albedo scaled to 1.26..1.8, a
    sun_v in [0.9, 1] and an early opaque sample, so that a channel clamps at 1; ray 4 has j0 = S - 1 and a last sample with dens >= 1.
    ``smooth``: moderate x everywhere (no saturated alpha) and colours inside (0, 1)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)  # noqa: E731
    z = (0.1 + torch.cumsum((0.2 + rnd(n, s)) / s, -1)).float()
    delta = torch.cat([(z[:, 1:] - z[:, :-1]).double(), torch.ones(n, 1, dtype=torch.float64)], -1)
    cat = rnd(n, s)
    x_tiny = 10.0 ** (-7.0 + 2.9 * rnd(n, s))
    x_mod = 0.01 + 2.49 * rnd(n, s)
    x_sat = 25.0 + 35.0 * rnd(n, s)
    neg = -3.0 * rnd(n, s)
    if smooth:
        dens = x_mod * min(1.0, 8.0 / s) / delta
        dens[:, -1] = -1.0          # the last sample would saturate
    else:
        j0 = (((torch.arange(n, dtype=torch.float64) * 0.6180339887) % 1.0) * s).floor().unsqueeze(-1)
        if n >= 9:
            j0[4] = s - 1           # ray 4 reaches its last sample alive and is opaque there: the one place the 1e10 interval is seen
        front = torch.arange(s, dtype=torch.float64).unsqueeze(0) < j0
        x_front = torch.where(cat < 0.45, x_tiny, x_mod * torch.clamp(30.0 / j0.clamp(min=1.0), max=1.0))
        x_back = torch.where(cat < 0.42, x_tiny, torch.where(cat < 0.60, x_mod, x_sat))
        dens = torch.where(cat < 0.30, neg, torch.where(front, x_front, x_back) / delta)
        dens[:, -1] = torch.where(cat[:, -1] < 0.5, neg[:, -1], 1.0 + x_mod[:, -1])
        if n >= 9:
            dens[0] = neg[0]
            dens[4, -1] = 1.0 + x_mod[4, -1]
            dens[1, 0] = x_sat[1, 0] / delta[1, 0]
            if s > 2:
                dens[2:4, :2] = x_mod[2:4, :2] / delta[2:4, :2]
                dens[2:4, 2] = x_sat[2:4, 2] / delta[2:4, 2]
    nz = torch.randn(n, s, generator=g, dtype=torch.float64).float() if noise else None
    sigma = dens if nz is None else dens - nz.double() * float(np.float32(noise_std))
    albedo = 0.05 + 0.9 * rnd(n, s, 3)
    sun_v = rnd(n, s)
    if not smooth and n >= 9:
        albedo[1:4] = 1.8 * (0.7 + 0.3 * rnd(3, s, 3))
        sun_v[1:4] = 0.9 + 0.1 * rnd(3, s)
    return {"z": z, "sigma": sigma.float(), "noise": nz, "noise_std": noise_std if noise else 0.0, "albedo": albedo.float(),
            "sun_v": sun_v.float(), "beta": (0.01 + 0.99 * rnd(n, s)).float(), "sky": (0.05 + 0.9 * rnd(n, 3)).float(),
            "target": rnd(n, 3).float()}


def coverage(inp):
    """What an input set reaches, from the reference alone: shares of saturated / dens <= 0 / tiny-x samples, the special rays, clamped
    rays, and the two undecidable kinds (both must be 0)."""
    out = composite(inp["z"], inp["sigma"], inp["noise"], inp["noise_std"], inp["albedo"], inp["sun_v"], inp["sky"])
    ch = out["chain"]
    f, c = ch.f.v.detach(), out["c"].v.detach()
    return {"saturated": float((f == c32(1e-10)).double().mean()), "dens_le_0": float((ch.dens <= 0).double().mean()),
            "tiny_x": float(((ch.x > 0) & (ch.x < 1e-4)).double().mean()),
            "all_off_rays": int((ch.dens <= 0).all(-1).sum()), "opaque_first_rays": int((f[:, 0] == c32(1e-10)).sum()),
            "clamped_rays": int((c > 1).any(-1).sum()), "undecided_clamp": undecided_clamp(out["c"], ch),
            "undecided_f": int((ch.ambs[2] > AMB_F_MAX * f).sum())}


# ---------------------------------------------------------------------------------------------------------------------- cases
# The input sets both test modules run: the host module with the float32 emulation as "the kernel", the GPU module with satnerf_amd.ops.
# sr_composite_fwd / sr_composite_bwd take sun_v and sky together or not at all, so "no sun_v" and "no sky" are one variant.
COMPOSITE_VARIANTS = ("full", "sigma_only", "no_sun_sky", "clamp_off", "no_g_rgb", "no_g_depth", "no_g_w", "no_g_T", "noise")
CASES = {
    "render_loss": [dict(n=n, s=s, noise=nz, warm=warm) for n, s in ((37, 64), (37, 63), (5, 7), (1, 2), (3, 1)) for nz in (True, False)
                    for warm in (False, True)],
    "composite": [dict(n=9, s=s, variant=v, noise=v == "noise") for s in (64, 50, 128, 130, 192, 1) for v in COMPOSITE_VARIANTS],
    "satnerf_loss": [dict(n=37, s=128, noise=True, grad_scale=gs, warm=warm) for gs in (1.0, 0.5) for warm in (False, True)],
    "sc_loss": [dict(n=9, s=s, noise=nz) for s in (64, 130) for nz in (True, False)],
    "depth_loss": [dict(n=n, stride=st, use_weights=uw) for n in (1, 257) for st in (2, 3) for uw in (True, False)],
    "composite_image": [dict(n=9, s=s, noise=True) for s in (50, 128)],
}
LAMBDA_SC, LAMBDA_DS = 0.05, 1000.0   # the project's defaults
_INPUTS = {}


def case_id(case):
    return "-".join(f"{k}={v}" for k, v in case.items())


def case_inputs(kind, case):
    """The case's input set (built once; nobody writes to it)."""
    key = (kind, case_id(case))
    if key in _INPUTS:
        return _INPUTS[key]
    if kind == "depth_loss":
        g = torch.Generator().manual_seed(11 + case["n"])
        inp = {"depth": (5 * torch.rand(case["n"], generator=g)).float(), "depths": (5 * torch.rand(case["n"], case["stride"], generator=g)).float()}
    else:
        inp = make_inputs(case["n"], case["s"], 100 + case["s"], noise=case["noise"])
        g = torch.Generator().manual_seed(7)
        n, s = case["n"], case["s"]
        if kind == "composite":
            v = case["variant"]
            gs = {"g_rgb": torch.randn(n, 3, generator=g), "g_depth": torch.randn(n, generator=g), "g_w": torch.randn(n, s, generator=g),
                  "g_T": torch.randn(n, s, generator=g)}
            if v.startswith("no_g_"):
                gs[v[3:]] = None
            inp.update(gs, clamp=v != "clamp_off")
            if v == "sigma_only":
                inp["albedo"] = None
            if v in ("sigma_only", "no_sun_sky"):
                inp["sun_v"] = inp["sky"] = None
        if kind == "satnerf_loss":   # the separate kernel reads a forward's outputs: any float32 data of that shape
            fwd = composite(inp["z"], inp["sigma"], inp["noise"], inp["noise_std"], inp["albedo"], inp["sun_v"], inp["sky"])
            inp["rgb"], inp["weights"] = fwd["rgb"].v.detach().float(), fwd["weights"].v.detach().float()
    _INPUTS[key] = inp
    return inp


_RAY = ("z", "sigma", "noise", "noise_std")


def _call(kind, case, inp, mode, fault=None, got=None):
    a = [inp[k] for k in _RAY] if kind != "depth_loss" and kind != "satnerf_loss" else None
    if kind == "render_loss":
        return render_loss(*a, inp["albedo"], inp["sun_v"], inp["beta"], inp["sky"], inp["target"], warm=case["warm"], mode=mode, fault=fault)
    if kind == "composite":
        fwd = composite(*a, inp["albedo"], inp["sun_v"], inp["sky"], inp["clamp"], mode=mode, fault=fault)
        src = got if got is not None else {k: fwd[k].v.detach() for k in ("weights", "transp")}
        bwd = composite_grads(*a, inp["albedo"], inp["sun_v"], inp["sky"], inp["clamp"], inp["g_rgb"], inp["g_depth"], inp["g_w"], inp["g_T"],
                              weights=src["weights"].detach().cpu(), transp=src["transp"].detach().cpu(), mode=mode, fault=fault)
        out = {k: fwd[k] for k in ("weights", "transp", "depth", "rgb")}
        out.update({k: bwd[k] for k in ("d_sigma", "d_sky") + (() if inp["albedo"] is None else ("d_albedo", "d_sun"))})   # sigma-only: not written
        out["chain"], out["chain_bwd"], out["c"], out["c_bwd"] = fwd["chain"], bwd["chain"], fwd["c"], bwd["c"]
        return out
    if kind == "satnerf_loss":
        return satnerf_loss(inp["rgb"], inp["weights"], inp["beta"], inp["target"], grad_scale=case["grad_scale"], warm=case["warm"], mode=mode,
                            fault=fault)
    if kind == "sc_loss":
        return sc_loss(*a, inp["sun_v"], LAMBDA_SC, mode=mode, fault=fault)
    if kind == "depth_loss":
        return depth_loss(inp["depth"], inp["depths"], LAMBDA_DS, case["use_weights"], mode=mode, fault=fault)
    if kind == "composite_image":
        return composite_image(*a, inp["albedo"], inp["sun_v"], inp["beta"], inp["sky"], mode=mode, fault=fault)
    raise KeyError(kind)


def emulate(kind, case, fault=None):
    """The float32 emulation's outputs as a kernel would return them: {name: float32 tensor, "loss": float}."""
    out = _call(kind, case, case_inputs(kind, case), "emu", fault)
    return {k: (v.v if isinstance(v, V) else v) for k, v in out.items() if k == "loss" or (isinstance(v, V) and k not in ("c", "c_bwd", "contrib", "b"))}


def compare(kind, case, got):
    """Every output of ``got`` (from ``emulate`` or from the device) against the reference under its gate -> {name: worst ratio}; asserts
    that no clamp of the case is undecidable (the rays left out are none)."""
    ref = _call(kind, case, case_inputs(kind, case), "ref", got=got)
    res = {}
    for k, v in ref.items():
        if not isinstance(v, V) or k in ("c", "c_bwd", "contrib", "b"):
            continue
        ch = ref.get("chain_bwd" if k.startswith("d_") and "chain_bwd" in ref else "chain")
        res[k] = ratio(got[k].cpu(), v, ch)[0]
    if "loss" in ref:
        res["loss"] = float(abs(float(got["loss"]) - float(ref["loss"])) / ref["loss_gate"])
    for ck, chk in (("c", "chain"), ("c_bwd", "chain_bwd")):
        if ref.get(ck) is not None and case.get("variant") != "clamp_off":
            assert undecided_clamp(ref[ck], ref.get(chk)) == 0, (kind, case, ck)
    return res
