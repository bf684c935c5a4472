"""High-precision reference of the weight-gradient contraction (csrc/wgrad.hip, wgrad8.hip, wgrad9.hip), restated from the sources.

* Decoders: a dpre / acts training workspace (SR_FMT16 or SR_FMT8, mlp_layout.h) -> the logical per-fragment matrices [points, 16] the
  kernels contract, in float64 (torch: the same code runs on the CPU and on the GPU).
* Operand models: what each kernel actually multiplies (its operand rounding), so that only fp32 accumulation order is left between a
  kernel and the modelled reference.
* Plan restatements: sr_wgrad_plan (wgrad.hip) and the way each kernel maps a workgroup to (job block, partial slot, tile range).

A plain helper module, imported by the tests (not a conftest)."""
import math

import numpy as np
import torch

from satnerf_amd import packing

KIND_BF16, KIND_PHASE = packing.KIND_BF16, packing.KIND_PHASE
TABLE_INTS, SLICES, FIRST, SPAN = 12, 9, 10, 11
PLAN_UNITS = 208          # mlp_layout.h kWg9PlanUnits
EMAX_TILES = 4            # mlp_layout.h kEmaxTiles
GATE = 2.0 ** -19         # |got - modelled reference| <= GATE * sum |dpre * act| for slices of <= 256 tiles (tests/test_hip_wgrad_reference.py)


def ws_tiles(n_points):
    """common.h ws_tiles: tiles a workspace holds (whole groups of 8)."""
    return ((n_points + 31) // 32 + 7) // 8 * 8


def wgrad9_fits(n_tiles, ak=PLAN_UNITS, dk=PLAN_UNITS):
    return n_tiles * max(ak, dk) * 1024 < (1 << 32)


# ---------------------------------------------------------------------------------------------------------------- decoding
# One 1-KiB unit = 64 lanes x 16 B; lane (p, h) = (lane & 31, lane >> 5) holds point p of the tile.  A bf16 fragment: element j of the lane
# = slot 8 h + j.  A double fragment (SR_FMT8): byte n of the lane = half n >> 3 (logical fragment 2 t + half), slot 8 h + (n & 7).

def _units(ws, units_per_tile, n_tiles):
    """int16 / uint8 workspace tensor -> uint8 view [n_tiles, units_per_tile, 64, 16] (only the first n_tiles tiles)."""
    b = ws.view(torch.uint8) if ws.dtype != torch.uint8 else ws
    return b[:n_tiles * units_per_tile * 1024].view(n_tiles, units_per_tile, 64, 16)


def _lane_major(x):
    """[tiles, 64, 16 | 8] per-lane values -> [tiles * 32, 16] point x slot (lane (p, h), element j -> slot 8 h + j; 16 bytes: 2 halves)."""
    t = x.shape[0]
    if x.shape[-1] == 8:
        return x.view(t, 2, 32, 8).permute(0, 2, 1, 3).reshape(t * 32, 16)
    return x.view(t, 2, 32, 2, 8).permute(3, 0, 2, 1, 4).reshape(2, t * 32, 16)   # [half, point, slot]


def bf16_bits_to_f64(bits16):
    return (bits16.to(torch.int32) << 16).view(torch.float32).to(torch.float64)


def _bf16_unit(u8):
    """[tiles, 64, 16] uint8 -> [points, 16] float64 of a bf16 fragment."""
    t = u8.shape[0]
    h = u8.contiguous().view(torch.int16).view(t, 64, 8)
    return _lane_major(bf16_bits_to_f64(h.to(torch.int32) & 0xffff))


class Operand:
    """One logical fragment: codec 'raw' (bf16 values), 'mx' (codes u and lane exponents E), 'ph8' / 'ph16' (phase codes u); [P, 16]."""

    def __init__(self, codec, val=None, u=None, e=None, group=None):
        self.codec, self.val, self.u, self.e, self.group = codec, val, u, e, group

    def exact(self):
        if self.codec == "raw":
            return self.val
        if self.codec == "mx":
            return (self.u.to(torch.float64) - 128.0) * torch.exp2(self.e.to(torch.float64) - 133.0)
        n = 256.0 if self.codec == "ph8" else 65535.0
        return torch.sin(2 * math.pi * self.u.to(torch.float64) / n)

    def revolutions(self):
        """Phase codecs: the saved pre-activation phase in revolutions (what the dX kernel takes the cos of, tests/dx_reference.py)."""
        assert self.codec in ("ph8", "ph16")
        return self.u.to(torch.float64) / (256.0 if self.codec == "ph8" else 65535.0)


def decode_workspaces(dpre, acts, n_points, feat, tau, fmt):
    """-> (rows: {dpre fragment: Operand}, cols: {act fragment (aux offset included): Operand}, emax table uint8 [entries, 16] or None)
    over the n_tiles = ceil(n_points / 32) tiles a kernel reads (padding points of the last tile included)."""
    auxs = packing.aux_steps(tau)
    n_tiles = (n_points + 31) // 32
    bm = packing.backward_maps(feat, tau)
    kinds = {}
    for b, cols in enumerate(bm["block_cols"]):
        for c in cols:
            kinds[c] = int(bm["blocks"][b, 8])
    row_frags = sorted({f for rows in bm["block_rows"] for f in rows})
    col_frags = sorted(set(kinds))
    rows, cols = {}, {}
    if fmt == 16:
        ks, hs = feat // 16, feat // 32
        dk = 9 * ks + 1 + 5 * hs + 1
        ak = auxs + 9 * ks + 5 * hs
        D, A = _units(dpre, dk, n_tiles), _units(acts, ak, n_tiles)
        for f in row_frags:
            rows[f] = Operand("raw", val=_bf16_unit(D[:, f]))
        for f in col_frags:
            if kinds[f] == KIND_PHASE:
                h = A[:, f].contiguous().view(torch.int16).view(n_tiles, 64, 8).to(torch.int32) & 0xffff
                cols[f] = Operand("ph16", u=_lane_major(h))
            else:
                cols[f] = Operand("raw", val=_bf16_unit(A[:, f]))
        for a in range(auxs):
            cols[("aux", a)] = Operand("raw", val=_bf16_unit(A[:, a]))
        return rows, cols, None
    g8 = packing.fmt8_geometry(feat)
    dk, ak = packing.dpre8_units(feat), packing.act8_units(auxs, feat)
    D, A = _units(dpre, dk, n_tiles), _units(acts, ak, n_tiles)
    for ws, frags, src_of in ((D, row_frags, lambda f: packing.dpre8_source(f, feat)), (A, col_frags, lambda f: packing.act8_source(f, auxs, feat))):
        out = rows if ws is D else cols
        for f in frags:
            s = src_of(f)
            if s["codec"] == packing.RAW16:
                out[f] = Operand("raw", val=_bf16_unit(ws[:, s["unit"]]), group=s.get("group"))
                continue
            u = _lane_major(ws[:, s["unit"]].to(torch.int32))[s["half"]]
            if s["codec"] == packing.PHASE8:
                out[f] = Operand("ph8", u=u)
            else:
                e = ws[:, s["scale_unit"], :, s["scale_byte"]].to(torch.int32)     # [tiles, 64]: the lane's exponent
                e = e.view(n_tiles, 2, 32).permute(0, 2, 1).reshape(n_tiles * 32, 2)  # [point, h]
                e = e.repeat_interleave(8, dim=1)                                   # slot 8 h + j
                out[f] = Operand("mx", u=u, e=e, group=s.get("group"))
    for a in range(auxs):
        cols[("aux", a)] = Operand("raw", val=_bf16_unit(A[:, a]))
    b = dpre.view(torch.uint8) if dpre.dtype != torch.uint8 else dpre
    off = ws_tiles(n_points) * dk * 1024
    emax = b[off:off + (n_tiles + EMAX_TILES - 1) // EMAX_TILES * 16].view(-1, 16)
    return rows, cols, emax


# ---------------------------------------------------------------------------------------------------------------- operand models
_NMANT = {torch.bfloat16: 7, torch.float16: 10}


def _round_with_ambiguity(v, dtype, tol):
    """RNE of v into ``dtype``, and the operand error a hardware function accurate to ``tol`` (absolute) might add: one ulp where v lies
    within tol of a rounding midpoint, else 0."""
    r = v.to(dtype).to(torch.float64)
    fin = torch.finfo(dtype)
    ulp = torch.exp2(torch.floor(torch.log2(r.abs().clamp_min(fin.tiny))) - _NMANT[dtype])
    near = ((v - r).abs() - ulp / 2).abs() <= tol
    return r, torch.where(near, ulp, torch.zeros_like(v))


# The sin accuracies below are assumptions, not documented bounds: the CDNA ISA guides give no error bound for v_sin_f32 / v_sin_f16.  They
# are what the kernels have met on MI355X so far (captured and synthetic workspaces, tests/test_hip_wgrad_reference.py): a hardware sin
# further from the true value than assumed would show there as a gate failure, not pass unnoticed.
EPS_SIN = 2.0 ** -19      # v_sin_f32: taken to be within this of the true sine (tests/fwd_reference.py makes the same assumption)


def model_operand(op, kernel, g=None):
    """(value, ambiguity) of what ``kernel`` multiplies for this operand.  ``g`` (wgrad9 only): the exponent E_max the kernel fitted fp16's
    range to for this operand (a row pair's, or the feats columns'), per point [P, 1] -- it changes along the slices."""
    z = torch.zeros_like(op.exact() if op.codec != "raw" else op.val)
    if kernel in ("wgrad", "wgrad8"):
        if op.codec == "raw":
            return op.val, z
        if op.codec == "mx":   # mx8_value: fma(u, s, -128 s), s = 2^(E-133) built as bits (E - 6) << 23: E = 6 decodes as 0; exact in bf16
            return torch.where(op.e > 6, op.exact(), z), z
        # v_sin_f32 of the phase, packed to bf16 (RNE): v_sin_f32 taken to be within 2^-19 of sin (assumed, see above)
        return _round_with_ambiguity(op.exact(), torch.bfloat16, EPS_SIN)
    assert kernel == "wgrad9"
    if op.codec == "mx":   # fp16 (u - 128) * 2^(E - er + 20 - 15), er = g - 20 ... a lane whose exponent field E - (g - 20) <= 0 flushes to 0
        keep = (op.e - (g - 20)) > 0
        return torch.where(keep, op.exact(), z), z
    if op.codec == "raw":   # bf16 * 2^(138 - g) -> fp16 (RNE, subnormals kept) -> unscaled (rows); aux columns: g None, scale 1
        s = 1.0 if g is None else torch.exp2(138.0 - g.to(torch.float64))
        return (op.val * s).to(torch.float16).to(torch.float64) / s, z
    # PHASE8 columns: two v_sin_f16 per pair of codes; v_sin_f16 taken to be within a quarter fp16 ulp of sin (assumed, see above)
    v = op.exact()
    fin = torch.finfo(torch.float16)
    r = v.to(torch.float16).to(torch.float64)
    ulp = torch.exp2(torch.floor(torch.log2(r.abs().clamp_min(fin.tiny))) - _NMANT[torch.float16])
    return _round_with_ambiguity(v, torch.float16, 0.0)[0], torch.where(((v - r).abs() - ulp / 2).abs() <= ulp / 4, ulp, z)


# ---------------------------------------------------------------------------------------------------------------- the planner
def _split_by_cost(cost, n_tiles, n_wg):
    nb = len(cost)
    sl = [1] * nb
    finish = lambda b: cost[b] * float((n_tiles + sl[b] - 1) // sl[b])  # noqa: E731
    for _ in range(n_wg - nb):
        worst, wt = -1, -1.0
        for b in range(nb):
            if finish(b) > wt and sl[b] < n_tiles:
                wt, worst = finish(b), b
        if worst < 0:
            break
        sl[worst] += 1
    return sl, max(finish(b) for b in range(nb))


def plan(blocks, n_points, n_wg, fmt, env=None, v1=False):
    """sr_wgrad_plan restated: returns (planned table, n_slices).  ``env``: the SATNERF_WGRAD_* switches the planner reads (dict)."""
    env = env or {}
    t = np.array(blocks, np.int32).copy()
    nb = t.shape[0]
    n_tiles = (n_points + 31) // 32
    span = 0
    if fmt != 8 or nb > n_wg:
        per = max(1, min(n_wg // nb, n_tiles))
        sl = [per] * nb
    elif v1:
        cost = [0.4 + 0.02 * (r[1] + r[3]) + 0.0175 * (r[5] + r[7]) for r in t]
        sl, _ = _split_by_cost(cost, n_tiles, n_wg)
    else:
        thin16, thin8 = 0.5, 0.4
        thin_on = env.get("SATNERF_WGRAD_THIN", "1")[:1] != "0"
        cost, any_thin = [], False
        for r in t:
            nr, nc = r[1] + r[3], r[5] + r[7]
            thin = thin_on and nr == 1 and r[8] == 1 and nc in (8, 16)
            cost.append((thin16 if nc == 16 else thin8) if thin else 1.0)
            any_thin |= thin and cost[-1] != 1.0
        sk_env = env.get("SATNERF_WGRAD_STREAMK")
        span_k = (nb * n_tiles + n_wg - 1) // n_wg
        weighted = False
        if any_thin and nb <= 64:
            sl, makespan = _split_by_cost(cost, n_tiles, n_wg)
            weighted = (sk_env[:1] != "1") if sk_env is not None else (makespan <= span_k * 1.03 or not wgrad9_fits(n_tiles))
        if not weighted:
            q, r = n_wg // nb, n_wg % nb
            worst = (n_tiles + q - 1) // q
            sl = [min(q + (b < r), n_tiles) for b in range(nb)]
            streamk = (sk_env[:1] == "1") if sk_env is not None else (span_k >= 8 and worst * 100 > span_k * 103)
            if streamk and wgrad9_fits(n_tiles):
                sl = [((b + 1) * n_tiles - 1) // span_k - (b * n_tiles) // span_k + 1 for b in range(nb)]
                span = span_k
    t[0, SPAN] = span
    first = 0
    for b in range(nb):
        t[b, SLICES], t[b, FIRST] = sl[b], first
        first += sl[b]
    return t, first


# ---------------------------------------------------------------------------------------------------------------- workgroup -> work
def _block_major(t, n_slices, n_tiles):
    nb = t.shape[0]
    out = []
    for wg in range(n_slices):
        b = 0
        while b + 1 < nb and wg >= t[b, FIRST] + t[b, SLICES]:
            b += 1
        tps = (n_tiles + t[b, SLICES] - 1) // t[b, SLICES]
        t0 = (wg - t[b, FIRST]) * tps
        out.append((wg, b, wg, t0, max(t0, min(t0 + tps, n_tiles))))
    return out


def work_of(kernel, t, n_slices, n_tiles):
    """Each workgroup's (workgroup, block, partial slot written, first tile, end tile) for a launch of ``n_slices`` workgroups on the planned
    table ``t`` -- the kernel's own numbering, restated.  wgrad.hip / wgrad8.hip: block-major search, slot = blockIdx; wgrad9.hip: the
    arithmetic equal split, the slice-major level walk of weighted plans (<= 64 blocks), block-major search otherwise, stream-K spans."""
    t = np.asarray(t)
    if kernel in ("wgrad", "wgrad8"):
        return _block_major(t, n_slices, n_tiles)
    nb = t.shape[0]
    span = int(t[0, SPAN])
    out = []
    if span > 0:
        u_all = nb * n_tiles
        for wg in range(n_slices):
            u0 = wg * span
            if u0 >= u_all:
                continue
            u_end = min(u0 + span, u_all)
            while True:
                b = u0 // n_tiles
                sb = u0 - b * n_tiles
                se = min(sb + (u_end - u0), n_tiles)
                sl = wg - (b * n_tiles) // span
                out.append((wg, b, int(t[b, FIRST]) + sl, sb, se))
                u0 += se - sb
                if u0 >= u_end:
                    break
        return out
    q, r = n_slices // nb, n_slices % nb
    equal = q > 0 and all(t[b, SLICES] == q + (b < r) for b in range(nb))
    levels = [(b, lvl) for lvl in range(int(t[:, SLICES].max())) for b in range(nb) if t[b, SLICES] > lvl]   # slice-major order
    for wg in range(n_slices):
        if equal:
            b, sl = (wg % nb, wg // nb) if wg < q * nb else (wg - q * nb, q)
        elif nb <= 64:
            b, sl = levels[wg] if wg < len(levels) else (nb - 1, 0)
        else:
            b = next(x for x in range(nb) if t[x, FIRST] <= wg < t[x, FIRST] + t[x, SLICES])
            sl = wg - t[b, FIRST]
        tps = (n_tiles + t[b, SLICES] - 1) // t[b, SLICES]
        t0 = sl * tps
        out.append((wg, b, int(t[b, FIRST]) + sl, t0, max(t0, min(t0 + tps, n_tiles))))
    return out


def check_coverage(work, t, n_slices, n_tiles):
    """Every (block, tile < n_tiles) covered exactly once; every partial slot of a block (the ones sr_unpack_grads / sr_grad_tail sum)
    written exactly once, by that block, inside [0, n_slices).  Returns a list of problems (empty = fine)."""
    t = np.asarray(t)
    nb = t.shape[0]
    bad = []
    cover = np.zeros((nb, n_tiles), np.int32)
    writes = {}
    for wg, b, slot, t0, t1 in work:
        cover[b, t0:t1] += 1
        if not (0 <= slot < n_slices):
            bad.append(("slot outside n_slices", wg, b, slot))
        if not (t[b, FIRST] <= slot < t[b, FIRST] + t[b, SLICES]):
            bad.append(("slot outside its block's slices", wg, b, slot))
        writes[slot] = writes.get(slot, 0) + 1
    if (cover != 1).any():
        b, tl = np.argwhere(cover != 1)[0]
        bad.append(("tile covered %d times" % cover[b, tl], int(b), int(tl)))
    for b in range(nb):
        for s in range(t[b, FIRST], t[b, FIRST] + t[b, SLICES]):
            if writes.get(int(s), 0) != 1:
                bad.append(("slot written %d times" % writes.get(int(s), 0), b, int(s)))
    if int(t[:, SLICES].sum()) != n_slices:
        bad.append(("slices of the table != n_slices", int(t[:, SLICES].sum()), n_slices))
    return bad


# ---------------------------------------------------------------------------------------------------------------- the contraction
def block_operands(feat, tau, b):
    """(row fragments, column fragments incl. ("aux", a)) of job block b; partial layout: main [16 nr, 16 nc] at row * 256 + col, aux
    columns at 256 * 256 + row * 32 + 16 a + slot."""
    bm = packing.backward_maps(feat, tau)
    return list(bm["block_rows"][b]), list(bm["block_cols"][b]) + [("aux", a) for a in range(bm["auxs"])]


def _slot_positions(nr, cols):
    n_main = sum(1 for c in cols if not isinstance(c, tuple))
    r = torch.arange(16 * nr)[:, None]
    pos = []
    for j, c in enumerate(cols):
        cs = torch.arange(16)[None, :]
        if isinstance(c, tuple):
            pos.append(256 * 256 + r * 32 + 16 * c[1] + cs)
        else:
            pos.append(r * 256 + 16 * j + cs)
    assert n_main <= 16
    return torch.cat(pos, 1)    # [16 nr, 16 ncols]


def reference(feat, tau, rows, cols, n_points, kernel=None, work=None, emax=None, blocks_loads=None):
    """Per block b: (positions in the partial block [16 nr, 16 n_cols], R_b exact, A_b = sum |dpre act|, M_b = modelled reference of
    ``kernel`` (None: R_b), B_b = operand-ambiguity bound).  Sums over points < n_points.  wgrad9: ``work`` (work_of) and ``emax``
    (the dX kernel's table) give each slice's fitted range; ``blocks_loads`` = packing.wgrad8_loads (pair groups)."""
    bm = packing.backward_maps(feat, tau)
    out = []
    for b in range(len(bm["block_rows"])):
        rf, cf = block_operands(feat, tau, b)
        X = torch.cat([rows[f].exact()[:n_points] for f in rf], 1)
        Y = torch.cat([cols[c].exact()[:n_points] for c in cf], 1)
        R = X.T @ Y
        A = X.abs().T @ Y.abs()
        pos = _slot_positions(len(rf), cf).to(R.device)
        if kernel is None:
            out.append((pos, R, A, R, torch.zeros_like(R)))
            continue
        if kernel != "wgrad9":
            Xm, Xa = zip(*(model_operand(rows[f], kernel) for f in rf))
            Ym, Ya = zip(*(model_operand(cols[c], kernel) for c in cf))
            Xm, Xa, Ym, Ya = (torch.cat(v, 1)[:n_points] for v in (Xm, Xa, Ym, Ya))
            M = Xm.T @ Ym
            B = Xm.abs().T @ Ya + Xa.T @ Ym.abs() + Xa.T @ Ya
            out.append((pos, R, A, M, B))
            continue
        # wgrad9: the fitted range depends on the slice -- contract each piece of work with its own E_max
        groups = packing.wgrad9_pair_groups(feat, tau)[b]
        M = torch.zeros_like(R)
        B = torch.zeros_like(R)
        for _, wb, _, t0, t1 in work:
            if wb != b or t1 <= t0:
                continue
            ent = emax[t0 // EMAX_TILES:(t1 - 1) // EMAX_TILES + 1].to(torch.int64).amax(0)
            clamp = lambda e: min(max(int(e), 32), 254)  # noqa: E731
            p0, p1 = 32 * t0, min(32 * t1, n_points)
            if p1 <= p0:
                continue
            xs, xa = [], []
            for j, f in enumerate(rf):
                g = groups[j // 2]
                e = clamp(ent[g]) if g >= 0 else 32
                gt = torch.tensor(e, device=R.device)
                op = rows[f]
                sub = Operand(op.codec, val=None if op.val is None else op.val[p0:p1], u=None if op.u is None else op.u[p0:p1],
                              e=None if op.e is None else op.e[p0:p1])
                v, a = model_operand(sub, "wgrad9", gt)
                xs.append(v), xa.append(a)
            ys, ya = [], []
            ec = clamp(ent[packing.EMAX_FEATS])
            for c in cf:
                op = cols[c]
                sub = Operand(op.codec, val=None if op.val is None else op.val[p0:p1], u=None if op.u is None else op.u[p0:p1],
                              e=None if op.e is None else op.e[p0:p1])
                v, a = model_operand(sub, "wgrad9", None if isinstance(c, tuple) else torch.tensor(ec, device=R.device))
                ys.append(v), ya.append(a)
            Xm, Xa, Ym, Ya = torch.cat(xs, 1), torch.cat(xa, 1), torch.cat(ys, 1), torch.cat(ya, 1)
            M += Xm.T @ Ym
            B += Xm.abs().T @ Ya + Xa.T @ Ym.abs() + Xa.T @ Ya
        out.append((pos, R, A, M, B))
    return out


def sum_slices(partial, t, b):
    """fp64 sum of block b's partial slots -> [kWgBlockFloats]."""
    bf = packing.WG_BLOCK_FLOATS
    f, n = int(t[b, FIRST]), int(t[b, SLICES])
    return partial[f * bf:(f + n) * bf].view(n, bf).to(torch.float64).sum(0)


def kernel_for(fmt, feat, tau, n_tiles, v1=False):
    """Which kernel a launch runs: wgrad.hip for SR_FMT16; for SR_FMT8 the 4-wave kernel unless SATNERF_WGRAD_V1=1 or the workspaces exceed its
    32-bit per-lane offsets (checked with the real units per tile, sr_satnerf_wgrad8), then the r02 kernel."""
    if fmt != 8:
        return "wgrad"
    ak, dk = packing.act8_units(packing.aux_steps(tau), feat), packing.dpre8_units(feat)
    return "wgrad8" if v1 or not wgrad9_fits(n_tiles, ak, dk) else "wgrad9"


# ---------------------------------------------------------------------------------------------------------------- synthetic workspaces
def emax_table(D, A, n_points, feat, tau):
    """The table of exponent maxima the dX kernel leaves behind the dpre workspace, restated (tests/test_hip_emax.py): one 16-byte entry
    per EMAX_TILES tiles of the workspace; byte g < 14 = largest scale byte of dpre group g, 14 = of the feats scale bytes, 15 = largest
    biased exponent of the bf16 rows d_sigma_pre / d_head.  D, A: uint8 views [ws_tiles, units, 64, 16]."""
    g8 = packing.fmt8_geometry(feat)
    tiles = D.shape[0]
    mt, gpu = g8["MT"], g8["GROUPS_PER_UNIT"]
    out = torch.zeros(tiles // EMAX_TILES, 16, dtype=torch.uint8, device=D.device)
    per4 = lambda x: x.reshape(tiles // EMAX_TILES, -1).amax(1)  # noqa: E731
    for g in range(14):
        nb = mt if g < 9 else g8["MTH"]
        out[:, g] = per4(D[:, g8["D8_SCALE"] + g // gpu, :, (g % gpu) * mt:(g % gpu) * mt + nb])
    out[:, packing.EMAX_FEATS] = per4(A[:, packing.aux_steps(tau) + g8["A8_SCALE"], :, :mt])
    raw = torch.stack([D[:, g8["D8_SIGMA"]], D[:, g8["D8_HEAD"]]], 1).contiguous().view(torch.int16).to(torch.int32) & 0x7fff
    out[:, packing.EMAX_RAW] = per4((raw >> 7).to(torch.uint8))
    return out


def synthetic_fmt8(feat, tau, n_points, device, gen, group_e, raw_e=(100, 127), zero_groups=(), live_tiles=None, pad_zero=True):
    """A pair of SR_FMT8 workspaces (dpre with its table of exponent maxima, acts) of random content, as flat uint8 tensors.

    ``group_e[g]`` = (lo, hi) of the MX8 exponent bytes of dpre scale group g (lanes spread inside: some fall 20+ binades below their pair's
    maximum and flush in wgrad9); ``raw_e`` = range of the biased exponents of the bf16 rows d_sigma_pre / d_head; ``zero_groups``: scale
    groups whose exponent bytes all hold the clamp minimum E = 6 (what the encoder writes for an all-zero lane; wgrad8 decodes it as 0,
    wgrad9 flushes it); ``live_tiles``: only these tiles hold data,
    every other tile decodes to zero (MX8 code 128, PHASE8 code 0, bf16 0); ``pad_zero``: dpre of points >= n_points is zero, as the dX
    kernel leaves it (else random: the weight-gradient kernels mask nothing)."""
    g8 = packing.fmt8_geometry(feat)
    auxs = packing.aux_steps(tau)
    dk, ak = packing.dpre8_units(feat), packing.act8_units(auxs, feat)
    wt = ws_tiles(n_points)
    emax_bytes = (wt // EMAX_TILES * 16 + 1023) // 1024 * 1024
    D = torch.zeros(wt * dk * 1024 + emax_bytes, dtype=torch.uint8, device=device)
    A = torch.zeros(wt * ak * 1024, dtype=torch.uint8, device=device)
    Dv, Av = D[:wt * dk * 1024].view(wt, dk, 64, 16), A.view(wt, ak, 64, 16)
    # tiles without data decode to zero as the encoder writes it: MX8 code 128 with the smallest exponent byte E = 6 (codec8.h clamps E to
    # [6, 254]; E < 6 is outside the format -- wgrad8.hip's scale bits (E - 6) << 23 would wrap), PHASE8 code 0, bf16 0
    Dv[:, :g8["D8_SIGMA"]] = 128
    Dv[:, g8["D8_SCALE"]:] = 6
    Av[:, auxs + g8["A8_SCALE"]] = 6
    Av[:, auxs + g8["ACT_FEATS"] // 2:auxs + (g8["ACT_FEATS"] + g8["KS"]) // 2] = 128
    # tiles are addressed by plain slices only: an index kernel over a workspace past 4 GiB (torch's index_put) faults on the device
    sels = [slice(0, (n_points + 31) // 32)] if live_tiles is None else [slice(int(t), int(t) + 1) for t in live_tiles]
    ri = lambda lo, hi, *shape: torch.randint(lo, hi, shape, generator=gen, device=device, dtype=torch.int32).to(torch.uint8)  # noqa: E731

    def bf16(e_lo, e_hi, *shape):
        e = torch.randint(e_lo, e_hi + 1, shape, generator=gen, device=device, dtype=torch.int32)
        m = torch.randint(0, 1 << 8, shape, generator=gen, device=device, dtype=torch.int32)
        s = torch.randint(0, 2, shape, generator=gen, device=device, dtype=torch.int32)
        return ((s << 15) | (e << 7) | (m & 0x7f)).to(torch.int16).view(torch.uint8).view(*shape[:-1], shape[-1] * 2)

    mt, gpu = g8["MT"], g8["GROUPS_PER_UNIT"]
    f0, f1 = auxs + g8["ACT_FEATS"] // 2, auxs + (g8["ACT_FEATS"] + g8["KS"]) // 2
    for sel in sels:
        Dt, At = Dv[sel], Av[sel]
        k = Dt.shape[0]
        Dt[:, :g8["D8_SIGMA"]] = ri(1, 256, k, g8["D8_SIGMA"], 64, 16)
        Dt[:, g8["D8_SIGMA"]:g8["D8_SCALE"]] = bf16(raw_e[0], raw_e[1], k, 2, 64, 8)
        for g in range(14):
            nb = mt if g < 9 else g8["MTH"]
            lo, hi = (6, 6) if g in zero_groups else group_e[g]
            Dt[:, g8["D8_SCALE"] + g // gpu, :, (g % gpu) * mt:(g % gpu) * mt + nb] = ri(lo, hi + 1, k, 64, nb)
        At[:, auxs:auxs + g8["A8_SCALE"]] = ri(0, 256, k, g8["A8_SCALE"], 64, 16)
        At[:, f0:f1] = ri(1, 256, k, f1 - f0, 64, 16)
        At[:, auxs + g8["A8_SCALE"], :, :mt] = ri(118, 131, k, 64, mt)
        At[:, :auxs] = bf16(120, 127, k, auxs, 64, 8)
    n_tiles = (n_points + 31) // 32
    if pad_zero and n_points % 32:   # the last tile's points >= n_points: zero pre-activation gradients (lanes p >= n_points % 32)
        last = Dv[n_tiles - 1].view(dk, 2, 32, 16)
        p = n_points % 32
        last[:g8["D8_SIGMA"], :, p:] = 128
        last[g8["D8_SIGMA"]:g8["D8_SCALE"], :, p:] = 0
    table = D[wt * dk * 1024:wt * dk * 1024 + wt // EMAX_TILES * 16].view(-1, 16)
    if live_tiles is None:
        table[:] = emax_table(Dv, Av, n_points, feat, tau)
    else:   # (only the entries of live tiles: the r02 kernel, the one that runs past 4 GiB, does not read the table)
        for e in sorted({int(t) // EMAX_TILES for t in live_tiles}):
            sl = slice(EMAX_TILES * e, EMAX_TILES * e + EMAX_TILES)
            table[e:e + 1] = emax_table(Dv[sl], Av[sl], n_points, feat, tau)
    return D, A


def gather_tiles(ws, units_per_tile, tiles):
    """A compact copy of the given tiles of a flat uint8 workspace (plain slices: see synthetic_fmt8)."""
    return torch.cat([ws[int(t) * units_per_tile * 1024:(int(t) + 1) * units_per_tile * 1024] for t in tiles])
