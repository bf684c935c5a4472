"""The layer-path kernels of csrc/linear.hip (linear_kernel<kFwd|kDx|kDw>, colsum_kernel, points_along_kernel, positional_map_kernel)
against the float64 reference of tests/linear_reference.py, every output element under the gate derived there.

Every case of linear_reference.CASES runs FWD, DX of each source and DW + colsum through satnerf_amd.ops (ops' torch.empty / torch.zeros
are replaced so that each output lies in a buffer pre-filled with a known pattern and followed by a canary); DX and DW are handed the
device's own y.  What ops cannot express -- ldg / ldy / ldd / the forward's ldy wider than the matrix, a pre-filled d_weight / d_bias, DW
twice into the same buffers -- is driven through the C entries with buffers owned here: padding columns and canaries must keep their bits.
One forward and one DW launch with a single weight / gy element changed by a relative 2^-10 must leave the gate exactly in that column /
row: the comparison is wired to every element.

Worst |error| / gate on MI355X over all cases (a record of one run, 2026-10-21; nothing below depends on it):
    fwd 0.97   dx 0.51   dw 0.39   db 0.03   positional_map 0.63      (points_along: every bit equal)
    fwd: a sigmoid_rgb output near -0.001 is one rounding of 1.002f s - 0.001f, and the gate of one rounding is sharp; the float32
    emulation of tests/test_linear_reference_host.py gives the same four figures to two digits.  No case missed a gate.
fwd / dx / dw rest on EPS_SIN (v_sin_f32 / v_cos_f32) for sine sources and on EPS_EXP / EPS_LOG (expf / log1pf) for softplus and sigmoid
heads; db on EPS_EXP through out_act' of softplus; positional_map on EPS_SINF (library sinf / cosf within one ulp); points_along on nothing:
it is compared bit for bit."""
import pytest
import torch

from . import linear_reference as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PATTERN, CANARY = 0x5a5a5a5a, 1024       # the float32 1.5e16 in every pre-filled word; words behind each buffer
IDS = [L.case_id(c) for c in L.CASES]
_WORST = {}


def _record(kind, value):
    _WORST[kind] = max(_WORST.get(kind, 0.0), float(value))
    print(f"worst |err| / gate  {kind}: {float(value):.3f}  (so far: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(_WORST.items())) + ")")


class Arena:
    """Output buffers with known content: every word PATTERN, CANARY words behind each."""

    def __init__(self):
        self.bufs = []

    def alloc(self, *shape, zero=False):
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else shape
        n = 1
        for s in shape:
            n *= int(s)
        base = torch.empty(n + CANARY, dtype=torch.int32, device=DEV).fill_(PATTERN).view(torch.float32)
        self.bufs.append((base, n))
        out = base[:n].view(*shape)
        return out.zero_() if zero else out

    def intact(self):
        return all(bool((base[n:].view(torch.int32) == PATTERN).all()) for base, n in self.bufs)


class _Torch:
    """``torch`` as satnerf_amd.ops sees it in this module: float32 outputs come from the arena."""

    def __init__(self, arena):
        self._arena = arena

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, dtype=None, device=None):
        return self._arena.alloc(*shape) if dtype == torch.float32 else torch.empty(*shape, dtype=dtype, device=device)

    def zeros(self, *shape, dtype=None, device=None):
        return self._arena.alloc(*shape, zero=True) if dtype == torch.float32 else torch.zeros(*shape, dtype=dtype, device=device)


@pytest.fixture(autouse=True)
def arena(monkeypatch):
    from satnerf_amd import ops

    a = Arena()
    monkeypatch.setattr(ops, "torch", _Torch(a))
    yield a
    torch.cuda.synchronize()
    assert a.intact(), "a kernel wrote behind its output"


def dev(t):
    """A CPU tensor on the device with the memory layout it has here: a view stays a view of a copy of its base."""
    if t is None:
        return None
    base = t._base if t._base is not None else t
    return base.to(DEV).as_strided(t.shape, t.stride(), t.storage_offset())


def dev_srcs(srcs):
    return [(dev(x), act, w0, div) for x, act, w0, div in srcs]


class Dev:
    """The kernels behind the interface of linear_reference.Emu, through satnerf_amd.ops."""

    def fwd(self, srcs, w, b, p, oa):
        from satnerf_amd import ops
        return ops.linear_fwd(dev_srcs(srcs), dev(w), dev(b), p, oa).cpu()

    def dx(self, gy, y, oa, w, col0, target, p):
        from satnerf_amd import ops
        return ops.linear_bwd_input(dev(gy), dev(y), oa, dev(w), col0, dev_srcs([target])[0], p).cpu()

    def dw(self, gy, y, oa, srcs, p, n_out, want_bias=True):
        from satnerf_amd import ops
        gw, gb = ops.linear_bwd_weight(dev(gy), dev(y), oa, dev_srcs(srcs), p, n_out, want_bias)
        return gw.cpu(), (None if gb is None else gb.cpu())


@pytest.mark.parametrize("c", L.CASES, ids=IDS)
def test_layer_kernels_inside_every_gate(c, arena):
    w = L.worst(L.run_case(c, Dev()))
    for k, v in w.items():
        _record(k, v)
    assert all(v <= 1.0 for v in w.values()), w
    assert len(arena.bufs) >= 3


@pytest.mark.parametrize("c", [c for c in L.CASES if any(s[4] != "dense" for s in c["srcs"])], ids=L.case_id)
def test_a_view_and_its_dense_copy_give_the_same_forward_bits(c):
    from satnerf_amd import ops

    t = L.build(c)
    views = dev_srcs(t.srcs)
    assert any(x.stride(0) > x.shape[1] and (x.data_ptr() % 16 or (4 * x.stride(0)) % 16) for x, *_ in views)     # ld > k, rows off 16 bytes
    dense = [(x.contiguous(), act, w0, div) for x, act, w0, div in views]
    assert all(x.data_ptr() % 16 == 0 for x, *_ in dense)
    a = ops.linear_fwd(views, dev(t.w), dev(t.b), t.p, t.oa)
    b = ops.linear_fwd(dense, dev(t.w), dev(t.b), t.p, t.oa)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    gy = dev(t.gy)
    yy = a if t.oa is not None else None
    wa, _ = ops.linear_bwd_weight(gy, yy, t.oa, views, t.p, t.n_out)
    wb, _ = ops.linear_bwd_weight(gy, yy, t.oa, dense, t.p, t.n_out)
    if t.p <= L.KCHUNK:      # one chunk per output tile: no atomic meets another, the order of additions is fixed
        assert torch.equal(wa.view(torch.int32), wb.view(torch.int32))


# ------------------------------------------------------------------------------------------ the C entries, buffers owned here
def _padded(a, t, ld, fill=float("nan")):
    """A device copy of the CPU matrix ``t`` in an arena buffer of leading dimension ``ld``; the padding columns hold ``fill``."""
    buf = a.alloc(t.shape[0], ld)
    buf.fill_(fill)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf


def _untouched(buf, width):
    return bool((buf[:, width:].contiguous().view(torch.int32) == PATTERN).all())


def _raw(t, arena, pad, pre_w=None, pre_b=None, twice=False):
    """FWD, DX of every source, DW through sr_linear_fwd / _bwd_input / _bwd_weight with every leading dimension ``pad`` wider than its
    matrix (``pad``: dict ldy_out, ldg, ldy, ldd) -> the outputs (CPU) after asserting that no padding column was written."""
    from satnerf_amd import _lib, ops

    srcs = dev_srcs(t.srcs)
    arr = ops._linear_srcs(srcs, t.p)
    w, b = dev(t.w), dev(t.b)
    oa = ops.OUT_ACTS[t.oa]
    ktot = t.w.shape[1]
    y = arena.alloc(t.p, t.n_out + pad["ldy_out"])
    _lib.call("sr_linear_fwd", arr, len(srcs), ops._p(w), ops._p(b), t.p, t.n_out, oa, ops._p(y), y.shape[1], ops._stream())
    assert _untouched(y, t.n_out), "forward wrote into the padding of y"
    y_cpu = y[:, :t.n_out].cpu()
    gy = _padded(arena, t.gy, t.n_out + pad["ldg"])
    yin = _padded(arena, y_cpu, t.n_out + pad["ldy"]) if t.oa is not None else None
    ldy = 0 if yin is None else yin.shape[1]
    out = {"y": y_cpu, "dx": []}
    for (x, act, w0, div), col0 in zip(srcs, t.col0):
        if act is not None and div != 1:
            continue
        k = x.shape[1]
        d = arena.alloc(t.p, k + pad["ldd"])
        tgt = ops._linear_srcs([(x, act, w0, div)], t.p)
        _lib.call("sr_linear_bwd_input", ops._p(gy), gy.shape[1], ops._p(yin), ldy, oa, ops._p(w), ktot, col0, tgt, t.p, t.n_out, ops._p(d),
                  d.shape[1], ops._stream())
        assert _untouched(d, k), "DX wrote into the padding of d_src"
        out["dx"].append(d[:, :k].cpu())
    gw, gb = arena.alloc(t.n_out, ktot), arena.alloc(t.n_out)
    gw.copy_(pre_w.to(DEV)) if pre_w is not None else gw.zero_()
    gb.copy_(pre_b.to(DEV)) if pre_b is not None else gb.zero_()
    for _ in range(2 if twice else 1):
        _lib.call("sr_linear_bwd_weight", ops._p(gy), gy.shape[1], ops._p(yin), ldy, oa, arr, len(srcs), t.p, t.n_out, ops._p(gw), ops._p(gb),
                  ops._stream())
        out.setdefault("dw_first", (gw.cpu(), gb.cpu()))
    out["dw"] = (gw.cpu(), gb.cpu())
    torch.cuda.synchronize()
    assert arena.intact()
    return out


RAW = [L.case(129, 129, L.SKIP), L.case(1025, 136, (L.S(3), L.S(64, "sin", 30.0)), "softplus"),
       L.case(129, 5, (L.S(33, "relu", 1.0),), "sigmoid_rgb", deep=True), L.case(129, 136, (L.S(35, "sin", 1.7, lay="off1"),), "softplus")]


@pytest.mark.parametrize("c", RAW, ids=L.case_id)
@pytest.mark.parametrize("pad", [dict(ldy_out=5, ldg=3, ldy=7, ldd=1), dict(ldy_out=128, ldg=4, ldy=0, ldd=13), dict(ldy_out=0, ldg=0, ldy=0, ldd=0)],
                         ids=["odd", "wide", "dense"])
def test_leading_dimensions_wider_than_the_matrix(c, pad, arena):
    assert L.case_id(c) in IDS
    t = L.build(c)
    got = _raw(t, arena, pad)
    y = got["y"]
    yy = y if t.oa is not None else None
    r = {"fwd": L.ratio(y, *L.fwd(t.srcs, t.w, t.b, t.p, t.oa))}
    live = [(s, c0) for s, c0 in zip(t.srcs, t.col0) if s[1] is None or s[3] == 1]
    for i, ((src, col0), d) in enumerate(zip(live, got["dx"])):
        r[f"dx{i}"] = L.ratio(d, *L.dx(t.gy, yy, t.oa, t.w, col0, src, t.p))
    mw, gate_w, mb, gate_b = L.dw(t.gy, yy, t.oa, t.srcs, t.p, t.n_out)
    r["dw"], r["db"] = L.ratio(got["dw"][0], mw, gate_w), L.ratio(got["dw"][1], mb, gate_b)
    w = L.worst(r)
    for k, v in w.items():
        _record(k, v)
    assert all(v <= 1.0 for v in w.values()), w


@pytest.mark.parametrize("c", [L.case(129, 129, L.SKIP), L.case(2048 + 17, 129, L.SKIP), L.case(1025, 136, (L.S(3), L.S(64, "sin", 30.0)), "softplus")],
                         ids=L.case_id)
def test_dw_adds_to_what_the_buffers_hold(c, arena):
    """DW into a non-zero pre-fill = pre-fill + gradient; DW twice into the same buffers = the first result + the gradient."""
    t = L.build(c)
    g = torch.Generator().manual_seed(5)
    pw, pb = torch.randn(t.n_out, t.w.shape[1], generator=g), torch.randn(t.n_out, generator=g)
    pad = dict(ldy_out=0, ldg=0, ldy=0, ldd=0)
    got = _raw(t, arena, pad, pw, pb)
    yy = got["y"] if t.oa is not None else None
    mw, gate_w, mb, gate_b = L.dw(t.gy, yy, t.oa, t.srcs, t.p, t.n_out, True, pw, pb)
    w = {"dw": float(L.ratio(got["dw"][0], mw, gate_w).max()), "db": float(L.ratio(got["dw"][1], mb, gate_b).max())}
    got = _raw(t, arena, pad, twice=True)
    first_w, first_b = got["dw_first"]
    mw, gate_w, mb, gate_b = L.dw(t.gy, yy, t.oa, t.srcs, t.p, t.n_out, True, first_w, first_b)
    w["dw"] = max(w["dw"], float(L.ratio(got["dw"][0], mw, gate_w).max()))
    w["db"] = max(w["db"], float(L.ratio(got["dw"][1], mb, gate_b).max()))
    fresh = L.dw(t.gy, yy, t.oa, t.srcs, t.p, t.n_out)
    assert float(L.ratio(first_w, fresh[0], fresh[1]).max()) <= 1.0 and float(L.ratio(first_b, fresh[2], fresh[3]).max()) <= 1.0
    for k, v in w.items():
        _record(k, v)
    assert all(v <= 1.0 for v in w.values()), w


def test_no_bias_gradient_leaves_none_and_null_bias_adds_nothing(arena):
    from satnerf_amd import ops

    t = L.build(L.case(129, 35, L.SKIP, "sigmoid", bias=False))
    assert t.b is None
    y = ops.linear_fwd(dev_srcs(t.srcs), dev(t.w), None, t.p, t.oa)
    z = ops.linear_fwd(dev_srcs(t.srcs), dev(t.w), torch.zeros(t.n_out, device=DEV), t.p, t.oa)
    assert torch.equal(y.view(torch.int32), z.view(torch.int32))
    gw, gb = ops.linear_bwd_weight(dev(t.gy), y, t.oa, dev_srcs(t.srcs), t.p, t.n_out, want_bias=False)
    assert gb is None
    gw2, gb2 = ops.linear_bwd_weight(dev(t.gy), y, t.oa, dev_srcs(t.srcs), t.p, t.n_out, want_bias=True)
    assert torch.equal(gw.view(torch.int32), gw2.view(torch.int32)) and gb2 is not None


# ---------------------------------------------------------------------------------------------------- fault check on the device
def test_one_changed_element_leaves_the_gate_where_it_is_read(arena):
    """A weight (FWD) / a gy element (DW) changed by a relative 2^-10 against the reference of the unchanged data: outside the gate in
    that column / row, inside everywhere else.  Small contractions (K = 3 columns, 2 points), so that one term is a large share of A."""
    be = Dev()
    t = L.build(L.case(129, 3, (L.S(3),)))
    y_ref, gate = L.fwd(t.srcs, t.w, t.b, t.p, t.oa)
    w = t.w.clone()
    w[1, 2] *= 1 + 2.0 ** -10
    r = L.ratio(be.fwd(t.srcs, w, t.b, t.p, t.oa), y_ref, gate)
    assert float(r[:, 1].max()) > 1.0 and float(r[:, [0, 2]].max()) <= 1.0, r.max(0)
    assert float(L.ratio(be.fwd(t.srcs, t.w, t.b, t.p, t.oa), y_ref, gate).max()) <= 1.0
    t = L.build(L.case(2, 3, (L.S(3),)))
    mw, gate_w, mb, gate_b = L.dw(t.gy, None, None, t.srcs, t.p, t.n_out)
    gy = t.gy.clone()
    gy[1, 2] *= 1 + 2.0 ** -10
    gw, gb = be.dw(gy, None, None, t.srcs, t.p, t.n_out)
    rw, rb = L.ratio(gw, mw, gate_w), L.ratio(gb, mb, gate_b)
    assert float(rw[2].max()) > 1.0 and float(rw[:2].max()) <= 1.0, rw
    assert float(rb[2]) > 1.0 and float(rb[:2].max()) <= 1.0, rb
    gw, gb = be.dw(t.gy, None, None, t.srcs, t.p, t.n_out)
    assert float(L.ratio(gw, mw, gate_w).max()) <= 1.0 and float(L.ratio(gb, mb, gate_b).max()) <= 1.0


# ------------------------------------------------------------------------------------------------ the small kernels of the file
@pytest.mark.parametrize("stride,dir_col", [(11, 3), (11, 8), (8, 3)])
@pytest.mark.parametrize("n,s", [(1, 1), (257, 1), (1, 257), (37, 7)])
def test_points_along_bit_for_bit(stride, dir_col, n, s):
    from satnerf_amd import ops

    g = torch.Generator().manual_seed(stride + dir_col + n + s)
    rays = 3 * torch.randn(n, stride, generator=g)
    z = 10 * torch.rand(n, s, generator=g)
    z[0, 0] = 0.0
    rays[0, dir_col] = -0.0
    got = ops.points_along(rays.to(DEV), dir_col, z.to(DEV)).cpu()
    want = L.points_along(rays, dir_col, z)
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("n_freqs", [4, 10])
@pytest.mark.parametrize("rows,strided", [(1, False), (257, False), (257, True), (1, True)])
def test_positional_map_inside_its_gate(n_freqs, rows, strided):
    """dim = 3, |x| up to 6 (arguments up to 3072 radians at 2^9); rows * width = 257 * 60 at n_freqs = 10 (an output has at least two
    columns, so the smallest launch is one row)."""
    from satnerf_amd import ops

    g = torch.Generator().manual_seed(rows + n_freqs)
    base = (12 * torch.rand(rows, 11, generator=g) - 6).float()
    base[0, 8] = 6.0
    x = base[:, 8:11] if strided else base[:, 8:11].contiguous()
    xd = dev(x)
    assert rows == 1 or xd.stride(0) == (11 if strided else 3)
    got = ops.positional_map(xd, n_freqs).cpu()
    want, gate = L.positional_map(x, n_freqs)
    r = L.ratio(got, want, gate)
    _record("positional_map", r.max())
    assert float(r.max()) <= 1.0, (float(r.max()), int(r.argmax()))
