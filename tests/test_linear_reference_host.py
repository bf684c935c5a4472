"""tests/linear_reference.py checked on the CPU, before any kernel is held to it.

1. The formulas are nn.Linear's: in float64 ("exact" mode: nothing rounded) every value equals a float64 restatement of the layer
   (activation on load, concatenation, repeat_interleave for per-ray rows, Linear, output activation) and every gradient torch.autograd's
   through it, on every case the GPU module runs.
2. The float32 emulation of the kernel's arithmetic (linear_reference.Emu: bf16 hi/lo split, three passes, fp32 accumulation per 16-wide
   k-step, colsum's accumulators, the modelled phase, out_act' from y) lies inside every gate on every case.  Worst |error| / gate over
   all cases (a record, nothing is derived from it):   fwd 0.97   dx 0.51   dw 0.39   db 0.03
   (fwd: a sigmoid_rgb output near -0.001 is fl(1.002f s - 0.001f), one rounding of a difference: the gate of one rounding is sharp;
   dw: a single point, one product, 1.3 * 2^-16 of it from the bf16 split against the 3 * 2^-16 allowed)
   and of the plain three-pass product at (M, K, N) = (296, 203, 136), (136, 2065, 203), (129, 3, 64), (64, 35, 1): 0.04, 0.01, 0.39,
   0.05; with the lo*hi pass dropped 17.6, 3.8, 74, 20 times the gate, with the last k masked 1450, 78, 21678, 2807 times.
3. Every planted fault (linear_reference.FAULTS) puts the emulation outside a gate on the case built for it, by 17 times or more
   (the smallest: a dropped lo pass, 17.6 on dW; a dropped split-K chunk or an unmasked row behind one, 93).
4. DW into buffers that hold something: the sum, within the gate; twice into the same buffers: twice the gradient."""
import pytest
import torch

from . import linear_reference as L

IDS = [L.case_id(c) for c in L.CASES]
PIN = 1e-11
_WORST = {}


def test_the_case_matrix_is_the_issues():
    """Every row count, width, contraction length and source pair of the issue's matrix is present, and no two cases share an id."""
    assert len(set(IDS)) == len(IDS)
    assert {c["p"] for c in L.CASES} >= {1, 127, 128, 129, 296, 511, 512, 513, 1023, 1024, 1025, 2065}
    assert {c["n_out"] for c in L.CASES} >= {1, 3, 127, 128, 129, 136}
    single = {c["srcs"][0][0] for c in L.CASES if len(c["srcs"]) == 1}
    assert single >= {1, 3, 31, 32, 33, 35, 130}
    pairs = {(c["srcs"][0][0], c["srcs"][1][0]) for c in L.CASES if len(c["srcs"]) == 2}
    assert pairs >= {(3, 64), (3, 256), (63, 4), (61, 16), (64, 5), (60, 24)}
    assert {s[3] for c in L.CASES for s in c["srcs"]} >= {1, 4, 50}
    assert {s[4] for c in L.CASES for s in c["srcs"]} >= {"dense", "rays", "off1"}
    combos = {(c["srcs"][0][1], c["srcs"][0][2], c["oa"]) for c in L.CASES}
    assert combos >= {(a, w, oa) for a, w in L.ACTS for oa in L.OUT_ACTS}
    assert any(not c["bias"] for c in L.CASES) and any(not c["want_bias"] for c in L.CASES)
    for c in L.CASES:       # per-ray sources: n_points no multiple of row_div, rows to spare
        t = L.build(c)
        for x, _, _, div in t.srcs:
            if div > 1:
                assert c["p"] % div and x.shape[0] * div > c["p"] + div


def _layer64(t, leaves):
    """The layer as torch would run it, float64: leaves = [x0, (x1), w, (b)] with requires_grad."""
    xs = leaves[:len(t.srcs)]
    w = leaves[len(t.srcs)]
    b = leaves[len(t.srcs) + 1] if t.b is not None else None
    cols = []
    for x, (_, act, w0, div) in zip(xs, t.srcs):
        a = torch.sin(w0 * x) if act == "sin" else torch.relu(x) if act == "relu" else x
        cols.append(torch.repeat_interleave(a, div, 0)[:t.p])
    pre = torch.nn.functional.linear(torch.cat(cols, 1), w, b)
    if t.oa is None:
        return pre
    if t.oa == "softplus":
        return torch.nn.functional.softplus(pre)
    return torch.sigmoid(pre) if t.oa == "sigmoid" else torch.sigmoid(pre) * 1.002 - 0.001


def _close(got, want, what):
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert got.shape == want.shape and err <= PIN * max(float(want.abs().max()), 1.0), (what, err)


@pytest.mark.parametrize("c", L.CASES, ids=IDS)
def test_reference_is_autograd_through_a_float64_linear(c):
    t = L.build(c)
    leaves = [s[0].double().clone().requires_grad_(True) for s in t.srcs] + [t.w.double().requires_grad_(True)]
    if t.b is not None:
        leaves.append(t.b.double().requires_grad_(True))
    y = _layer64(t, leaves)
    grads = torch.autograd.grad(y, leaves, t.gy.double())
    srcs = [(x.detach(), a, w0, div) for x, (_, a, w0, div) in zip(leaves, t.srcs)]
    y_ref, _ = L.fwd(srcs, t.w, t.b, t.p, t.oa, mode="exact")
    _close(y_ref, y.detach(), "y")
    yy = y_ref if t.oa is not None else None
    for i, (src, col0) in enumerate(zip(srcs, t.col0)):
        if src[1] is not None and src[3] != 1:
            continue
        d, _ = L.dx(t.gy, yy, t.oa, t.w, col0, src, t.p, mode="exact")
        per_row = torch.zeros_like(grads[i]).index_add_(0, torch.arange(t.p) // src[3], d)      # autograd sums a ray's points
        _close(per_row, grads[i], f"d_src{i}")
    mw, _, mb, _ = L.dw(t.gy, yy, t.oa, srcs, t.p, t.n_out, True, mode="exact")
    _close(mw, grads[len(srcs)], "dW")
    if t.b is not None:
        _close(mb, grads[len(srcs) + 1], "db")


@pytest.mark.parametrize("c", L.CASES, ids=IDS)
def test_emulation_lies_inside_every_gate(c):
    w = L.worst(L.run_case(c, L.Emu()))
    for k, v in w.items():
        _WORST[k] = max(_WORST.get(k, 0.0), v)
    print("worst |err| / gate:", {k: round(v, 3) for k, v in w.items()}, "so far:", {k: round(v, 3) for k, v in _WORST.items()})
    assert all(v <= 1.0 for v in w.values()), w


PLAIN = [(296, 203, 136), (136, 2065, 203), (129, 3, 64), (64, 35, 1)]


@pytest.mark.parametrize("m,k,n", PLAIN)
def test_plain_three_pass_product(m, k, n):
    """The gate is not vacuous: the three-pass product sits well inside, a dropped lo pass or a masked k well outside."""
    g = torch.Generator().manual_seed(m + k + n)
    a, b = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g)
    z = torch.zeros(m, k, dtype=torch.float64), torch.zeros(n, k, dtype=torch.float64)
    want, gate, _ = L.gemm(a.double(), b.double(), *z, 3 * L._ceil(k, 16))
    ok = float(L.ratio(L.gemm_emu(a, b), want, gate).max())
    lo = float(L.ratio(L.gemm_emu(a, b, "drop_lo"), want, gate).max())
    cut = a.clone()
    cut[:, -1] = 0
    masked = float(L.ratio(L.gemm_emu(cut, b), want, gate).max())
    print(f"({m}, {k}, {n}): three passes {ok:.3f}, lo pass dropped {lo:.1f}, last k masked {masked:.1f}")
    assert ok <= 1.0 and lo > 1.0 and masked > 1.0


SKIP129 = L.case(129, 129, L.SKIP)
COLOUR = L.case(129, 3, (L.S(60, "relu"), L.S(24, None, 1.0, 4)), "sigmoid")
FAULT_CASES = {
    "drop_lo": (SKIP129, ("fwd", "dx", "dw")),
    "k_late": (L.case(1025, 129, L.SKIP), ("dw",)),
    "k_early": (L.case(129, 5, (L.S(33, "sin", 1.7),), None, deep=True), ("fwd", "dx", "dw")),
    "src_boundary": (SKIP129, ("fwd", "dw")),
    "no_row_div": (COLOUR, ("fwd", "dw")),
    "no_col0": (SKIP129, ("dx",)),
    "softplus_sigmoid_y": (L.case(129, 5, (L.S(33, "relu", 1.0),), "softplus", deep=True), ("dx", "dw", "db")),
    "no_rgb_pad": (L.case(129, 5, (L.S(33, "relu", 1.0),), "sigmoid_rgb", deep=True), ("fwd",)),
    "drop_chunk": (L.case(1025, 129, L.SKIP), ("dw",)),
    "drop_slab": (L.case(513, 129, L.SKIP), ("db",)),
    "bias_twice": (SKIP129, ("fwd",)),
}


def test_every_fault_has_a_case():
    assert set(FAULT_CASES) | {"dw_overwrite"} == set(L.FAULTS)
    assert all(L.case_id(c) in IDS for c, _ in FAULT_CASES.values())      # the GPU module runs the very cases the faults are shown on


@pytest.mark.parametrize("fault", sorted(FAULT_CASES))
def test_planted_fault_leaves_its_gate(fault):
    c, kinds = FAULT_CASES[fault]
    w = L.worst(L.run_case(c, L.Emu(fault)))
    print(fault, {k: round(v, 2) for k, v in w.items()})
    for k in kinds:
        assert w[k] > 1.0, (fault, k, w)


def _prefilled(c):
    t = L.build(c)
    y = L.Emu().fwd(t.srcs, t.w, t.b, t.p, t.oa) if t.oa is not None else None
    g = torch.Generator().manual_seed(5)
    return t, y, torch.randn(t.n_out, t.w.shape[1], generator=g), torch.randn(t.n_out, generator=g)


@pytest.mark.parametrize("c", [SKIP129, L.case(1025, 129, L.SKIP)], ids=L.case_id)
def test_dw_adds_to_what_the_buffers_hold(c):
    t, y, pw, pb = _prefilled(c)
    mw, gate_w, mb, gate_b = L.dw(t.gy, y, t.oa, t.srcs, t.p, t.n_out, True, pw, pb)
    fresh = L.dw(t.gy, y, t.oa, t.srcs, t.p, t.n_out, True)
    assert torch.equal(mw, fresh[0] + pw.double()) and torch.equal(mb, fresh[2] + pb.double())
    gw, gb = L.Emu().dw(t.gy, y, t.oa, t.srcs, t.p, t.n_out, True, pw, pb)
    assert float(L.ratio(gw, mw, gate_w).max()) <= 1.0 and float(L.ratio(gb, mb, gate_b).max()) <= 1.0
    gw, gb = L.Emu("dw_overwrite").dw(t.gy, y, t.oa, t.srcs, t.p, t.n_out, True, pw, pb)
    assert float(L.ratio(gw, mw, gate_w).max()) > 1.0 and float(L.ratio(gb, mb, gate_b).max()) > 1.0
    # twice into the same buffers: the second call's reference starts from the first call's result
    g1 = L.Emu().dw(t.gy, y, t.oa, t.srcs, t.p, t.n_out, True)
    g2 = L.Emu().dw(t.gy, y, t.oa, t.srcs, t.p, t.n_out, True, *g1)
    mw, gate_w, mb, gate_b = L.dw(t.gy, y, t.oa, t.srcs, t.p, t.n_out, True, *g1)
    assert float(L.ratio(g2[0], mw, gate_w).max()) <= 1.0 and float(L.ratio(g2[1], mb, gate_b).max()) <= 1.0


def test_small_kernels_reference():
    g = torch.Generator().manual_seed(1)
    rays, z = torch.randn(5, 11, generator=g), torch.rand(5, 7, generator=g)
    got = L.points_along(rays, 8, z).double()
    want = (rays[:, None, 0:3].double() + rays[:, None, 8:11].double() * z.double()[..., None]).reshape(-1, 3)
    bound = L.U * (want.abs() + 2 * (rays[:, None, 8:11].double() * z.double()[..., None]).abs().reshape(-1, 3))
    assert got.dtype == torch.float64 and bool(((got - want).abs() <= bound).all())
    x = (12 * torch.rand(257, 3, generator=g) - 6).float()
    for nf in (4, 10):
        v, gate = L.positional_map(x, nf)
        assert v.shape == (257, 2 * nf * 3)
        for f in range(nf):      # Mapping.forward's column order: frequency, then sin | cos, then channel
            arg = 2.0 ** f * x.double()
            assert torch.equal(v[:, 6 * f:6 * f + 3], torch.sin(arg)) and torch.equal(v[:, 6 * f + 3:6 * f + 6], torch.cos(arg))
        assert bool((gate > 0).all()) and bool((gate <= L.EPS_SINF + L.TINY).all())
