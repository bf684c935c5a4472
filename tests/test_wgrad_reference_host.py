"""CPU checks of the weight-gradient reference (tests/wgrad_reference.py) and of the split-K plans.

* The workspace decoder against workspaces built on the host from known logical matrices, by encoders restated from csrc/codec8.h (PHASE8,
  MX8) and the lane layout of csrc/mlp_layout.h -- every PHASE8 code, MX8 exponents at the clamp edges.
* Plan coverage: sr_wgrad_plan (the C planner) against its restatement, and for every plan the workgroup numbering of the kernel that runs
  it (wgrad.hip, wgrad8.hip, wgrad9.hip's equal / weighted / stream-K paths): every (block, tile) covered once, every partial slot a
  reduction sums written once, inside n_slices."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from satnerf_amd import _lib, packing

from . import wgrad_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- encoders (codec8.h)
def phase8_encode(rev):
    """round-to-nearest-even(x * 256) mod 256 of a phase in revolutions (codec8.h phase8_bits)."""
    return (np.round(np.asarray(rev, np.float64) * 256.0).astype(np.int64) & 255).astype(np.uint8)


def mx8_encode(v16):
    """16 values of one lane -> (exponent E, 16 codes u): E = biased exponent of max|v| (1 + 2^-7) clamped to [6, 254], u = RNE(v / 2^(E-133)) + 128."""
    v16 = np.asarray(v16, np.float32)
    m = np.float32(np.abs(v16).max())
    m = np.float32(m * np.float32(0.0078125) + m)
    e = int(np.frexp(np.float64(m))[1] + 126) if m > 0 else 0
    e = min(max(e, 6), 254)
    u = np.round(v16.astype(np.float64) * 2.0 ** (133 - e)).astype(np.int64) + 128
    assert (u >= 1).all() and (u <= 255).all()
    return e, u.astype(np.uint8)


def bf16_bits(x):
    b = np.asarray(x, np.float32).view(np.uint32)
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)   # RNE


def put_bf16_fragment(unit, frag):
    """frag [32 points, 16 slots] -> unit bytes [64, 16]: lane (p, h), element j = slot 8 h + j."""
    bits = bf16_bits(frag)
    for lane in range(64):
        p, h = lane & 31, lane >> 5
        unit[lane] = bits[p, 8 * h:8 * h + 8].view(np.uint8)


def put_df(unit, codes):
    """codes [2 halves, 32 points, 16 slots] -> unit bytes: byte n of lane (p, h) = half n >> 3, slot 8 h + (n & 7)."""
    for lane in range(64):
        p, h = lane & 31, lane >> 5
        for n in range(16):
            unit[lane, n] = codes[n >> 3, p, 8 * h + (n & 7)]


@pytest.mark.parametrize("feat,tau", [(256, 4), (256, 16), (512, 4), (512, 16)])
def test_fmt8_decoder_reads_known_matrices(feat, tau):
    rng = np.random.default_rng(feat + tau)
    auxs = packing.aux_steps(tau)
    g8 = packing.fmt8_geometry(feat)
    dk, ak = packing.dpre8_units(feat), packing.act8_units(auxs, feat)
    n_tiles, n_points = 3, 3 * 32 - 5
    D = np.zeros((W.ws_tiles(n_points) * dk * 1024 + 1024,), np.uint8)
    A = np.zeros((W.ws_tiles(n_points) * ak * 1024,), np.uint8)
    Du, Au = D[:W.ws_tiles(n_points) * dk * 1024].reshape(-1, dk, 64, 16), A.reshape(-1, ak, 64, 16)
    want_rows, want_cols = {}, {}
    bm = packing.backward_maps(feat, tau)
    rows = sorted({f for r in bm["block_rows"] for f in r})
    cols = sorted({c for r in bm["block_cols"] for c in r})
    # every PHASE8 code appears (256 codes over the points of the first column fragments); MX8 lanes at E = 6, 7, 253, 254 and in between
    edge_e = [6, 7, 100, 253, 254]
    for t in range(n_tiles):
        for ws, frags, src_of, want in ((Du, rows, lambda f: packing.dpre8_source(f, feat), want_rows),
                                        (Au, cols, lambda f: packing.act8_source(f, auxs, feat), want_cols)):
            for f in frags:
                s = src_of(f)
                if s["codec"] == packing.RAW16:
                    v = rng.standard_normal((32, 16)).astype(np.float32) * 2.0 ** rng.integers(-40, 40)
                    put_bf16_fragment(ws[t, s["unit"]], v)
                    want.setdefault(f, []).append(np.frombuffer(bf16_bits(v).astype(np.uint32) << 16, np.float32).reshape(32, 16))
                    continue
                if s["half"] == 1:
                    continue   # written with its even partner
                if s["codec"] == packing.PHASE8:
                    rev = (np.arange(2 * 32 * 16).reshape(2, 32, 16) + 37 * t + f) % 256 / 256.0 + rng.integers(-3, 3, (2, 32, 16))
                    codes = phase8_encode(rev)
                    put_df(ws[t, s["unit"]], codes)
                    for h in range(2):
                        want.setdefault(f + h, []).append(np.sin(2 * np.pi * codes[h] / 256.0))
                    continue
                vals = np.zeros((2, 32, 16))
                codes = np.zeros((2, 32, 16), np.uint8)
                for lane in range(64):
                    p, h = lane & 31, lane >> 5
                    e_t = edge_e[(lane + f + t) % len(edge_e)]
                    v = rng.uniform(-1, 1, 16) * 2.0 ** (e_t - 127)
                    v[rng.integers(16)] = 2.0 ** (e_t - 127) * 1.5 * (1 if lane & 1 else -1)   # a maximum that lands on E = e_t
                    e, u = mx8_encode(v)
                    assert e == min(max(e_t, 6), 254) or e_t < 7
                    ws[t, s["scale_unit"], lane, s["scale_byte"]] = e
                    for n in range(16):
                        codes[n >> 3, p, 8 * h + (n & 7)] = u[n]
                        vals[n >> 3, p, 8 * h + (n & 7)] = (int(u[n]) - 128) * 2.0 ** (e - 133)
                put_df(ws[t, s["unit"]], codes)
                for h in range(2):
                    want.setdefault(f + h, []).append(vals[h])
        for a in range(auxs):
            v = rng.standard_normal((32, 16)).astype(np.float32)
            put_bf16_fragment(Au[t, a], v)
            want_cols.setdefault(("aux", a), []).append(np.frombuffer(bf16_bits(v).astype(np.uint32) << 16, np.float32).reshape(32, 16))
    got_rows, got_cols, emax = W.decode_workspaces(torch.from_numpy(D), torch.from_numpy(A), n_points, feat, tau, 8)
    assert emax is not None and emax.shape == ((n_tiles + 3) // 4, 16)
    for want, got in ((want_rows, got_rows), (want_cols, got_cols)):
        assert set(want) <= set(got)
        for f, parts in want.items():
            w = np.concatenate(parts).astype(np.float64)
            np.testing.assert_array_equal(got[f].exact().numpy(), w, err_msg=str(f))
    # every PHASE8 code of [0, 256) was used, every MX8 edge exponent met
    codes = torch.cat([o.u.flatten() for o in got_cols.values() if o.codec == "ph8"])
    assert set(codes.tolist()) == set(range(256))
    es = torch.cat([o.e.flatten() for o in got_rows.values() if o.codec == "mx"])
    assert {6, 7, 253, 254} <= set(es.tolist())


@pytest.mark.parametrize("tau", [4, 16])
def test_fmt16_decoder_reads_known_matrices(tau):
    rng = np.random.default_rng(tau)
    feat = 256
    auxs = packing.aux_steps(tau)
    dk, ak = 186, auxs + 184   # mlp_layout.h kDpFrags, act_ksteps(auxs)
    n_points = 64
    D, A = np.zeros((2, dk, 64, 16), np.uint8), np.zeros((2, ak, 64, 16), np.uint8)
    bm = packing.backward_maps(feat, tau)
    kind = {c: int(bm["blocks"][b, 8]) for b, cs in enumerate(bm["block_cols"]) for c in cs}
    want = {}
    for t in range(2):
        for f in sorted({f for r in bm["block_rows"] for f in r}):
            v = rng.standard_normal((32, 16)).astype(np.float32)
            put_bf16_fragment(D[t, f], v)
            want.setdefault(("r", f), []).append(np.frombuffer(bf16_bits(v).astype(np.uint32) << 16, np.float32).reshape(32, 16))
        for c in sorted(kind):
            if kind[c] == W.KIND_PHASE:   # unorm16 phase: sin(2 pi u / 65535)
                u = rng.integers(0, 65536, (32, 16)).astype(np.uint16)
                for lane in range(64):
                    p, h = lane & 31, lane >> 5
                    A[t, c, lane] = u[p, 8 * h:8 * h + 8].view(np.uint8)
                want.setdefault(("c", c), []).append(np.sin(2 * np.pi * u / 65535.0))
            else:
                v = rng.standard_normal((32, 16)).astype(np.float32)
                put_bf16_fragment(A[t, c], v)
                want.setdefault(("c", c), []).append(np.frombuffer(bf16_bits(v).astype(np.uint32) << 16, np.float32).reshape(32, 16))
    rows, cols, _ = W.decode_workspaces(torch.from_numpy(D.reshape(-1)), torch.from_numpy(A.reshape(-1)), n_points, feat, tau, 16)
    for (side, f), parts in want.items():
        got = (rows if side == "r" else cols)[f].exact().numpy()
        np.testing.assert_allclose(got, np.concatenate(parts), rtol=0, atol=1e-15, err_msg=str(f))


def test_reference_contraction_and_operand_models_on_a_small_case():
    """R_b is the fp64 contraction of the decoded fragments at the positions the scatter map reads; the operand models only ever move a value
    by at most its own rounding (or flush it, wgrad9), and A_b bounds |R_b|."""
    rng = np.random.default_rng(1)
    feat, tau, n_points = 256, 4, 70
    auxs = packing.aux_steps(tau)
    dk, ak = packing.dpre8_units(feat), packing.act8_units(auxs, feat)
    D = rng.integers(0, 256, W.ws_tiles(n_points) * dk * 1024 + 1024, dtype=np.uint8)
    A = rng.integers(0, 256, W.ws_tiles(n_points) * ak * 1024, dtype=np.uint8)
    Du = D[:W.ws_tiles(n_points) * dk * 1024].reshape(-1, dk, 64, 16)
    Au = A.reshape(-1, ak, 64, 16)
    g8 = packing.fmt8_geometry(feat)
    Du[:, g8["D8_SCALE"]:] = rng.integers(96, 112, Du[:, g8["D8_SCALE"]:].shape, dtype=np.uint8)
    Au[:, ak - 1] = rng.integers(118, 130, Au[:, ak - 1].shape, dtype=np.uint8)
    for u in [0, g8["D8_SIGMA"], g8["D8_HEAD"]]:
        if u:
            Du[:, u] = (bf16_bits(rng.standard_normal((Du.shape[0], 64, 8)) * 1e-5).view(np.uint8)).reshape(Du.shape[0], 64, 16)
    Au[:, 0] = bf16_bits(rng.standard_normal((Au.shape[0], 64, 8))).view(np.uint8).reshape(Au.shape[0], 64, 16)
    rows, cols, emax = W.decode_workspaces(torch.from_numpy(D), torch.from_numpy(A), n_points, feat, tau, 8)
    ref = W.reference(feat, tau, rows, cols, n_points)
    b = 2
    rf, cf = W.block_operands(feat, tau, b)
    pos, R, Ab, M, B = ref[b]
    x = rows[rf[3]].exact()[:n_points, 5]
    y = cols[cf[1]].exact()[:n_points, 7]
    assert float((x * y).sum()) == pytest.approx(float(R[16 * 3 + 5, 16 + 7]), rel=1e-12)
    assert int(pos[16 * 3 + 5, 16 + 7]) == (16 * 3 + 5) * 256 + 16 + 7
    assert (R.abs() <= Ab * (1 + 1e-12)).all()
    for kernel in ("wgrad8",):
        _, R8, A8, M8, B8 = W.reference(feat, tau, rows, cols, n_points, kernel)[b]
        assert ((M8 - R8).abs() <= 2.0 ** -7 * A8 + B8).all()


# ---------------------------------------------------------------------------------------------------------------- plan coverage
@pytest.fixture(scope="module")
def handle():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.lib()


def c_plan(handle, blocks, n_points, n_wg, fmt):
    t = np.ascontiguousarray(np.array(blocks, np.int32).copy())
    n = ctypes.c_int(0)
    assert handle.sr_wgrad_plan(t.ctypes.data_as(ctypes.c_void_p), t.shape[0], n_points, n_wg, fmt, ctypes.byref(n)) == 0
    return t, n.value


FITS_TILES = (1 << 32) // (W.PLAN_UNITS * 1024)   # the last tile count the planner's bound accepts
POINTS = [1, 31, 32, 33, 127, 128, 129, 4095, 65536, 1 << 22, 32 * FITS_TILES, 32 * FITS_TILES + 1]
N_WG = [1, 8, 64, 80, 256, 304]


def _check_grid(handle, env, v1=False, points=POINTS):
    seen = set()
    for feat in (256, 512):
        for tau in (4, 8, 16):
            blocks = packing.backward_maps(feat, tau)["blocks"]
            for fmt in (8, 16):
                for n_points in points:
                    n_tiles = (n_points + 31) // 32
                    for n_wg in N_WG:
                        t, ns = c_plan(handle, blocks, n_points, n_wg, fmt)
                        want, ns_want = W.plan(blocks, n_points, n_wg, fmt, env, v1=v1)
                        case = (feat, tau, fmt, n_points, n_wg)
                        assert ns == ns_want and (t == want).all(), (case, np.argwhere(t != want)[:5])
                        # the plan's own contract: 1 <= slices <= tiles per block, at most one round of workgroups (stream-K: one per span
                        # plus the block boundaries it crosses), the r02 kernel never gets a stream-K plan
                        assert (t[:, W.SLICES] >= 1).all() and (t[:, W.SLICES] <= n_tiles).all(), case
                        kernel = W.kernel_for(fmt, feat, tau, n_tiles, v1)
                        span = int(t[0, W.SPAN])
                        assert ns <= max(n_wg, len(blocks)) + (len(blocks) - 1 if span else 0), case
                        assert span == 0 or kernel == "wgrad9", case
                        work = W.work_of(kernel, t, ns, n_tiles)
                        bad = W.check_coverage(work, t, ns, n_tiles)
                        assert not bad, (case, kernel, bad[:5])
                        seen.add((kernel, "sk" if span else "eq" if len(set(t[:, W.SLICES].tolist())) <= 2 else "w"))
    return seen


def test_plans_cover_every_tile_once_default(handle, monkeypatch):
    for k in ("SATNERF_WGRAD_STREAMK", "SATNERF_WGRAD_THIN", "SATNERF_WGRAD_THIN_COST"):
        monkeypatch.delenv(k, raising=False)
    seen = _check_grid(handle, {})
    # the grid reaches every kernel and every kind of plan the default build makes
    assert {("wgrad", "eq"), ("wgrad8", "eq"), ("wgrad9", "eq"), ("wgrad9", "sk"), ("wgrad9", "w")} <= seen, seen


@pytest.mark.parametrize("env", [{"SATNERF_WGRAD_STREAMK": "0"}, {"SATNERF_WGRAD_STREAMK": "1"}, {"SATNERF_WGRAD_THIN": "0"}])
def test_plans_cover_every_tile_once_with_switches(handle, monkeypatch, env):
    """The planner reads these switches on every call (wgrad.hip), so they are set in this process."""
    for k in ("SATNERF_WGRAD_STREAMK", "SATNERF_WGRAD_THIN", "SATNERF_WGRAD_THIN_COST"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check_grid(handle, env, points=[1, 33, 129, 4095, 65536, 32 * FITS_TILES + 1])


CHILD_V1 = r"""
import ctypes, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from satnerf_amd import _lib, packing
lib = _lib.lib()
out = []
for feat, tau, n_points, n_wg in json.loads(sys.argv[2]):
    t = np.ascontiguousarray(packing.backward_maps(feat, tau)["blocks"].copy())
    n = ctypes.c_int(0)
    assert lib.sr_wgrad_plan(t.ctypes.data_as(ctypes.c_void_p), t.shape[0], n_points, n_wg, 8, ctypes.byref(n)) == 0
    out.append([t.tolist(), n.value])
print(json.dumps(out))
"""


def test_plans_cover_every_tile_once_v1(handle):
    """SATNERF_WGRAD_V1=1 is read once per process (wgrad8.hip wgrad_v1): the planner runs in a child with the switch set."""
    cases = [[feat, tau, n, w] for feat in (256, 512) for tau in (4, 16) for n in (1, 33, 4095, 65536, 1 << 22) for w in N_WG]
    r = subprocess.run([sys.executable, "-c", CHILD_V1, ROOT, json.dumps(cases)], env=dict(os.environ, SATNERF_WGRAD_V1="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    for (feat, tau, n_points, n_wg), (t, ns) in zip(cases, json.loads(r.stdout.strip().splitlines()[-1])):
        t = np.array(t, np.int32)
        want, ns_want = W.plan(packing.backward_maps(feat, tau)["blocks"], n_points, n_wg, 8, {}, v1=True)
        assert ns == ns_want and (t == want).all(), (feat, tau, n_points, n_wg)
        assert int(t[0, W.SPAN]) == 0
        n_tiles = (n_points + 31) // 32
        assert not W.check_coverage(W.work_of("wgrad8", t, ns, n_tiles), t, ns, n_tiles)


def test_coverage_check_catches_a_dropped_tile_and_a_shared_slot():
    """The coverage check itself: a slice one tile short, and two workgroups writing one slot, are reported."""
    blocks = packing.backward_maps(256, 4)["blocks"]
    t, ns = W.plan(blocks, 4095, 64, 8)
    n_tiles = (4095 + 31) // 32
    work = W.work_of("wgrad9", t, ns, n_tiles)
    assert not W.check_coverage(work, t, ns, n_tiles)
    wg, b, slot, t0, t1 = work[5]
    assert W.check_coverage(work[:5] + [(wg, b, slot, t0, t1 - 1)] + work[6:], t, ns, n_tiles)
    assert W.check_coverage(work[:5] + [(wg, b, work[4][2], t0, t1)] + work[6:], t, ns, n_tiles)
