"""DSM registration on the GPU (csrc/dsm_register.hip through satnerf_amd.dsm): dsmr.compute_shift / dsmr.apply_shift and the
registered DSM MAE against the reference's fixtures (tests/golden/dsmr/) and, on inputs no fixture covers, against the numpy
restatement of tests/test_dsmr_host.py; known shift, determinism, graph capture and errors."""
import numpy as np
import pytest
import torch

from tests.test_dsmr_host import FIXTURES, apply_shift, bits, compute_shift, load, registered_err

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dsm():
    from satnerf_amd import dsm, ops

    return dsm, ops


def _t(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).to(DEV)


def city(rng, h, w, n_boxes):
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    z = 20.0 + 0.05 * ii - 0.03 * jj + 2.0 * np.sin(ii / 23.0) * np.cos(jj / 31.0)
    for _ in range(n_boxes):
        bh, bw = rng.integers(6, 40, size=2)
        y0, x0 = rng.integers(0, h - bh), rng.integers(0, w - bw)
        z[y0:y0 + bh, x0:x0 + bw] += rng.uniform(4.0, 40.0)
    return z


def pair(rng, hu, wu, hv, wv, dx, dy, dz, n_boxes, noise=0.05, pad=60):
    """fp32 u and v with v[j + dy, i + dx] = u[j, i] + dz (+ noise)."""
    f = city(rng, max(hu, hv) + 2 * pad, max(wu, wv) + 2 * pad, n_boxes)
    u = f[pad:pad + hu, pad:pad + wu] + rng.normal(0, noise, (hu, wu))
    v = f[pad - dy:pad - dy + hv, pad - dx:pad - dx + wv] + dz + rng.normal(0, noise, (hv, wv))
    return u.astype(np.float32), v.astype(np.float32)


def gpu_register(u, v, irange=5, scaling=True, scratch=None):
    """(shift (dx, dy), coef (8,), ncc maps (levels, n, n), starts (levels, 2)) on the host."""
    _, ops = _dsm()
    out, ncc, starts = ops.dsm_compute_shift(_t(u, torch.float64), _t(v, torch.float64), irange=irange, scaling=scaling,
                                             scratch=scratch, maps=True)
    host = out.cpu()
    return tuple(host[8:].view(torch.int32).tolist()), host[:8].view(torch.float64).numpy(), ncc.cpu().numpy(), starts.cpu().numpy()


def same_maps(got, want, tol=1e-12):
    """Equal NaN patterns and |got - want| <= tol on the finite entries."""
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    f = ~np.isnan(want)
    return not f.any() or np.abs(got[f] - want[f]).max() <= tol


def check_against_restatement(u, v, irange=5, scaling=True):
    r = compute_shift(u, v, scaling=scaling, irange=irange)
    shift, coef, ncc, starts = gpu_register(u, v, irange, scaling)
    assert ncc.shape[0] == len(r["levels"])
    for k in range(len(r["levels"])):
        assert tuple(starts[k]) == r["start"][k], f"level {k} start"
        assert same_maps(ncc[k], r["ncc"][k]), f"level {k} ncc"
    assert shift == r["shift"]
    want = np.array([r["a"], r["b"], *r["stats"][1:6], r["stats"][0]])
    f = np.isfinite(want)
    assert np.array_equal(np.isnan(coef), np.isnan(want))
    assert np.all(np.abs(coef[f] - want[f]) <= 1e-12 * np.abs(want[f]))
    return r, shift, coef


def margin_ok(r, need=1e-9):
    """The restatement's winner beats its runner-up by `need` at every level (so equal shifts are a fair gate)."""
    for m in r["ncc"]:
        top = np.sort(m[np.isfinite(m)])[::-1]
        if len(top) > 1 and top[0] - top[1] < need:
            return False
    return True


# ---- against the reference's fixtures --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture(name):
    dsm, ops = _dsm()
    g = load(name)
    levels = int(g["levels"])
    su, sv = _t(g["u"], torch.float64), _t(g["v"], torch.float64)
    for k in range(1, levels):
        su, sv = ops.dsm_downsample2x(su), ops.dsm_downsample2x(sv)
        assert np.array_equal(bits(su.cpu().numpy()), bits(g[f"su{k}"])), f"level {k} u"
        assert np.array_equal(bits(sv.cpu().numpy()), bits(g[f"sv{k}"])), f"level {k} v"
    irange, scaling = int(g["irange"]), bool(g["scaling"])
    shift, coef, ncc, starts = gpu_register(g["u"], g["v"], irange, scaling)
    assert ncc.shape == (levels, 2 * irange + 1, 2 * irange + 1)
    for k in range(levels):
        assert tuple(starts[k]) == tuple(g[f"start{k}"]), f"level {k} start"
        assert np.abs(ncc[k] - g[f"ncc{k}"]).max() <= 1e-12, f"level {k} ncc"
    assert shift == tuple(g["shift"])
    want = g["coef"]  # a, b, mu_u, mu_v, sig_u, sig_v, xcorr
    assert np.all(np.abs(coef[:7] - want) <= 1e-12 * np.abs(want))
    # the public API: same answer, and apply_shift bitwise the reference's at the reference's coefficients
    dx, dy, a, b = dsm.compute_shift(_t(g["u"]), _t(g["v"]), scaling=scaling, irange=irange)
    assert (dx, dy) == shift and a == coef[0] and b == coef[1]
    out = dsm.apply_shift(_t(g["v"]), *(int(s) for s in g["shift"]), float(want[0]), float(want[1]))
    assert out.dtype == torch.float32 and out.is_cuda
    assert np.array_equal(bits(out.cpu().numpy()), bits(g["apply"]))


def test_metric_fixture():
    dsm, _ = _dsm()
    g = load("dsmr_metric")
    pred = g["v"].copy()
    pred[g["mask"] == 9] = 5.0  # dsm_mae must put the water NaNs back itself
    mae, err, rdsm, (dx, dy, a, b) = dsm.dsm_mae(_t(pred), _t(g["u"]), _t(g["mask"], torch.uint8), register="xyz")
    assert (dx, dy) == tuple(g["shift"]) and a == 1.0
    assert err.dtype == torch.float32 and rdsm.dtype == torch.float32
    assert np.array_equal(bits(err.cpu().numpy()), bits(g["err"]))
    assert np.array_equal(bits(rdsm.cpu().numpy()), bits(g["apply"]))
    assert abs(mae - float(g["mae"])) <= 1e-6 * float(g["mae"])


# ---- against the restatement -----------------------------------------------------------------------------------------------------
def test_2048_pair_matches_restatement():
    u, v = pair(np.random.default_rng(11), 2048, 2048, 2048, 2048, 37, -22, 1.5, 3000)
    u[100:140, 300:420] = np.nan
    r, shift, _ = check_against_restatement(u, v, scaling=False)
    assert len(r["levels"]) == 6 and margin_ok(r)
    assert shift == (37, -22)


def test_single_level_pair_matches_restatement():
    u, v = pair(np.random.default_rng(12), 80, 97, 91, 75, -3, 2, 0.4, 20)
    r, shift, _ = check_against_restatement(u, v)
    assert len(r["levels"]) == 1 and margin_ok(r) and shift == (-3, 2)


def test_shifts_without_overlap_are_never_chosen():
    rng = np.random.default_rng(13)
    u = rng.normal(size=(40, 40)).astype(np.float32)
    v = np.full((20, 20), np.nan, np.float32)
    v[:4, :4] = rng.normal(size=(4, 4))  # shifts with dx >= 4 or dy >= 4 pair nothing, dx or dy = 3 one row / column
    r, shift, _ = check_against_restatement(u, v)
    m = r["ncc"][0]
    assert np.isnan(m).any() and np.isfinite(m).any() and np.isfinite(m[shift[1] + 5, shift[0] + 5])


def test_constant_image():
    c = np.full((60, 70), 12.5, np.float32)
    for scaling in (False, True):
        r, shift, coef = check_against_restatement(c, c, scaling=scaling)
        assert np.isnan(r["ncc"][0]).all() and shift == (0, 0)
    assert np.isnan(coef[0])  # scaling: sig_u / sig_v = 0 / 0


@pytest.mark.parametrize("irange", [1, 16])
def test_irange_extremes(irange):
    u, v = pair(np.random.default_rng(14 + irange), 150, 170, 150, 170, 2 * irange, -2 * irange, 0.3, 30)
    r, shift, _ = check_against_restatement(u, v, irange=irange, scaling=False)
    assert len(r["levels"]) == 2 and margin_ok(r) and shift == (2 * irange, -2 * irange)


# ---- behaviour -------------------------------------------------------------------------------------------------------------------
def test_known_shift_recovered():
    dsm, _ = _dsm()
    u, v = pair(np.random.default_rng(15), 512, 512, 512, 512, 13, -11, 0.7, 150, noise=0.0)
    dx, dy, a, b = dsm.compute_shift(_t(u), _t(v), scaling=False)
    assert (dx, dy) == (13, -11) and a == 1.0 and abs(b + 0.7) <= 1e-6
    out = dsm.apply_shift(_t(v), dx, dy, a, b)
    assert torch.nanmean((out - _t(u)).abs()).item() <= 1e-5  # registered back onto u


def test_deterministic_with_garbage_scratch():
    _, ops = _dsm()
    u, v = pair(np.random.default_rng(16), 700, 600, 690, 610, 9, 6, -1.0, 200)
    nbytes, _ = ops.dsm_register_plan(u.shape, v.shape, 5)
    runs = []
    for fill in (0x7F, 0xA5):  # NaN-ish and arbitrary bytes
        scratch = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
        runs.append(gpu_register(u, v, 5, True, scratch=scratch))
    (s0, c0, n0, t0), (s1, c1, n1, t1) = runs
    assert s0 == s1 and np.array_equal(bits(c0), bits(c1)) and np.array_equal(bits(n0), bits(n1)) and np.array_equal(t0, t1)


def test_graph_capture_replays_on_new_inputs():
    _, ops = _dsm()
    rng = np.random.default_rng(17)
    u0, v0 = pair(rng, 300, 320, 300, 320, 4, 7, 0.5, 60)
    u1, v1 = pair(rng, 300, 320, 300, 320, -12, 3, -2.0, 60)
    su, sv = _t(u0, torch.float64), _t(v0, torch.float64)
    nbytes, _ = ops.dsm_register_plan(su.shape, sv.shape, 5)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.empty(9, dtype=torch.int64, device=DEV)
    rdsm = torch.empty(sv.shape, dtype=torch.float32, device=DEV)

    def step():
        ops.dsm_compute_shift(su, sv, irange=5, scaling=False, out=out, scratch=scratch)
        ops.dsm_apply_shift(sv, out[8:].view(torch.int32), out[:8].view(torch.float64), out=rdsm)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    su.copy_(_t(u1, torch.float64))
    sv.copy_(_t(v1, torch.float64))
    graph.replay()
    torch.cuda.synchronize()
    got_out, got_rdsm = out.clone(), rdsm.clone()
    step()  # eager on the same (new) inputs
    torch.cuda.synchronize()
    assert torch.equal(got_out, out) and torch.equal(got_rdsm.view(torch.int32), rdsm.view(torch.int32))
    assert got_out[8:].view(torch.int32).tolist() == [-12, 3]


def test_errors():
    dsm, ops = _dsm()
    from satnerf_amd import _lib

    u = torch.zeros(20, 20, device=DEV)
    with pytest.raises(ValueError):
        dsm.compute_shift(torch.zeros(20, 20), u)  # CPU
    with pytest.raises(ValueError):
        dsm.apply_shift(torch.zeros(20, 20))
    with pytest.raises(ValueError):
        dsm.compute_shift(torch.zeros(2, 20, 20, device=DEV), u)  # not 2-D
    for bad in (0, 17, 2.5):
        with pytest.raises(ValueError):
            dsm.compute_shift(u, u, irange=bad)
    with pytest.raises(_lib.SatRenderError):
        ops.dsm_compute_shift(u.double(), u.double(), irange=17)  # the library checks too
    nan = torch.full((30, 30), float("nan"), device=DEV)
    with pytest.raises(ValueError):
        dsm.compute_shift(nan, nan)
    with pytest.raises(ValueError):
        dsm.dsm_mae(nan, nan, register="xyz")
    with pytest.raises(ValueError):
        dsm.dsm_mae(u, u, register="xy")


def test_register_z_is_unchanged():
    """register="z" (and the default) is the Z-only MAE dsm_mae has always computed, bit for bit."""
    dsm, _ = _dsm()
    rng = np.random.default_rng(18)
    gt, pred = pair(rng, 64, 72, 64, 72, 0, 0, 0.8, 10)
    pred[3:9, 5:20] = np.nan
    mask = np.zeros(gt.shape, np.uint8)
    mask[40:50, 10:30] = 9
    g, p, m = _t(gt), _t(pred), _t(mask, torch.uint8)
    q = p.double().clone()
    q[m == 9] = float("nan")
    shift = torch.nanmean(g.double() - q)
    rdsm_w = q + shift
    err_w = rdsm_w - g.double()
    for kw in ({}, {"register": "z"}):
        mae, err, rdsm, s = dsm.dsm_mae(p, g, m, **kw)
        assert s == shift.item() and mae == torch.nanmean(err_w.abs()).item()
        assert torch.equal(err.view(torch.int64), err_w.view(torch.int64)) and torch.equal(rdsm.view(torch.int64), rdsm_w.view(torch.int64))


def test_xyz_equals_restatement_on_unregistered_pred():
    dsm, _ = _dsm()
    gt, pred = pair(np.random.default_rng(19), 240, 260, 240, 260, -6, 8, 2.2, 60)
    mask = np.zeros(gt.shape, np.uint8)
    mask[200:230, 20:90] = 9
    err_w, rdsm_w, r = registered_err(pred, gt, mask)
    mae, err, rdsm, (dx, dy, a, b) = dsm.dsm_mae(_t(pred), _t(gt), _t(mask, torch.uint8), register="xyz")
    assert (dx, dy) == r["shift"] == (-6, 8) and abs(b - r["b"]) <= 1e-12 * abs(r["b"])
    assert np.array_equal(bits(rdsm.cpu().numpy()), bits(apply_shift(np.where(mask == 9, np.nan, pred), dx, dy, a, b)))
    assert np.abs(err.cpu().numpy() - err_w)[np.isfinite(err_w)].max() <= 1e-5
    assert abs(mae - float(np.nanmean(np.abs(err_w.astype(np.float64))))) <= 1e-6 * mae
