"""The weight-gradient kernels against an fp64 contraction of the workspaces they read (tests/wgrad_reference.py).

Workspaces are captured from a real training step (the ``wgrad_partials`` spy of test_hip_emax.py).  Each block's split-K slices are summed
in fp64 and compared, at every position the gradient scatter map reads, with the reference under the kernel's operand model:

    |got - M_b| <= 2^-19 A_b + B_b + 1e-30      A_b = sum_p |dpre[p, r] act[p, c]|,  B_b = bound of the operand-rounding ambiguity

Once operand rounding is modelled (wgrad.hip: bf16 as stored, sin packed to bf16; wgrad8.hip: bf16 fragments, MX8 exact in bf16; wgrad9.hip:
fp16 with the range fitted per 32-row pair from the table of exponent maxima, lanes below the range flushed), only fp32 accumulation order
is left.  The products are exact in fp32, the sum of one slice is a chain of MFMA accumulations: its rounding error is a sum of one
2^-24 relative error per k-step (two per tile), which for random signs grows like sqrt(k-steps): 2^-19 holds for slices of up to 256
tiles, and the gate grows by sqrt(tiles / 256) beyond (a one-slice-per-block plan of 2048 tiles measured 1.35 x 2^-19 A).  This is a
statistical bound (random rounding directions), not a worst case: the deterministic bound, k-steps x 2^-24 A, is 2^-14 A for a 2048-tile
slice and would not notice a wrong tile.  Data whose rounding errors all point one way could exceed it; training gradients and the
random synthetic workspaces below do not.  Separately, the exact-operand reference R_b is checked at a looser per-format bound (operand rounding itself),
which keeps the operand model honest.

Padding contract: the kernels contract every point of tiles [0, ceil(n_points / 32)) and mask nothing; the dX kernel writes zero pre-
activation gradients for points at and beyond n_points (the last tile's padding).  Both sides are checked when a batch has a partial tile:
the decoded dpre rows are zero there, and the reference sums over points < n_points only.  (A training batch has n_rays x 64 points, so
its last tile is always full; the synthetic workspaces below cover both sides: zero padding summed over points < n_points, random
padding summed over every point of the last tile.)

Offsets past 4 GiB: the 4-wave kernel steps 32-bit per-lane offsets, so workspaces beyond them go to the r02 kernel (wgrad8.hip,
mlp_layout.h wgrad9_fits); test_r02_fallback_past_the_32_bit_bound runs it there.  wgrad.hip (SR_FMT16) needs no such case: every per-tile
address is 64-bit pointer arithmetic (``prm.dpre + tile * kDpFrags * 64`` with a long tile), the per-lane offset handed to the DMA is
below 1 KiB, and the partial-block index is (long)blockIdx.x * kWgBlockFloats."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import satnerf_oracle as O

from . import wgrad_reference as W

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# exact-operand bound per operand rounding: bf16 (8 bits) for wgrad / wgrad8, fp16 (11 bits) + flushed lanes for wgrad9
EXACT_BOUND = {"wgrad": 2.0 ** -8, "wgrad8": 2.0 ** -8, "wgrad9": 2.0 ** -10}
WORST = {}


def capture(mode, feat, tau, n_rays, seed=0, n_samples=64):
    from satnerf_amd import ops
    from satnerf_amd.models import load_model
    from satnerf_amd.train import Trainer

    torch.manual_seed(seed)
    args = O.default_args(mlp_mode=mode, fc_units=feat, t_embbeding_tau=tau, n_samples=n_samples)
    models = {"coarse": load_model(args).to(DEV), "t": torch.nn.Embedding(30, tau).to(DEV)}
    rays, ts = O.synthetic_rays(n_rays, seed=3 + n_rays)
    seen = {}
    real = ops.wgrad_partials

    def spy(feat_, tau_, n_points, dpre, acts, blocks, fmt=16, loads=None, **k):
        partial, plan = real(feat_, tau_, n_points, dpre, acts, blocks, fmt, loads, **k)
        seen.update(dpre=dpre, acts=acts, n=n_points, blocks=blocks, fmt=fmt, loads=loads, partial=partial.clone(), plan=plan.clone())
        return partial, plan

    mp = pytest.MonkeyPatch()
    mp.setattr(ops, "wgrad_partials", spy)
    try:
        tr = Trainer(models, args, use_graph=False, lr=0.0)
        tr._forward_backward(rays.to(DEV), ts.to(DEV), torch.rand(n_rays, 3, device=DEV))
        torch.cuda.synchronize()
    finally:
        mp.undo()
    return seen


def check_partials(feat, tau, ws, partial, plan, kernel, label):
    """Gate every position the scatter map reads; returns the worst |err| / (2^-19 A)."""
    from satnerf_amd import packing

    n, fmt = ws["n"], ws["fmt"]
    n_tiles = (n + 31) // 32
    t = plan.cpu().numpy()
    n_slices = partial.numel() // packing.WG_BLOCK_FLOATS
    work = W.work_of(kernel, t, n_slices, n_tiles)
    assert not W.check_coverage(work, t, n_slices, n_tiles)
    rows, cols, emax = W.decode_workspaces(ws["dpre"], ws["acts"], n, feat, tau, fmt)
    if n % 32:   # padding contract: the dX kernel zeroes the pre-activation gradients of points >= n_points
        for f, op in rows.items():
            assert float(op.exact()[n:].abs().max()) == 0.0, f
    ref = W.reference(feat, tau, rows, cols, n, kernel, work, emax)
    gidx = torch.from_numpy(packing.backward_maps(feat, tau)["gidx"].astype(np.int64)).to(DEV)
    gidx = gidx[gidx >= 0]
    worst = worst_gate = 0.0
    for b, (pos, R, A, M, B) in enumerate(ref):
        S = W.sum_slices(partial, t, b)
        longest = max(t1 - t0 for _, wb, _, t0, t1 in work if wb == b)
        # 2^-19 covers slices of up to 256 tiles (512 fp32 roundings: sqrt(512) 2^-24 = 2^-19.5).  Longer slices (few workgroups: one
        # slice of 2048 tiles at n_wg = 8 measured 1.35 x 2^-19 A) accumulate error like the square root of their length
        scale = max(1.0, (longest / 256) ** 0.5)
        lo, hi = b * packing.WG_BLOCK_FLOATS, (b + 1) * packing.WG_BLOCK_FLOATS
        used = torch.zeros(packing.WG_BLOCK_FLOATS, dtype=torch.bool, device=DEV)
        used[gidx[(gidx >= lo) & (gidx < hi)] - lo] = True
        m = used[pos]
        if not m.any():
            continue
        got = S[pos][m]
        err = (got - M[m]).abs()
        gate = scale * W.GATE * A[m] + B[m] + 1e-30
        bad = err > gate
        assert not bad.any(), (label, kernel, b, int(bad.sum()), float((err / gate).max()), float(got[bad][0]), float(M[m][bad][0]))
        worst = max(worst, float((err / (W.GATE * A[m] + 1e-30)).max()))
        worst_gate = max(worst_gate, float((err / gate).max()))
        exact_err = (got - R[m]).abs()
        assert (exact_err <= EXACT_BOUND[kernel] * A[m] + 1e-6 * float(R.abs().max()) + 1e-30).all(), (label, kernel, b)
    key = (kernel, fmt)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print(f"{label} {kernel} fmt{fmt}: worst |err| / (2^-19 A) = {worst:.3f}, / gate = {worst_gate:.3f}")
    return worst


def check_unpack(feat, tau, partial, plan):
    """sr_unpack_grads: grad[e] (+)= gscale[e] * sum of the slices of partial[gidx[e]], accumulate 0 and 1."""
    from satnerf_amd import _lib, ops, packing

    bm = packing.backward_maps(feat, tau)
    gidx = torch.from_numpy(bm["gidx"]).to(DEV)
    gscale = torch.from_numpy(np.asarray(bm["gscale"], np.float32)).to(DEV)
    t = plan.cpu().numpy()
    k = gidx.long().clamp_min(0)
    blk = k // packing.WG_BLOCK_FLOATS
    ns = torch.from_numpy(t[:, W.SLICES].astype(np.int64)).to(DEV)[blk]
    first = torch.from_numpy(t[:, W.FIRST].astype(np.int64)).to(DEV)[blk]
    off = k - blk * packing.WG_BLOCK_FLOATS
    P = partial.view(-1, packing.WG_BLOCK_FLOATS).to(torch.float64)
    want = torch.zeros_like(off, dtype=torch.float64)
    absum = torch.zeros_like(want)
    for s in range(int(t[:, W.SLICES].max())):
        live = s < ns
        v = P[(first + s).clamp_max(P.shape[0] - 1), off]
        want += torch.where(live, v, torch.zeros_like(v))
        absum += torch.where(live, v.abs(), torch.zeros_like(v))
    want *= gscale.to(torch.float64)
    tol = (2.0 ** -23 * ns.to(torch.float64) * absum + 1e-38) * gscale.abs().to(torch.float64) + 2.0 ** -24 * want.abs()
    mine = gidx >= 0
    for acc in (0, 1):
        base = torch.randn(gidx.numel(), device=DEV)
        grad = base.clone()
        _lib.call("sr_unpack_grads", ops._p(partial), ops._p(gidx), ops._p(gscale), gidx.numel(), ops._p(plan), ops._p(grad), acc, ops._stream())
        torch.cuda.synchronize()
        exp = want + (base.to(torch.float64) if acc else 0.0)
        extra = 2.0 ** -24 * exp.abs() if acc else 0.0
        err = (grad.to(torch.float64) - exp).abs()
        assert (err[mine] <= (tol + extra)[mine]).all(), (acc, float((err - tol - extra)[mine].max()))
        assert torch.equal(grad[~mine], base[~mine])   # entries the fused MLP does not produce are left alone


def check_grad_tail(feat, tau, partial, plan):
    """sr_grad_tail (the reduction of the data-parallel step; sr_grad_tail_adam shares its slice sum): the flat gradient against the fp64
    slice sums times gscale, accumulate 0 and 1.  Its sky-head and embedding parts get a one-ray, one-sample batch of zeros."""
    from satnerf_amd import _lib, ops, packing

    bm = packing.backward_maps(feat, tau)
    gidx = torch.from_numpy(bm["gidx"]).to(DEV)
    gscale = torch.from_numpy(np.asarray(bm["gscale"], np.float32)).to(DEV)
    want, tol = slice_sums(partial, plan, gidx, gscale)
    mine = gidx >= 0
    z = lambda *shape: torch.zeros(*shape, device=DEV)  # noqa: E731
    hidden = 8
    sun, w1, b1, w2, sky, d_sky = z(1, 3), z(hidden, 8), z(hidden), z(8, hidden), z(1, 3), z(1, 3)
    g_w1, g_b1, g_w2, g_b2, d_t, g_emb = z(hidden, 8), z(hidden), z(8, hidden), z(8), z(1, tau), z(30, tau)
    ts = torch.zeros(1, dtype=torch.int64, device=DEV)
    for acc in (0, 1):
        base = torch.randn(gidx.numel(), device=DEV)
        grad = base.clone()
        p = ops._p
        args = _lib.GradTailArgs(partial=p(partial), gidx=p(gidx), gscale=p(gscale), n_params=gidx.numel(), blocks=p(plan), n_blocks=plan.shape[0],
                                 grad=p(grad), accumulate=acc, sun=p(sun), sun_stride=3, n_rays=1, hidden=hidden, w1=p(w1), b1=p(b1), w2=p(w2),
                                 sky=p(sky), d_sky=p(d_sky), g_w1=p(g_w1), g_b1=p(g_b1), g_w2=p(g_w2), g_b2=p(g_b2), d_t=p(d_t), ts=p(ts),
                                 n_samples=1, tau=tau, g_emb=p(g_emb))
        _lib.call("sr_grad_tail", C.byref(args), ops._stream())
        torch.cuda.synchronize()
        exp = want + (base.to(torch.float64) if acc else 0.0)
        extra = 2.0 ** -24 * exp.abs() if acc else 0.0
        err = (grad.to(torch.float64) - exp).abs()
        assert (err[mine] <= (tol + extra)[mine]).all(), ("sr_grad_tail", acc, float((err - tol - extra)[mine].max()))


def slice_sums(partial, plan, gidx, gscale):
    """fp64 gscale[e] * sum of the slices of partial[gidx[e]], and the fp32 summation bound of a kernel that adds them in order."""
    from satnerf_amd import packing

    t = plan.cpu().numpy()
    k = gidx.long().clamp_min(0)
    blk = k // packing.WG_BLOCK_FLOATS
    ns = torch.from_numpy(t[:, W.SLICES].astype(np.int64)).to(DEV)[blk]
    first = torch.from_numpy(t[:, W.FIRST].astype(np.int64)).to(DEV)[blk]
    off = k - blk * packing.WG_BLOCK_FLOATS
    P = partial.view(-1, packing.WG_BLOCK_FLOATS)
    want = torch.zeros_like(off, dtype=torch.float64)
    absum = torch.zeros_like(want)
    for s in range(int(t[:, W.SLICES].max())):
        live = s < ns
        v = P[(first + s).clamp_max(P.shape[0] - 1), off].to(torch.float64)
        want += torch.where(live, v, torch.zeros_like(v))
        absum += torch.where(live, v.abs(), torch.zeros_like(v))
    want *= gscale.to(torch.float64)
    return want, (2.0 ** -23 * ns.to(torch.float64) * absum + 1e-38) * gscale.abs().to(torch.float64) + 2.0 ** -24 * want.abs()


def read_positions(feat, tau, t):
    """Flat indices of every partial-slot element sr_unpack_grads / sr_grad_tail read under the planned table ``t``."""
    from satnerf_amd import packing

    bf = packing.WG_BLOCK_FLOATS
    g = torch.from_numpy(packing.backward_maps(feat, tau)["gidx"].astype(np.int64))
    g = g[g >= 0].unique()
    blk = g // bf
    out = []
    for s in range(int(t[:, W.SLICES].max())):
        live = s < torch.from_numpy(t[:, W.SLICES].astype(np.int64))[blk]
        out.append(((torch.from_numpy(t[:, W.FIRST].astype(np.int64))[blk] + s) * bf + g - blk * bf)[live])
    return torch.cat(out).to(DEV)


CASES = [("bf16", 256, 4, 1), ("bf16", 256, 4, 33), ("bf16", 256, 16, 301), ("bf16", 256, 4, 1024),
         ("bf16", 512, 4, 3), ("bf16", 512, 16, 301), ("bf16", 512, 4, 1024),
         ("bf16x3", 256, 4, 1), ("bf16x3", 256, 16, 33), ("bf16x3", 256, 4, 1024)]


@pytest.mark.parametrize("mode,feat,tau,n_rays", CASES)
def test_captured_step_matches_the_fp64_contraction(mode, feat, tau, n_rays):
    ws = capture(mode, feat, tau, n_rays)
    n_tiles = (ws["n"] + 31) // 32
    kernel = W.kernel_for(ws["fmt"], feat, tau, n_tiles)
    assert (ws["fmt"] == 8) == (mode == "bf16")
    check_partials(feat, tau, ws, ws["partial"], ws["plan"], kernel, f"{mode} w{feat} tau{tau} {n_rays} rays")
    check_unpack(feat, tau, ws["partial"], ws["plan"])
    check_grad_tail(feat, tau, ws["partial"], ws["plan"])


def test_captured_step_with_a_part_filled_last_tile():
    """40 samples per ray, 3 rays: 120 points, the last tile a quarter full -- the dX kernel's side of the padding contract on a real step
    (check_partials asserts zero pre-activation gradients at points >= n_points)."""
    ws = capture("bf16", 256, 4, 3, n_samples=40)
    assert ws["n"] == 120
    check_partials(256, 4, ws, ws["partial"], ws["plan"], "wgrad9", "bf16 w256 tau4 3 rays x 40 samples")


@pytest.mark.parametrize("mode,feat,tau,n_rays", [("bf16", 256, 4, 1024), ("bf16", 512, 16, 301), ("bf16x3", 256, 4, 301)])
def test_every_plan_on_one_workspace(mode, feat, tau, n_rays):
    """One captured workspace, plans for 8 / 64 / 80 / 256 / 304 workgroups: the equal split, the weighted thin split and stream-K on one box.
    Two launches of one plan are bitwise equal (the kernels use no atomics: every slot is written by one workgroup)."""
    from satnerf_amd import ops

    ws = capture(mode, feat, tau, n_rays)
    n_tiles = (ws["n"] + 31) // 32
    kernel = W.kernel_for(ws["fmt"], feat, tau, n_tiles)
    kinds = set()
    for n_wg in (8, 64, 80, 256, 304):
        partial, plan = ops.wgrad_partials(feat, tau, ws["n"], ws["dpre"], ws["acts"], ws["blocks"], ws["fmt"], ws["loads"], n_wg=n_wg)
        p1 = partial.clone()
        partial2, _ = ops.wgrad_partials(feat, tau, ws["n"], ws["dpre"], ws["acts"], ws["blocks"], ws["fmt"], ws["loads"], n_wg=n_wg)
        torch.cuda.synchronize()
        t = plan.cpu().numpy()
        read = read_positions(feat, tau, t)   # what a reduction reads (quadrants nobody reads are never written)
        assert torch.equal(p1[read].view(torch.int32), partial2[read].view(torch.int32)), n_wg
        kinds.add("sk" if t[0, W.SPAN] else "eq" if len(set(t[:, W.SLICES].tolist())) <= 2 else "w")
        check_partials(feat, tau, ws, p1, plan, kernel, f"{mode} w{feat} tau{tau} {n_rays} rays n_wg={n_wg}")
    # the plan kinds sr_wgrad_plan makes here (tests/test_wgrad_reference_host.py checks the planner itself): 8-bit width 256 tau 4 --
    # equal (n_wg 8), stream-K (64), weighted thin (80..304); width 512 tau 16 (two aux fragments: no thin blocks) -- equal, stream-K;
    # 16-bit -- equal only
    want = {("bf16", 256): {"eq", "sk", "w"}, ("bf16", 512): {"eq", "sk"}, ("bf16x3", 256): {"eq"}}[(mode, feat)]
    assert kinds == want, kinds


CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from tests.test_hip_wgrad_reference import capture
ws = capture("bf16", int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
torch.save({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in ws.items()}, sys.argv[2])
"""


@pytest.mark.parametrize("env,feat,tau,n_rays", [({"SATNERF_WGRAD_V1": "1"}, 256, 4, 301), ({"SATNERF_WGRAD_V1": "1"}, 512, 16, 33),
                                                 ({"SATNERF_WGRAD_THIN": "0"}, 256, 4, 301), ({"SATNERF_WGRAD_STREAMK": "1"}, 256, 4, 1024)])
def test_switch_variants_match_the_fp64_contraction(tmp_path, env, feat, tau, n_rays):
    """The r02 kernel (SATNERF_WGRAD_V1=1, read once per process) and the planner / stream switches, each in a child process."""
    path = str(tmp_path / "ws.pt")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", CHILD, ROOT, path, str(feat), str(tau), str(n_rays)],
                       env=dict(os.environ, **env), capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    ws = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in torch.load(path).items()}
    n_tiles = (ws["n"] + 31) // 32
    kernel = W.kernel_for(ws["fmt"], feat, tau, n_tiles, v1=env.get("SATNERF_WGRAD_V1") == "1")
    check_partials(feat, tau, ws, ws["partial"], ws["plan"], kernel, f"{env} w{feat} tau{tau} {n_rays} rays")


def run_synthetic(feat, tau, n_points, D, A, n_wg=0):
    from satnerf_amd import ops, packing

    blocks = torch.from_numpy(packing.backward_maps(feat, tau)["blocks"]).to(DEV)
    loads = torch.from_numpy(packing.wgrad8_loads(feat, tau)).to(DEV)
    partial, plan = ops.wgrad_partials(feat, tau, n_points, D.view(torch.int16), A.view(torch.int16), blocks, 8, loads, n_wg=n_wg)
    torch.cuda.synchronize()
    return partial, plan


# scale groups of dpre: 0..7 trunk layers, 8 feats, 9 rgbh, 10 s1, 11 e1, 12 s2, 13 s3 (mlp_layout.h).  Lanes spread over 24 binades
# inside each group, so a pair's lanes 20+ binades below its maximum flush in the 4-wave kernel.
SPREAD = {g: (b - 24, b) for g, b in enumerate([110, 80, 66, 110, 80, 66, 110, 80, 66, 112, 78, 68, 110, 72])}   # neighbours 30-44 apart
EDGES = {
    "spread": dict(group_e=SPREAD),
    "raw_limits": dict(group_e={g: (90, 100) for g in range(14)}, raw_e=(1, 242)),       # bf16 rows from 2^-126 to 2^115: fp16 subnormals
    "zero_groups": dict(group_e={**{g: (90, 100) for g in range(14)}, 5: (6, 7)}, zero_groups=(3, 9, 13)),   # E = 6 groups, E = 6 / 7 lanes
    "pad_zero": dict(group_e=SPREAD, pad_zero=True),
    "pad_random": dict(group_e=SPREAD, pad_zero=False),
}


@pytest.mark.parametrize("edge", sorted(EDGES))
@pytest.mark.parametrize("feat,tau,n_points", [(256, 4, 32 * 97 + 5), (512, 16, 32 * 61 + 19)])
def test_synthetic_workspaces_at_the_edges(edge, feat, tau, n_points):
    """Workspaces built on the host (wgrad_reference.synthetic_fmt8, exponent table by the restatement of test_hip_emax.py): row pairs of one
    block 30-44 binades apart, RAW16 rows across the bf16 range (fp16 subnormals after the range fit), all-zero scale groups (E = 6) and E = 6 / 7
    lanes, a part-filled last tile.  The 4-wave kernel at the default plan and at an equal split of 8 workgroups.

    Padding: with zero padding (the dX kernel's side of the contract) the reference sums points < n_points; with random padding it has to
    sum every point of the last tile -- the weight-gradient kernels mask nothing."""
    spec = dict(EDGES[edge])
    pad_zero = spec.pop("pad_zero", True)
    gen = torch.Generator(device=DEV).manual_seed(100 * sorted(EDGES).index(edge) + feat)
    D, A = W.synthetic_fmt8(feat, tau, n_points, DEV, gen, pad_zero=pad_zero, **spec)
    n_tiles = (n_points + 31) // 32
    ws = dict(dpre=D, acts=A, n=n_points if pad_zero else 32 * n_tiles, fmt=8)
    for n_wg in (0, 8):
        partial, plan = run_synthetic(feat, tau, n_points, D, A, n_wg)
        check_partials(feat, tau, ws, partial, plan, "wgrad9", f"synthetic {edge} w{feat} tau{tau} n_wg={n_wg}")


PAST_BOUND = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from tests.test_hip_wgrad_reference import past_bound_case
past_bound_case()
"""


def past_bound_case():
    """Width 512, tau 4, n_tiles = the first count past the 4-wave kernel's 32-bit offsets (20,972 tiles, 671,097 points; 4.3 + 4.0 GB of
    workspaces): the launcher hands the workspaces to the r02 kernel, under the cost-weighted plan the planner makes there.  Only tiles
    around the 4-GiB byte offset of dpre, the first and the last (part-filled) tiles hold data -- every other tile decodes to
    zero -- so the reference contracts those tiles alone."""
    from satnerf_amd import packing

    feat, tau = 512, 4
    dk, ak = packing.dpre8_units(feat), packing.act8_units(packing.aux_steps(tau), feat)
    n_tiles = (1 << 32) // (dk * 1024) + 1
    n_points = 32 * n_tiles - 7
    assert not W.wgrad9_fits(n_tiles, ak, dk) and W.wgrad9_fits(n_tiles - 1, ak, dk)
    assert W.kernel_for(8, feat, tau, n_tiles) == "wgrad8"
    # the tiles around 4 GiB into dpre (the acts workspace, 186 units per tile, ends just short of 4 GiB: its last tiles instead)
    td = (1 << 32) // (dk * 1024)
    live = sorted({t for t in (0, 1, td - 1, td, td + 1, n_tiles - 3, n_tiles - 2, n_tiles - 1) if t < n_tiles})
    gen = torch.Generator(device=DEV).manual_seed(5)
    D, A = W.synthetic_fmt8(feat, tau, n_points, DEV, gen, group_e=SPREAD, live_tiles=live)
    partial, plan = run_synthetic(feat, tau, n_points, D, A)
    t = plan.cpu().numpy()
    assert int(t[0, W.SPAN]) == 0 and len(set(t[:, W.SLICES].tolist())) > 2   # the weighted thin split (run as full blocks)
    n_slices = partial.numel() // packing.WG_BLOCK_FLOATS
    assert not W.check_coverage(W.work_of("wgrad8", t, n_slices, n_tiles), t, n_slices, n_tiles)
    Dc, Ac = W.gather_tiles(D, dk, live), W.gather_tiles(A, ak, live)
    del D, A
    n_c = 32 * len(live)   # (the last live tile's padding is zero: summing it adds nothing)
    rows, cols, _ = W.decode_workspaces(Dc, Ac, n_c, feat, tau, 8)
    worst = 0.0
    for b, (pos, R, Ab, M, B) in enumerate(W.reference(feat, tau, rows, cols, n_c, "wgrad8")):
        S = W.sum_slices(partial, t, b)[pos]
        used = torch.zeros(packing.WG_BLOCK_FLOATS, dtype=torch.bool, device=DEV)
        g = torch.from_numpy(packing.backward_maps(feat, tau)["gidx"].astype(np.int64)).to(DEV)
        g = g[(g >= b * packing.WG_BLOCK_FLOATS) & (g < (b + 1) * packing.WG_BLOCK_FLOATS)] - b * packing.WG_BLOCK_FLOATS
        used[g] = True
        m = used[pos]
        err = (S[m] - M[m]).abs()
        gate = W.GATE * Ab[m] + B[m] + 1e-30
        assert (err <= gate).all(), (b, float((err / gate).max()))
        worst = max(worst, float((err / (W.GATE * Ab[m] + 1e-30)).max()))
    print(f"past the 32-bit bound: wgrad8 fmt8 worst |err| / (2^-19 A) = {worst:.3f}")


def test_r02_fallback_past_the_32_bit_bound():
    """The only place the r02 kernel and its weighted thin plan run by default.  In a child process under its own time limit (8.3 GB of
    workspaces)."""
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", PAST_BOUND, ROOT], capture_output=True, text=True, cwd=ROOT)
    print(r.stdout[-500:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
