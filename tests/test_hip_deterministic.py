"""Deterministic training steps: the sky head's and the embedding rows' gradients summed in a fixed order (the ``*_det`` launches) instead
of landing as float atomics.  Kernel level: the ordered reduction bit for bit against its host emulation (tests/late_grads_reference.py),
the sums against an fp64 evaluation, repeated launches byte for byte.  Tail level: the two tail launches on a recorded step's arguments.
Trainer level: two trainers from the same seed end with the same bits."""
import contextlib
import math

import numpy as np
import pytest
import torch

from oracle import satnerf_oracle as O

from . import late_grads_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEP_SWITCHES = ("SATNERF_TAIL_ADAM", "SATNERF_TAIL_PACK", "SATNERF_DP_PACK", "SATNERF_GATHER_IN_FWD", "SATNERF_TRAIN_FUSED", "SATNERF_FWD_V1",
                 "SATNERF_GRAPH_SAMPLER", "SATNERF_GRAPH_ALLREDUCE", "SATNERF_FORCE_ALLREDUCE")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool((a == b).all())


@pytest.fixture(scope="module")
def traffic():
    """64 MB of unrelated copies: odd launches run behind one (dirty lines in every L2), as the stress test of the fused tail does."""
    src = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)
    return src, torch.empty_like(src)


# ---- kernel level ------------------------------------------------------------------------------------------------------------------------
def sky_inputs(n, hidden, seed):
    """Inputs of the sky head's backward whose hidden pre-activations all have |h| >= 1e-4 in fp64 (b1 is shifted until they do): the ReLU mask
    is then the same in every arithmetic."""
    g = torch.Generator().manual_seed(seed)
    sun = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    w1 = (torch.rand(hidden, 3, generator=g) * 2 - 1) / math.sqrt(3.0)
    b1 = (torch.rand(hidden, generator=g) * 2 - 1) * 0.5
    w2 = (torch.rand(3, hidden, generator=g) * 2 - 1) / math.sqrt(hidden)
    b2 = (torch.rand(3, generator=g) * 2 - 1) * 0.1
    for _ in range(1000):
        close = (R.hidden_preacts_fp64(sun, w1, b1).abs() < 1e-4).any(0)
        if not close.any():
            break
        b1[close] += 3.1e-4
    h = R.hidden_preacts_fp64(sun, w1, b1)
    assert float(h.abs().min()) >= 1e-4 and 0 < int((h > 0).sum()) < h.numel()
    sky = torch.sigmoid(torch.relu(h) @ w2.double().t() + b2.double()).float()
    d_sky = torch.randn(n, 3, generator=g)
    return tuple(t.to(DEV).contiguous() for t in (sun, w1, b1, w2, sky, d_sky))


@pytest.mark.parametrize("n", [1, 77, 1024])
@pytest.mark.parametrize("hidden", [128, 256])
def test_sky_bwd_det(traffic, n, hidden):
    from satnerf_amd import ops

    inp = sky_inputs(n, hidden, seed=100 + n + hidden)
    want, terms = R.sky_grads_fp64(*inp)
    bound = R.late_bound(n, terms)
    shapes = ((hidden, 3), (hidden,), (3, hidden), (3,))
    scratch = torch.zeros(R.scratch_words(n, hidden, 0, 0), device=DEV)  # a stand-alone launch's scratch: [counter | sky_part], to the byte
    gen = torch.Generator().manual_seed(7)
    g0 = [torch.randn(*s, generator=gen).to(DEV) for s in shapes]

    def run(fn, start, *extra):
        g = [t.clone() for t in start]
        fn(*inp, *g, *extra)
        return g

    # the reduction phase, bit for bit, on a non-zero gradient
    g = run(ops.sky_bwd_det, g0, scratch)
    torch.cuda.synchronize()
    counter, part, _, _ = R.scratch_views(scratch, n, hidden, 0, 0)
    assert counter == 0 and part.shape == (R.sky_blocks(n), 7 * hidden + 3)
    emu = R.reduce_sky(part, R.join_sky(*[t.cpu().numpy() for t in g0]))
    assert same_bits(R.join_sky(*[t.cpu().numpy() for t in g]), emu)
    # partials and totals against fp64
    zero = [torch.zeros_like(t) for t in g0]
    got = R.join_sky(*[t.cpu().numpy() for t in run(ops.sky_bwd_det, zero, scratch)]).astype(np.float64)
    err, perr = np.abs(got - want), np.abs(part.astype(np.float64).sum(0) - want)
    print(f"sky n={n} hidden={hidden}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f} (partials {float((perr / np.maximum(bound, 1e-300)).max()):.3f})")
    assert (err <= bound).all() and (perr <= bound).all()
    # the atomic twin agrees within twice the bound
    atomic = R.join_sky(*[t.cpu().numpy() for t in run(ops.sky_bwd, zero)]).astype(np.float64)
    assert (np.abs(atomic - got) <= 2 * bound).all()
    # 16 launches, odd ones behind unrelated traffic: identical bytes, partials included
    outs = []
    for k in range(16):
        if k % 2:
            traffic[1].copy_(traffic[0])
        outs.append((torch.cat([t.reshape(-1) for t in run(ops.sky_bwd_det, g0, scratch)]), scratch.clone()))
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(o[0].view(torch.int32), outs[0][0].view(torch.int32)) and torch.equal(o[1].view(torch.int32), outs[0][1].view(torch.int32))
    assert same_bits(outs[0][0].cpu().numpy(), emu)
    # a scratch one word short is refused
    with pytest.raises(ops._lib.SatRenderError, match="scratch"):
        run(ops.sky_bwd_det, g0, scratch[:-1])


@pytest.mark.parametrize("n", [1, 77, 1024])
@pytest.mark.parametrize("tau", [4, 16, 3])
def test_embedding_bwd_det(traffic, n, tau):
    from satnerf_amd import ops

    rows = 30
    gen = torch.Generator().manual_seed(200 + n + tau)
    for s, ts_kind in [(64, "rows"), (50, "rows"), (64, "zero"), (50, "zero")]:
        d_t = torch.randn(n, s, tau, generator=gen).to(DEV)
        if ts_kind == "rows":  # 30 rows, every seventh of them never named
            ts = torch.randint(0, rows, (n,), generator=gen)
            ts = torch.where(ts % 7 == 0, ts + 1, ts)
        else:
            ts = torch.zeros(n, dtype=torch.int64)
        want, terms = R.emb_grads_fp64(d_t, ts, rows)
        bound = R.late_bound(n, terms)
        ts_d = ts.to(DEV)
        scratch = torch.zeros(R.scratch_words(0, 0, n, tau), device=DEV)  # [counter | emb_part | first], to the byte
        g0 = torch.randn(rows, tau, generator=gen).to(DEV)

        def run(fn, start, *extra):
            g = start.clone()
            fn(d_t, ts_d, n, s, tau, g, *extra)
            return g

        g = run(ops.embedding_bwd_det, g0, scratch)
        torch.cuda.synchronize()
        counter, _, part, first = R.scratch_views(scratch, 0, 0, n, tau)
        assert counter == 0 and part.shape == (n, tau) and (first == R.first_of_row(ts)).all()
        emu = R.reduce_emb(part, ts, g0.cpu().numpy())
        assert same_bits(g.cpu().numpy(), emu), (s, ts_kind)
        unused = np.setdiff1d(np.arange(rows), ts.numpy())
        assert unused.size and same_bits(g.cpu().numpy()[unused], g0.cpu().numpy()[unused])  # rows no ray names are not touched
        zero = torch.zeros_like(g0)
        got = run(ops.embedding_bwd_det, zero, scratch).cpu().numpy().astype(np.float64)
        per_ray = d_t.cpu().double().sum(1).numpy()
        # (a ray's sum: at most 16 adds per lane and a 6-level lane tree, fewer than 32 roundings on any path)
        assert (np.abs(part - per_ray) <= 32 * 2.0 ** -24 * d_t.cpu().double().abs().sum(1).numpy()).all()
        err = np.abs(got - want)
        print(f"emb n={n} tau={tau} S={s} ts={ts_kind}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (err <= bound).all()
        atomic = run(ops.embedding_bwd, zero).cpu().numpy().astype(np.float64)
        assert (np.abs(atomic - got) <= 2 * bound).all()
        outs = []
        for k in range(16):
            if k % 2:
                traffic[1].copy_(traffic[0])
            outs.append((run(ops.embedding_bwd_det, g0, scratch), scratch.clone()))
        torch.cuda.synchronize()
        for o in outs:
            assert torch.equal(o[0].view(torch.int32), outs[0][0].view(torch.int32)) and torch.equal(o[1].view(torch.int32), outs[0][1].view(torch.int32))
        assert same_bits(outs[0][0].cpu().numpy(), emu)
    with pytest.raises(ops._lib.SatRenderError, match="scratch"):
        run(ops.embedding_bwd_det, g0, scratch[:-1])


# ---- tail level --------------------------------------------------------------------------------------------------------------------------
def recorded_step(n):
    """The arguments of the tail launch of a real step (the default trainer's third), and that trainer."""
    from satnerf_amd import ops
    from satnerf_amd.models import load_model
    from satnerf_amd.train import Trainer

    torch.manual_seed(0)
    args = O.default_args(mlp_mode="bf16")
    models = {"coarse": load_model(args).to(DEV), "t": torch.nn.Embedding(30, 4).to(DEV)}
    tr = Trainer(models, args, use_graph=True, steps_per_epoch=1000)
    rays, ts = O.synthetic_rays(n, seed=77)
    rays, ts, tgt = rays.to(DEV), ts.to(DEV), torch.rand(n, 3, device=DEV)
    seen = {}
    real = ops.grad_tail_adam

    def spy(*a, **k):
        seen["a"], seen["k"] = a, k
        return real(*a, **k)

    ops.grad_tail_adam = spy
    try:
        for _ in range(3):
            tr.step(rays, ts, tgt, validate=False)
        torch.cuda.synchronize()
    finally:
        ops.grad_tail_adam = real
    return tr, models, seen["a"], dict(seen["k"])


@pytest.mark.parametrize("n", [128, 1024])
def test_tail_launches_on_a_recorded_step(n):
    from satnerf_amd import ops
    from satnerf_amd.models import _stream_kind

    tr, models, a, k = recorded_step(n)
    tail, (params, m, v, late_idx, state) = a[:21], a[21:26]
    g_sky, g_emb, ts, tau, hidden = tail[11:15], tail[20], tail[16], tail[19], tail[6].shape[0]
    assert tail[17] == n and k["pack"] is not None
    grads = tr.state.grads
    late = late_idx.long()
    mlp = torch.ones(grads.numel(), dtype=torch.bool, device=DEV)
    mlp[late] = False
    scratch = ops.late_grad_scratch(n, hidden, tau, DEV)
    assert scratch.numel() * 4 == R.scratch_bytes(n, hidden, tau)
    # sr_grad_tail_det against sr_grad_tail, on top of a non-zero gradient buffer
    g_init = torch.randn(grads.numel(), generator=torch.Generator().manual_seed(3)).to(DEV) * 1e-3
    grads.copy_(g_init)
    ops.grad_tail(*tail)
    want = grads.clone()
    grads.copy_(g_init)
    sky0, emb0 = R.join_sky(*[t.cpu().numpy() for t in g_sky]), g_emb.cpu().numpy().copy()
    ops.grad_tail_det(*tail, scratch)
    torch.cuda.synchronize()
    got = grads.clone()
    assert torch.equal(got[mlp], want[mlp]) and not torch.equal(got[mlp], g_init[mlp])
    assert not torch.equal(got[late], g_init[late])
    counter, sky_part, emb_part, first = R.scratch_views(scratch, n, hidden, n, tau)
    assert counter == 0 and (first == R.first_of_row(ts.cpu().numpy())).all()
    assert same_bits(R.join_sky(*[t.cpu().numpy() for t in g_sky]), R.reduce_sky(sky_part, sky0))
    assert same_bits(g_emb.cpu().numpy(), R.reduce_emb(emb_part, ts.cpu().numpy(), emb0))
    # sr_grad_tail_adam_det against sr_grad_tail_det + sr_adam_step_graph from the same state.  The fused and the unfused launches share
    # adam_one, but the compiler contracts its multiply-adds per kernel: from non-zero moments sr_grad_tail_adam itself differs from ITS pair
    # in the last bit of a fifth of the first moments (split-K range and `late` alike).  With zero moments -- a first step's -- b * 0 + x has
    # one value however it is contracted, so that is the state at which "the same update" can be asked bit for bit, as
    # test_fused_tail_adam_matches_tail_then_adam asks it after one step ...
    snap = (params.clone(), m.clone(), v.clone())
    assert float(m.abs().max()) > 0 and float(v.abs().max()) > 0

    def restore(moments=True):
        params.copy_(snap[0])
        m.copy_(snap[1]) if moments else m.zero_()
        v.copy_(snap[2]) if moments else v.zero_()
        grads.zero_()

    def fused(fn, *extra):
        fn(*tail, params, m, v, late_idx, state, *extra, **k)
        torch.cuda.synchronize()
        assert float(grads.abs().max()) == 0.0 and int(state.view(torch.int32)[3].item()) == 0 and int(scratch[:1].view(torch.int32).item()) == 0
        return params.clone(), m.clone(), v.clone()

    restore(moments=False)
    ops.grad_tail_det(*tail, scratch)
    assert grads.numel() == params.numel()
    ops.adam_step_graph(params, grads, m, v, state, lr=-1.0, grad_scale=1.0, zero_grad=True)
    torch.cuda.synchronize()
    ref = (params.clone(), m.clone(), v.clone())
    assert not torch.equal(ref[0][late], snap[0][late]) and not torch.equal(ref[0][mlp], snap[0][mlp])
    restore(moments=False)
    for x, y, what in zip(fused(ops.grad_tail_adam_det, scratch), ref, ("params", "exp_avg", "exp_avg_sq")):
        assert torch.equal(x, y), (what, int((x != y).sum()))
    # ... and from the recorded, non-zero moments: outside `late` the launch is sr_grad_tail_adam bit for bit (the split-K range is the same
    # code); inside, it is the SAME bits whenever it runs, which the atomic launch is not asked
    restore()
    atomic = fused(ops.grad_tail_adam)
    restore()
    det = fused(ops.grad_tail_adam_det, scratch)
    restore()
    again = fused(ops.grad_tail_adam_det, scratch)
    for x, y, z, what in zip(det, atomic, again, ("params", "exp_avg", "exp_avg_sq")):
        assert torch.equal(x[mlp], y[mlp]) and torch.equal(x, z), what
    assert not torch.equal(det[0][late], snap[0][late])
    # ... and its pack leaves the streams a fresh sr_pack_all of the updated parameters
    model = models["coarse"]
    bufs, maps = model._pack_cache[("buf", _stream_kind("bf16"), True)], model._device_maps()
    hi2, l02 = torch.full_like(bufs["hi"], -1), torch.full_like(bufs["l0"], -1.0)
    ops.pack_all(model.flat_params(), bufs["idx"], bufs["scale"], hi2, None, maps["l0_idx"], maps["l0_scale"], l02, None)
    torch.cuda.synchronize()
    assert k["pack"]["hi"].data_ptr() == bufs["hi"].data_ptr() and torch.equal(hi2, bufs["hi"]) and torch.equal(l02, bufs["l0"])
    # the scratch's dtype, device and size are checked before the launch
    with pytest.raises(ValueError, match="scratch"):
        ops.grad_tail_det(*tail, scratch[:-1])
    with pytest.raises(ValueError, match="scratch"):
        ops.grad_tail_adam_det(*tail, params, m, v, late_idx, state, scratch.double(), **k)
    with pytest.raises(ValueError, match="scratch"):
        ops.grad_tail_det(*tail, scratch.cpu())
    restore()


# ---- trainer level -----------------------------------------------------------------------------------------------------------------------
VARIANTS = {
    "four launches": dict(steps=12),
    "tail then Adam": dict(steps=12, env={"SATNERF_TAIL_ADAM": "0"}),
    "eager": dict(steps=12, use_graph=False),
    "solar correction and depth": dict(steps=6, args=dict(sc_lambda=0.1, ds_lambda=1000.0), depth=True),
    "s-nerf": dict(steps=6, args=dict(model="s-nerf")),
    "width 512": dict(steps=4, args=dict(fc_units=512)),
}


def train(variant, deterministic=True, steps=None):
    """One trainer from the fixed seeds on the fixed bank: (parameters, both moments, losses, trainer, bank, initial parameters)."""
    from satnerf_amd.data import DepthBank, RayBank
    from satnerf_amd.models import load_model
    from satnerf_amd.train import Trainer

    cfg = VARIANTS[variant]
    n_bank, bs = 4 * 128 + 9, 128
    rays, ts = O.synthetic_rays(n_bank, seed=34)
    rgbs = torch.rand(n_bank, 3, generator=torch.Generator().manual_seed(35))
    torch.manual_seed(0)
    args = O.default_args(mlp_mode="bf16", **cfg.get("args", {}))
    models = {"coarse": load_model(args).to(DEV)}
    if args.model != "s-nerf":
        models["t"] = torch.nn.Embedding(30, 4).to(DEV)
    tr = Trainer(models, args, steps_per_epoch=1000, use_graph=cfg.get("use_graph", True), deterministic=deterministic)
    bank = RayBank(rays.to(DEV), rgbs.to(DEV), ts.to(DEV), bs, seed=9)
    dbank = None
    if cfg.get("depth"):
        d_rays, d_ts = O.synthetic_rays(3 * 64 + 5, seed=36)
        g = torch.Generator().manual_seed(37)
        depths = torch.stack([0.3 + 0.4 * torch.rand(d_rays.shape[0], generator=g), 0.5 + torch.rand(d_rays.shape[0], generator=g)], 1)
        dbank = DepthBank(d_rays.to(DEV), depths.to(DEV), d_ts.to(DEV), batch_size=64, seed=10)
    losses, start = [], tr.state.params.clone()
    for _ in range(cfg["steps"] if steps is None else steps):
        losses.append(tr.step_from_bank(bank, dbank).item())
    torch.cuda.synchronize()
    return tr.state.params.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), losses, tr, bank, start


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_two_deterministic_trainings_are_the_same_bits(monkeypatch, variant):
    for name in STEP_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in VARIANTS[variant].get("env", {}).items():
        monkeypatch.setenv(name, value)
    a, b = train(variant), train(variant)
    tr = a[4]
    assert tr.direct and tr.deterministic and (tr._graph is not None) == VARIANTS[variant].get("use_graph", True)
    assert any(name.endswith("_det") for name in tr._plan(a[5]).names)
    assert all(x == x for x in a[3]) and not torch.equal(a[0], a[6]) and torch.equal(a[6], b[6])  # finite losses, parameters that moved
    assert a[3] == b[3], (a[3], b[3])
    for x, y, what in zip(a[:3], b[:3], ("params", "exp_avg", "exp_avg_sq")):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (variant, what, int((x != y).sum()))


def test_deterministic_capture_records_the_det_tail(monkeypatch):
    """The launches a capture records are the ones the plan names, sr_grad_tail_adam_det last: every call through the C ABI made while
    ops.graph_capture is open, host-only entry points aside."""
    from satnerf_amd import _lib, ops

    for name in STEP_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    recorded, recording = [], [False]
    real_call, real_capture = _lib.call, ops.graph_capture

    def call(name, *args):
        if recording[0]:
            recorded.append(name)
        return real_call(name, *args)

    @contextlib.contextmanager
    def capture(graph):
        with real_capture(graph):
            recording[0] = True
            try:
                yield
            finally:
                recording[0] = False

    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(ops, "graph_capture", capture)
    *_, losses, tr, bank, _ = train("four launches", steps=1)
    plan = tr._plan(bank)
    launched = tuple(n for n in recorded if n != "sr_wgrad_plan")  # (the split-K plan is made on the host)
    assert tr._graph is not None and losses[0] == losses[0] and int(tr.adam_state[0].item()) == 1
    assert launched == plan.names == ("sr_satnerf_render_train", "sr_satnerf_mlp_bwd", "sr_satnerf_wgrad8", "sr_grad_tail_adam_det")


def test_deterministic_step_is_the_default_step_up_to_the_late_sums(monkeypatch):
    """One step: outside `late` the two trainers' parameters are the same bits (same batch, same jitter, same split-K sums, same Adam); inside,
    Adam's first update is at most lr per parameter, so two of them differ by at most 2 lr."""
    for name in STEP_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    det, default = train("four launches", steps=1), train("four launches", deterministic=False, steps=1)
    tr = det[4]
    late = tr._late_idx.long()
    mlp = torch.ones(det[0].numel(), dtype=torch.bool, device=DEV)
    mlp[late] = False
    assert torch.equal(det[0][mlp], default[0][mlp]) and det[3] == default[3]
    assert (det[0][late] - default[0][late]).abs().max().item() <= 2 * tr.lr
    assert not default[4].deterministic and "sr_grad_tail_adam" in default[4]._plan(default[5]).names
