"""The per-ray kernels against the float64 restatement of tests/ray_reference.py, element by element under its gates:
sr_render_loss, sr_composite_fwd + sr_composite_bwd, sr_satnerf_loss, sr_sc_loss, sr_depth_loss, sr_composite_image, each called
through satnerf_amd.ops on the input sets of ray_reference.CASES (tests/test_ray_reference_host.py runs the same sets through a float32
emulation, plants the faults and asserts what the inputs reach).  The loss is the float64 sum of loss_parts.  sr_composite_bwd is held to
the reference of what it reads: the weights and transparency sr_composite_fwd wrote, which the forward half of the same case has held to
their own gate.

Worst |error| / gate per kernel and output over all cases, MI355X (a record: it informs, nothing is derived from it; the emulation's
figures stand in tests/test_ray_reference_host.py):
  render_loss      rgb 0.17   d_sigma 0.09   d_albedo 0.34   d_sun 0.33   g_beta 0.33   d_sky 0.16   loss 0.16
  composite        weights 0.42   transp 0.38   depth 0.12   rgb 0.18
  composite_bwd    d_sigma 0.22   d_albedo 0.99   d_sun 0.53   d_sky 0.22      (d_albedo without a sun head: one rounding, a sharp gate)
  satnerf_loss     g_rgb 0.33   g_weights 0.13   g_beta 0.11   loss 0.01
  sc_loss          d_sun 0.52   loss 0.01
  depth_loss       g_depth 0.56   loss 0.12
  composite_image  0.16"""
import pytest
import torch

from . import ray_reference as R
from .test_hip_parity import DEV

pytestmark = pytest.mark.gpu

ALL = [(kind, case) for kind, cases in R.CASES.items() for case in cases]
WORST = {}


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _sched(warm):
    """The captured step's schedule block: [step, learning rate, warm-up flag, reserved]."""
    return torch.tensor([3.0, 5e-4, 1.0 if warm else 0.0, 0.0], device=DEV)


def _total(parts):
    return float(parts.double().sum())


def device(kind, case):
    """The kernels' outputs for one case, named as ray_reference names them."""
    from satnerf_amd import ops

    inp = R.case_inputs(kind, case)
    if kind == "depth_loss":
        parts, g = ops.depth_loss(_d(inp["depth"]), _d(inp["depths"]), R.LAMBDA_DS, use_weights=case["use_weights"])
        assert parts.numel() == (case["n"] + 255) // 256
        return {"loss": _total(parts), "g_depth": g}
    if kind == "satnerf_loss":
        parts, g_rgb, g_w, g_b = ops.satnerf_loss(_d(inp["rgb"]), _d(inp["weights"]), _d(inp["beta"]), _d(inp["target"]), beta_min=0.05,
                                                  grad_scale=case["grad_scale"], sched=_sched(case["warm"]))
        return {"loss": _total(parts), "g_rgb": g_rgb, "g_weights": g_w, "g_beta": g_b}
    ray = (_d(inp["z"]), _d(inp["sigma"]), _d(inp["noise"]), inp["noise_std"])
    if kind == "render_loss":
        out = ops.render_loss(*ray, _d(inp["albedo"]), _d(inp["sun_v"]), _d(inp["beta"]), _d(inp["sky"]), _d(inp["target"]), sched=_sched(case["warm"]))
        return dict(zip(("loss", "rgb", "d_sigma", "d_albedo", "d_sun", "g_beta", "d_sky"), (_total(out[0]),) + tuple(out[1:])))
    if kind == "composite":
        head = (_d(inp["albedo"]), _d(inp["sun_v"]), _d(inp["sky"]))
        w, t, depth, rgb = ops.composite(*ray, *head, clamp_rgb=inp["clamp"])
        grads = ops.composite_bwd(*ray, *head, w, t, _d(inp["g_rgb"]), _d(inp["g_depth"]), _d(inp["g_w"]), _d(inp["g_T"]), clamp_rgb=inp["clamp"])
        return dict(zip(("weights", "transp", "depth", "rgb", "d_sigma", "d_albedo", "d_sun", "d_sky"), (w, t, depth, rgb) + tuple(grads)))
    if kind == "sc_loss":
        parts, d_sun = ops.sc_loss(*ray, _d(inp["sun_v"]), R.LAMBDA_SC)
        return {"loss": _total(parts), "d_sun": d_sun}
    if kind == "composite_image":
        return {"image": ops.composite_image(*ray, _d(inp["albedo"]), _d(inp["sun_v"]), _d(inp["beta"]), _d(inp["sky"]))}
    raise KeyError(kind)


@pytest.mark.parametrize("kind,case", ALL, ids=[f"{k}-{R.case_id(c)}" for k, c in ALL])
def test_kernel_is_inside_every_gate(kind, case):
    got = device(kind, case)
    torch.cuda.synchronize()
    res = R.compare(kind, case, got)
    for k, v in res.items():
        WORST[(kind, k)] = max(WORST.get((kind, k), 0.0), v)
    print("ratio", kind, R.case_id(case), {k: round(v, 3) for k, v in res.items()})
    assert res and all(v <= 1.0 for v in res.values()), res


def test_worst_ratios_are_printed():
    """Runs last in this module: the record for the header."""
    for (kind, k), v in sorted(WORST.items()):
        print(f"worst {kind:16s} {k:10s} {v:.3f}")


def test_render_loss_at_the_default_beta_min_and_without_a_schedule_block():
    """``beta_min`` left at its default and no ``sched`` at all is the non-warm-up loss: bit for bit what the schedule block with a zero
    flag gives."""
    from satnerf_amd import ops

    kind, case = "render_loss", R.CASES["render_loss"][0]
    inp = R.case_inputs(kind, case)
    a = [_d(inp[k]) if torch.is_tensor(inp[k]) else inp[k] for k in ("z", "sigma", "noise", "noise_std", "albedo", "sun_v", "beta", "sky", "target")]
    plain, sched = ops.render_loss(*a), ops.render_loss(*a, beta_min=0.05, sched=_sched(False))
    assert all(torch.equal(x, y) for x, y in zip(plain, sched))


def test_reference_runs_on_the_device():
    """The same reference evaluated on the GPU: float64 throughout, so it agrees with the CPU evaluation to float64 rounding."""
    kind, case = "render_loss", R.CASES["render_loss"][0]
    inp = R.case_inputs(kind, case)
    keys = ("z", "sigma", "noise", "noise_std", "albedo", "sun_v", "beta", "sky", "target")
    cpu = R.render_loss(*[inp[k] for k in keys])
    gpu = R.render_loss(*[_d(inp[k]) if torch.is_tensor(inp[k]) else inp[k] for k in keys])
    for k in ("rgb", "d_sigma", "d_albedo", "d_sun", "g_beta", "d_sky"):
        assert gpu[k].v.is_cuda
        a, b = gpu[k].v.detach().cpu(), cpu[k].v.detach()
        assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300), k
        assert gpu[k].gate(gpu["chain"].amb(gpu[k].v)).shape == b.shape
