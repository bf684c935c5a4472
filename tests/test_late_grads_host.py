"""Deterministic training steps, the parts a host can check: the launch plan names the fixed-order tails and nothing else changes, the size of
their scratch is the documented layout's, and ``Trainer(deterministic=True)`` refuses what it does not cover."""
import os

import pytest
import torch

from oracle import satnerf_oracle as O
from satnerf_amd import _lib, step_plan

from . import late_grads_reference as R
from .test_step_plan_host import ADVERTISED, captured

ROWS = ("single GPU", "tail then Adam", "two ranks, gloo", "bwd_fmt=16")
SWAP = {"sr_grad_tail": "sr_grad_tail_det", "sr_grad_tail_adam": "sr_grad_tail_adam_det"}


def planned(row, **extra):
    """``captured`` of test_step_plan_host.py with further keywords for ``launches``."""
    kw = dict(ADVERTISED[row][0])
    env, world, backend, fmt, bank = kw.get("env") or {}, kw.get("world", 1), kw.get("backend"), kw.get("fmt", 8), kw.get("bank", "RayBank")
    pg = backend is not None
    coll = step_plan.collective(world, pg, env)
    st = step_plan.capture_state(noise_zero=True, collective=coll, pg_initialised=pg, backend=backend, capture_failed=False, late_idx=True,
                                 fused_forward=step_plan.fused_forward(fmt, 64, True, env), env=env)
    return step_plan.launches(kernel_rng=st.kernel_rng, adam_in_graph=st.adam_in_graph, pack_in_tail=st.pack_in_tail, collective=coll, fmt=fmt,
                              n_samples=64, render_fused_ok=True, bank=bank is not None, ray_bank=bank == "RayBank", env=env, **extra)


@pytest.mark.parametrize("row", ROWS)
def test_deterministic_plan_swaps_the_tail_and_nothing_else(row):
    plain = captured(**ADVERTISED[row][0])
    assert planned(row) == plain                              # (this file's copy of ``captured`` is the original)
    assert planned(row, deterministic=False) == plain
    det = planned(row, deterministic=True)
    assert det._fields == plain._fields
    assert det.names == tuple(SWAP.get(n, n) for n in ADVERTISED[row][1]) and det.names != plain.names
    assert sum(n.endswith("_det") for n in det.names) == 1
    assert det._replace(names=plain.names) == plain


@pytest.fixture(scope="module")
def handle():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.lib()


@pytest.mark.parametrize("n_rays,hidden,tau", [(1, 128, 4), (77, 128, 3), (1024, 256, 16)])
def test_scratch_bytes_are_the_documented_layout(handle, n_rays, hidden, tau):
    want = 4 * (4 + -(-n_rays // 32) * (7 * hidden + 3) + n_rays * tau + n_rays)  # counter + padding | sky_part | emb_part | first
    assert handle.sr_late_grad_scratch_bytes(n_rays, hidden, tau) == want == R.scratch_bytes(n_rays, hidden, tau)
    assert want % 4 == 0 and handle.sr_late_grad_scratch_bytes(0, hidden, tau) == 16
    for bad in ((-1, hidden, tau), (n_rays, 0, tau), (n_rays, hidden, 0)):
        assert handle.sr_late_grad_scratch_bytes(*bad) == -1


def test_deterministic_trainer_refuses_what_it_does_not_cover():
    from satnerf_amd.models import load_model
    from satnerf_amd.train import Trainer, satnerf_loss

    args = O.default_args(mlp_mode="bf16")
    models = {"coarse": load_model(args), "t": torch.nn.Embedding(30, 4)}  # CPU tensors: no kernel-direct step
    with pytest.raises(ValueError, match="deterministic"):
        Trainer(models, args, steps_per_epoch=1000, deterministic=True)
    with pytest.raises(ValueError, match="loss_fn"):
        Trainer(models, args, steps_per_epoch=1000, loss_fn=satnerf_loss, deterministic=True)
    tr = Trainer(models, args, steps_per_epoch=1000)  # the default is off and stays constructible anywhere
    assert tr.deterministic is False
