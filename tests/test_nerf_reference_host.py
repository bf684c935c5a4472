"""The yardstick of the fused classic-NeRF kernel, checked on the CPU: the bf16-operand chain of tests/nerf_reference.py on lively weights
separates every planted layout fault from accumulation-order noise, and without rounding it is the oracle's nerf_mlp."""
import pytest
import torch

from oracle import satnerf_oracle as O
from tests import nerf_reference as R
from tests.helpers import maxnorm_rel

SEEDS = (1, 2, 3)


@pytest.fixture(scope="module")
def cases():
    out = []
    for seed in SEEDS:
        p = R.lively_nerf_params(256, seed)
        xyz, d = R.points(261, 100 + seed)
        out.append((p, xyz, d, R.chain(p, xyz, d)))
    return out


def _shift(a, b):
    return max(maxnorm_rel(a[0], b[0]), maxnorm_rel(a[1], b[1]))


def test_every_planted_fault_moves_the_chain(cases):
    worst = {}
    for p, xyz, d, ref in cases:
        for name, fault in R.FAULTS.items():
            s = _shift(R.chain(fault(p), xyz, d), ref)
            worst[name] = min(worst.get(name, 1e9), s)
    print({k: f"{v:.1e}" for k, v in worst.items()})
    assert min(worst.values()) > 3e-2, worst


def test_accumulation_width_is_far_below_the_faults(cases):
    worst = max(_shift(R.chain(p, xyz, d, acc=torch.float32), ref) for p, xyz, d, ref in cases)
    print(f"fp32 against fp64 accumulation: {worst:.1e}")
    assert worst < 1e-2


def test_unrounded_chain_is_the_oracle(cases):
    for p, xyz, d, _ in cases:
        rgb, sigma = R.chain(p, xyz, d, rounded=False)
        want = O.nerf_mlp(p, xyz, d)
        assert maxnorm_rel(rgb, want[:, :3]) < 1e-6 and maxnorm_rel(sigma, want[:, 3]) < 1e-6


def test_the_lively_weights_are_lively(cases):
    """What makes them a yardstick: sigma and rgb vary over the points (the plain procedural weights give sigma in 0.690 .. 0.700)."""
    for _, _, _, (rgb, sigma) in cases:
        assert sigma.max() / sigma.min() > 3 and rgb.max() - rgb.min() > 0.5
