"""The weight stream of the fused classic-NeRF kernel (packing.nerf_forward_maps), checked on the CPU: it holds every parameter once, and
a float64 walk that consumes it in the kernel's stage / tile / k-step order (csrc/nerf_fwd.inc) is the oracle's nerf_mlp."""
import os

import numpy as np
import pytest
import torch

from oracle import satnerf_oracle as O
from satnerf_amd import _lib, packing
from tests import nerf_reference as R


@pytest.fixture(scope="module")
def handle():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.lib()


def test_every_parameter_is_read_exactly_once():
    m = packing.nerf_forward_maps(256)
    idx, scale = m["idx"], m["scale"]
    live = idx >= 0
    assert m["n_params"] == sum(int(np.prod(s)) for s in O.nerf_param_shapes(256).values())
    assert np.array_equal(np.sort(idx[live]), np.arange(m["n_params"]))
    assert (scale[live] == 1).all() and (scale[~live] == 0).all() and (idx[~live] == -1).all()
    assert list(packing.nerf_param_shapes(256).items()) == list(O.nerf_param_shapes(256).items())  # the flat buffer's order
    with pytest.raises(ValueError):
        packing.nerf_forward_maps(384)


def test_stream_length_matches_the_library(handle):
    assert handle.sr_nerf_stream_elems(256) == packing.nerf_forward_maps(256)["idx"].size
    assert handle.sr_nerf_stream_elems(256) == 512 * sum(t * p for _, t, p in packing.nerf_stages(256))
    assert handle.sr_nerf_stream_elems(384) == -1 and handle.sr_nerf_stream_elems(512) == -1
    assert handle.sr_nerf_render_max_samples() == 256


def _walk(stream, xyz, dirs):
    """The kernel's schedule in float64: per stage, per 32-row tile, per 1-KiB piece [h][r][j] = rows 32 t + r, slots 16 s + 8 h + j; B
    operands in slot order: encoded k-steps as computed, activations permuted by slot_to_feat, a constant-1 k-step."""
    n = xyz.shape[0]
    pos = 0

    def aux(values, width, one):
        a = np.zeros((n, width))
        a[:, :values.shape[1]] = values
        a[:, one] = 1.0
        return a

    def slots(act):
        return act[:, packing.slot_to_feat(np.arange(act.shape[1]))]

    def stage(tiles, srcs):
        nonlocal pos
        b = np.concatenate(srcs, 1)
        ns = b.shape[1] // 16
        a = stream[pos:pos + tiles * ns * 512].reshape(tiles, ns, 2, 32, 8)
        pos += tiles * ns * 512
        return b @ a.transpose(0, 3, 1, 2, 4).reshape(tiles * 32, ns * 16).T

    enc = aux(O.positional_map(xyz, 10).numpy(), 16 * packing.NERF_ENC_STEPS, packing.NERF_ENC_ONE)
    dirf = aux(O.positional_map(dirs, 4).numpy(), 16 * packing.NERF_DIR_STEPS, packing.NERF_DIR_ONE)
    ones = aux(np.zeros((n, 0)), 16, 0)
    relu = lambda v: np.maximum(v, 0)  # noqa: E731
    h = relu(stage(8, [enc]))
    for layer in range(1, 8):
        h = relu(stage(8, [enc, slots(h)] if layer == 4 else [slots(h), ones]))
    feats = stage(8, [slots(h), ones])
    sigma = np.logaddexp(0, stage(1, [slots(h), ones])[:, 0])
    hid = relu(stage(4, [slots(feats), dirf]))
    logits = stage(1, [slots(hid), ones])
    assert pos == stream.size
    assert np.all(logits[:, 3:] == 0)  # the tile's unused rows are padding
    return 1.002 / (1 + np.exp(-logits[:, :3])) - 0.001, sigma


def test_float64_walk_of_the_stream_is_the_oracle():
    m = packing.nerf_forward_maps(256)
    for seed in (1, 2):
        p = {k: v.double() for k, v in R.lively_nerf_params(256, seed).items()}
        flat = torch.cat([p[k].reshape(-1) for k in packing.nerf_param_shapes(256)]).numpy()
        stream = np.where(m["idx"] >= 0, flat[np.maximum(m["idx"], 0)] * m["scale"].astype(np.float64), 0.0)
        xyz, d = R.points(64, 40 + seed)
        xyz, d = xyz.double(), d.double()
        rgb, sigma = _walk(stream, xyz, d)
        want = O.nerf_mlp(p, xyz, d).numpy()
        assert np.abs(rgb - want[:, :3]).max() < 1e-12 * np.abs(want[:, :3]).max()
        assert np.abs(sigma - want[:, 3]).max() < 1e-12 * np.abs(want[:, 3]).max()
