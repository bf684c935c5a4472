"""Host checks of the depth-only render's entry points (no GPU): CPU tensors raise as in the other entry points, and the ctypes
prototypes of the two new C entries exist and agree with include/satrender.h (in the style of tests/test_cabi.py, which also holds the
built library to every declared symbol)."""
import ctypes as C
import os
import re

import pytest
import torch

from oracle import satnerf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sr_satnerf_render_depth", "sr_satnerf_mlp_sigma")


def test_cpu_tensors_raise():
    from satnerf_amd import ops, rendering
    from satnerf_amd.models import load_model

    args = O.default_args(mlp_mode="bf16")
    models = {"coarse": load_model(args), "t": torch.nn.Embedding(args.t_embbeding_vocab, args.t_embbeding_tau)}
    rays, ts = O.synthetic_rays(4, seed=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rendering.render_depth(models, rays, ts, args)
    with pytest.raises(ValueError, match="GPU"):
        ops.render_depth(rays, ts, torch.zeros(30, 4), 64, 256, 4, "bf16", None, None, None)
    with pytest.raises(ValueError, match="GPU"):
        ops.satnerf_sigma(rays[:, 0:3], None, rays[:, 8:11], None, torch.zeros(4, 4), None, 4, 1, 256, 4, "bf16", None, None, None)
    with pytest.raises(ValueError):
        rendering.render_depth(models, rays, ts, O.default_args(model="bogus"))


def test_the_two_entries_are_declared_and_bound():
    from satnerf_amd import _lib

    with open(os.path.join(ROOT, "include", "satrender.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, f"{name} is not declared in include/satrender.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        res, argtypes = _lib.SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == n_args == 9, (name, n_args, len(argtypes))
        assert argtypes[-1] is C.c_void_p and argtypes[1:4] == [C.c_int] * 3  # (..., feat, tau, mode, ..., stream)
    assert _lib.SIGNATURES["sr_satnerf_mlp_sigma"][1][0] is _lib.SIGNATURES["sr_satnerf_mlp_fwd"][1][0]  # the same sr_mlp_inputs block
    assert _lib.SIGNATURES["sr_satnerf_render_depth"][1] == _lib.SIGNATURES["sr_satnerf_render_fwd"][1]

