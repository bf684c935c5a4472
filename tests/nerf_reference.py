"""Reference of the fused classic-NeRF forward (csrc/nerf_fwd.inc): the chain of ``NeRF.forward`` (models/nerf.py:184-227) with the operands
the kernel's MFMAs see -- weights, biases and every layer's inputs rounded to bf16 (round to nearest even), the positional encodings
included -- and wide accumulation.  Helper module, no tests.

``procedural_nerf_params`` gives an almost constant network (sigma in 0.690 .. 0.700), on which a wrong column order moves the outputs by
3e-5: the yardstick is ``lively_nerf_params`` (weights times sqrt(6), which keeps the variance under ReLU), on which every planted fault
below moves rgb or sigma by several percent (tests/test_nerf_reference_host.py).
"""
import math

import torch
import torch.nn.functional as F

from oracle import satnerf_oracle as O
from satnerf_amd import packing

IN_XYZ, IN_DIR = 60, 24


def lively_nerf_params(feat=256, seed=1):
    return {k: (v * math.sqrt(6.0) if k.endswith(".weight") else v.clone()) for k, v in O.procedural_nerf_params(feat, seed=seed).items()}


def bf16(t):
    """Round to bf16 (nearest even) by way of fp32, the path a kernel's fp32 accumulator takes; returned in float64."""
    return t.float().to(torch.bfloat16).double()


def chain(params, xyz, dirs, row_div=1, rounded=True, acc=torch.float64):
    """rgb (P,3), sigma (P,) in float64.  ``rounded``: bf16 operands; ``acc``: the accumulation type of the layers."""
    rnd = bf16 if rounded else (lambda t: t.double())
    xyz, dirs = xyz.float().cpu(), dirs.float().cpu()
    d_pts = dirs if row_div == 1 else torch.repeat_interleave(dirs, row_div, dim=0)[:xyz.shape[0]]

    def lin(x, name):
        w, b = rnd(params[name + ".weight"]), rnd(params[name + ".bias"])
        return F.linear(x.to(acc), w.to(acc), b.to(acc)).double()

    e = rnd(O.positional_map(xyz, 10))  # fp32, as the oracle computes it
    h = e
    for i in range(8):
        if i == 4:
            h = torch.cat([e, h], -1)
        h = rnd(torch.relu(lin(h, f"fc_net.{2 * i}")))
    sigma = F.softplus(lin(h, "sigma_from_xyz.0"))[:, 0]
    feats = rnd(lin(h, "feats_from_xyz"))
    r = torch.cat([feats, rnd(O.positional_map(d_pts, 4))], -1)
    r = rnd(torch.relu(lin(r, "rgb_from_xyzdir.0")))
    rgb = torch.sigmoid(lin(r, "rgb_from_xyzdir.2")) * (1 + 2 * 0.001) - 0.001
    return rgb, sigma


# ---- planted faults: what a wrong stream layout or stage list would compute ------------------------------------------------------------
def _with(params, **changed):
    out = {k: v.clone() for k, v in params.items()}
    out.update(changed)
    return out


def fault_kstep_zeroed(p, step=5):
    """One 16-column k-step of fc_net.6 zeroed (the columns the kernel's k-step holds: packing.slot_to_feat)."""
    w = p["fc_net.6.weight"].clone()
    w[:, torch.from_numpy(packing.slot_to_feat(16 * step + torch.arange(16).numpy()))] = 0
    return _with(p, **{"fc_net.6.weight": w})


def fault_skip_halves_exchanged(p):
    """fc_net.8 reading [h | enc] where torch.cat([e, h]) gives [enc | h]."""
    w = p["fc_net.8.weight"]
    return _with(p, **{"fc_net.8.weight": torch.cat([w[:, IN_XYZ:], w[:, :IN_XYZ]], 1)})


def fault_last_encoded_column_l0(p):
    w = p["fc_net.0.weight"].clone()
    w[:, IN_XYZ - 1] = 0
    return _with(p, **{"fc_net.0.weight": w})


def fault_encoded_column_skip(p):
    w = p["fc_net.8.weight"].clone()
    w[:, 3] = 0
    return _with(p, **{"fc_net.8.weight": w})


def fault_encoded_dir_column(p):
    w = p["rgb_from_xyzdir.0.weight"].clone()
    w[:, w.shape[1] - IN_DIR + 5] = 0
    return _with(p, **{"rgb_from_xyzdir.0.weight": w})


def fault_tile_zeroed(p):
    """Rows 64..95 of fc_net.10 (one output tile) zeroed, with their bias."""
    w, b = p["fc_net.10.weight"].clone(), p["fc_net.10.bias"].clone()
    w[64:96] = 0
    b[64:96] = 0
    return _with(p, **{"fc_net.10.weight": w, "fc_net.10.bias": b})


def fault_columns_exchanged(p):
    w = p["fc_net.6.weight"].clone()
    w[:, [0, 1]] = w[:, [1, 0]]
    return _with(p, **{"fc_net.6.weight": w})


FAULTS = {
    "k-step zeroed (fc_net.6)": fault_kstep_zeroed,
    "[enc | h] exchanged (fc_net.8)": fault_skip_halves_exchanged,
    "encoded-xyz column 59 zeroed (fc_net.0)": fault_last_encoded_column_l0,
    "encoded-xyz column 3 zeroed (fc_net.8)": fault_encoded_column_skip,
    "encoded-dir column 5 zeroed": fault_encoded_dir_column,
    "rows 64..95 zeroed (fc_net.10)": fault_tile_zeroed,
    "columns 0 / 1 exchanged (fc_net.6)": fault_columns_exchanged,
}


def points(n, seed):
    """n points in [-4, 4]^3 and unit directions."""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(n, 3, generator=g) * 8 - 4
    d = torch.randn(n, 3, generator=g)
    return xyz, d / d.norm(dim=1, keepdim=True)
