#!/usr/bin/env python3
"""Generate the depth-supervision fixture under tests/golden/depth_supervision/ by RUNNING THE REFERENCE's SatelliteDataset_depth.

Runs only in the build container (needs /root/reference, read-only).  A small synthetic scene is written as DATA -- ``scene.loc``,
``train.txt``, ``test.txt``, one JSON per image and ``pts3d.npy`` -- and ``datasets/satellite_depth.SatelliteDataset_depth(root,
root, split="train")`` runs on it unmodified.  Its two calls into the absent ``rpcm`` package (``RPCModel.localization`` in
``get_rays``, ``RPCModel.projection`` in the keypoint weights) are supplied by a duck-typed rpc object whose methods are
``oracle/rpc_oracle.py``'s, as ``make_golden.py``'s ``rpc_rays_case`` does; ``rasterio``, ``torchvision`` and ``kornia`` (the last
imported by ``datasets/__init__.py`` for the Blender loader; none is called on this path) are stubbed, and ``PIL`` too where it is
absent.  The reference's error matrix, ``e``, ``e_mean`` and weights, which it keeps
in locals, are recorded through a numpy proxy installed as the module's ``np`` that forwards every call.

The scene: 9 training images (``rpc_oracle.synthetic_rpc`` with distinct seeds) and one test image the training split must ignore;
400 tie points in the common footprint, 12 of them (3 %) seen by no training image; keypoints = the RPC projection + 0.3 px noise,
a few 5-20 px outliers, and one observation listed twice in one image (numpy's assignment keeps the last).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_depth_golden.py            # rewrite the fixture
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_depth_golden.py --check    # regenerate in a temporary directory, compare bit for bit

The expected outputs go to ``reference.npz`` (fixed zip timestamps: the same arrays give the same file bytes).
"""
import argparse
import importlib.machinery
import io
import json
import os
import sys
import tempfile
import types
import zipfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "depth_supervision")
REF = "/root/reference"
N_TRAIN, N_PTS, N_UNSEEN = 9, 400, 12
FILES = ["scene.loc", "train.txt", "test.txt", "pts3d.npy"] + [f"img_{k:02d}.json" for k in range(N_TRAIN + 1)]


def make_scene(root):
    """Write the synthetic dataset under root (deterministic: seeded generators, JSON floats printed with repr)."""
    sys.path.insert(0, REPO)
    from oracle import rpc_oracle as R

    g = np.random.default_rng(zlib.crc32(b"depth_supervision"))
    lat0, lon0 = 30.30, -81.66
    lat = lat0 + g.uniform(-0.5, 0.5, N_PTS) * 0.0035
    lon = lon0 + g.uniform(-0.5, 0.5, N_PTS) * 0.0040
    alt = g.uniform(-15.0, 45.0, N_PTS)
    pts3d = np.stack(R.latlon_to_ecef(lat, lon, alt), 1)
    np.save(os.path.join(root, "pts3d.npy"), pts3d)
    lo, hi = pts3d.min(0), pts3d.max(0)
    loc = {"X_scale": float((hi[0] - lo[0]) / 2 + 40.0), "X_offset": float((hi[0] + lo[0]) / 2),
           "Y_scale": float((hi[1] - lo[1]) / 2 + 40.0), "Y_offset": float((hi[1] + lo[1]) / 2),
           "Z_scale": float((hi[2] - lo[2]) / 2 + 40.0), "Z_offset": float((hi[2] + lo[2]) / 2)}
    with open(os.path.join(root, "scene.loc"), "w") as f:
        json.dump(loc, f, indent=2)
    unseen = set(g.choice(N_PTS, N_UNSEEN, replace=False).tolist())
    seen = np.array([p for p in range(N_PTS) if p not in unseen])
    views = [seen[g.random(seen.size) < 0.75] for _ in range(N_TRAIN)]
    covered = set(np.concatenate(views).tolist())
    views[0] = np.concatenate([views[0], np.array(sorted(set(seen.tolist()) - covered), dtype=np.int64)])
    views.append(np.arange(N_PTS)[g.random(N_PTS) < 0.5])  # the test image (sees unseen points too)
    for k, idx in enumerate(views):
        h, w = int(g.integers(300, 420)), int(g.integers(320, 480))
        rpc = R.synthetic_rpc(100 + 7 * k, height=h, width=w)
        idx = g.permutation(idx)
        col, row = R.projection(rpc, lon[idx], lat[idx], alt[idx])
        col = col + g.normal(0.0, 0.3, idx.size)
        row = row + g.normal(0.0, 0.3, idx.size)
        out = g.choice(idx.size, 3, replace=False)  # outliers
        ang = g.uniform(0, 2 * np.pi, 3)
        rad = g.uniform(5.0, 20.0, 3)
        col[out] += rad * np.cos(ang)
        row[out] += rad * np.sin(ang)
        coords = np.stack([col, row], 1).tolist()
        idx = idx.tolist()
        if k == 2:  # one point observed twice in one image: the later entry is what the reference keeps
            coords.append([coords[5][0] + 1.7, coords[5][1] - 2.2])
            idx.append(idx[5])
        d = {"img": f"img_{k:02d}.tif", "height": h, "width": w, "min_alt": float(-30.0 - 2 * k), "max_alt": float(70.0 + 3 * k),
             "sun_elevation": float(g.uniform(35, 75)), "sun_azimuth": float(g.uniform(100, 220)),
             "rpc": {key: (v.tolist() if isinstance(v, np.ndarray) else float(v)) for key, v in rpc.items()},
             "keypoints": {"2d_coordinates": coords, "pts3d_indices": idx}}
        with open(os.path.join(root, f"img_{k:02d}.json"), "w") as f:
            json.dump(d, f)
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("\n".join(f"img_{k:02d}.json" for k in range(N_TRAIN)))  # no trailing newline: the reference would read it as a file
    with open(os.path.join(root, "test.txt"), "w") as f:
        f.write(f"img_{N_TRAIN:02d}.json")


class _Stub(types.ModuleType):
    """Inert stand-in for an absent third-party import (never called on this path)."""

    def __init__(self, name):
        super().__init__(name)
        self.__path__ = []
        self.__spec__ = importlib.machinery.ModuleSpec(name, None)

    def __getattr__(self, item):
        if item.startswith("__"):
            raise AttributeError(item)
        return _Stub(f"{self.__name__}.{item}")

    def __call__(self, *a, **k):
        return _Stub(self.__name__ + "()")


def run_reference(root):
    """SatelliteDataset_depth(root, root) -> the arrays it builds, plus the locals of its keypoint weights."""
    import torch

    sys.path.insert(0, REPO)
    sys.path.insert(0, REF)
    from oracle import rpc_oracle as R

    class DuckRPC:  # rpcm.RPCModel(d, dict_format="rpcm"): the attributes sat_utils.rescale_rpc touches + localization / projection
        def __init__(self, d, dict_format="rpcm"):
            assert dict_format == "rpcm"
            self.d = dict(d)
            for k in ("row_scale", "col_scale", "row_offset", "col_offset"):
                setattr(self, k, float(d[k]))

        def _dict(self):
            return dict(self.d, row_scale=self.row_scale, col_scale=self.col_scale, row_offset=self.row_offset, col_offset=self.col_offset)

        def localization(self, cols, rows, alts):
            return R.localization(self._dict(), cols, rows, alts)

        def projection(self, lon, lat, alt):
            return R.projection(self._dict(), lon, lat, alt)

    rpcm = types.ModuleType("rpcm")
    rpcm.RPCModel = DuckRPC
    stubs = {"rpcm": rpcm}
    for m in ("rasterio", "torchvision", "torchvision.transforms", "kornia") + (() if _has("PIL") else ("PIL", "PIL.Image")):
        stubs[m] = _Stub(m)
    saved = {m: sys.modules.get(m) for m in stubs}
    sys.modules.update(stubs)
    rec = {}

    class NpSpy:  # the module's `np`: forwards everything, records the keypoint-weight locals (satellite_depth.py:125-127)
        def __getattr__(self, item):
            return getattr(np, item)

        def sum(self, a, axis=None):
            rec["errmat"], rec["e"] = np.array(a), np.sum(a, axis=axis)
            return rec["e"]

        def mean(self, a):
            rec["e_mean"] = np.mean(a)
            return rec["e_mean"]

        def exp(self, a):
            rec["kp_weights"] = np.exp(a)
            return rec["kp_weights"]

    try:
        import datasets.satellite_depth as sd

        sd.np = NpSpy()
        torch.set_num_threads(1)
        ds = sd.SatelliteDataset_depth(root, root, split="train")
    finally:
        for m, v in saved.items():
            if v is None:
                sys.modules.pop(m, None)
            else:
                sys.modules[m] = v
    return {"all_rays": ds.all_rays.numpy(), "all_depths": ds.all_depths.numpy(), "all_ids": ds.all_ids.numpy(),
            "center": ds.center.numpy(), "range": np.float32(ds.range.item()), "errmat": rec["errmat"], "e": rec["e"],
            "e_mean": np.float32(rec["e_mean"]), "kp_weights": rec["kp_weights"]}


def _has(mod):
    try:
        __import__(mod)
        return True
    except ImportError:
        return False


def npz_bytes(arrays):
    """np.savez_compressed with fixed member timestamps: equal arrays -> equal file bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, b.getvalue())
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--check", action="store_true", help="write nothing: regenerate in a temporary directory and compare bit for bit")
    a = ap.parse_args()
    sys.dont_write_bytecode = True
    with tempfile.TemporaryDirectory() as tmp:
        make_scene(tmp)
        ref = run_reference(tmp)
        blob = npz_bytes(ref)
        if a.check:
            bad = [f for f in FILES if open(os.path.join(tmp, f), "rb").read() != open(os.path.join(OUT, f), "rb").read()]
            z = np.load(os.path.join(OUT, "reference.npz"), allow_pickle=False)
            bad += sorted(set(z.files) ^ set(ref))
            for k in sorted(set(z.files) & set(ref)):
                x, y = np.asarray(ref[k]), z[k]
                if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
                    bad.append(k)
            print(f"depth_supervision  {'OK: ' + str(len(FILES)) + ' files and ' + str(len(ref)) + ' arrays bit-equal' if not bad else 'MISMATCH: ' + ', '.join(bad)}")
            return 1 if bad else 0
        os.makedirs(OUT, exist_ok=True)
        for f in FILES:
            with open(os.path.join(tmp, f), "rb") as src, open(os.path.join(OUT, f), "wb") as dst:
                dst.write(src.read())
        with open(os.path.join(OUT, "reference.npz"), "wb") as f:
            f.write(blob)
    extra = sorted(set(os.listdir(OUT)) - set(FILES) - {"reference.npz"})
    assert not extra, f"files without a recipe: {extra}"
    print(f"depth_supervision  {len(FILES)} files + reference.npz ({len(blob) / 1024:.0f} KiB), {ref['all_rays'].shape[0]} observations")
    return 0


if __name__ == "__main__":
    sys.exit(main())
