#!/usr/bin/env python3
"""Generate the scene.loc fixture under tests/golden/scene_loc/ by RUNNING THE REFERENCE's SatelliteDataset.init_scaling_params.

Runs only in the build container (needs /root/reference, read-only).  A small synthetic dataset is written as DATA -- one JSON per
image, ``train.txt``, ``test.txt`` and NO ``scene.loc`` -- and ``datasets/satellite.SatelliteDataset.init_scaling_params`` runs on it
unmodified, at ``img_downscale`` 1.0 and 2.0, on an instance that carries just the two attributes the method reads (``json_dir``,
``img_downscale``; the constructor would go on to open the images).  Its call into the absent ``rpcm`` package (``RPCModel.
localization`` in ``get_rays``) is supplied by a duck-typed rpc object whose method is ``oracle/rpc_oracle.py``'s, as
``make_depth_golden.py`` does; ``rasterio``, ``torchvision`` and ``kornia`` are stubbed (none is called on this path), and ``PIL`` too
where it is absent.  ``sat_utils.write_dict_to_json`` is replaced by a recorder: the real one raises ``TypeError: Object of type
float32 is not JSON serializable`` on the np.float32 values ``sat_utils.rpc_scaling_params`` returns.  ``rpc_scaling_params`` itself
runs unmodified behind a wrapper that also records the minimum, the maximum and the size of the vector it is given.

The dataset: four images from ``rpc_oracle.synthetic_rpc`` (seed, height x width, min_alt, max_alt) = (100, 37 x 29, -30, 70),
(107, 64 x 96, -32, 73), (114, 1 x 1, -20, 50), (121, 50 x 70, -25, 60); the first three are the training split, the last the test
split.  10,718 pixels at downscale 1; at downscale 2 the 1 x 1 image has an empty grid (``int(1 // 2) = 0``) and adds no ray: 2,663.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_scene_loc_golden.py            # rewrite the fixture
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_scene_loc_golden.py --check    # regenerate in a temporary directory, compare bit for bit

The expected values go to ``expected.npz`` (fixed zip timestamps: the same arrays give the same file bytes) -- not a ``.json``, which
the reference's ``glob`` would read as an image.
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

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "scene_loc")
REF = "/root/reference"
IMAGES = [(100, 37, 29, -30.0, 70.0), (107, 64, 96, -32.0, 73.0), (114, 1, 1, -20.0, 50.0), (121, 50, 70, -25.0, 60.0)]
N_TRAIN = 3
DOWNSCALES = (1.0, 2.0)
FILES = ["train.txt", "test.txt"] + [f"img_{k:02d}.json" for k in range(len(IMAGES))]


def make_scene(root):
    """Write the synthetic dataset under root (deterministic: seeded cameras, JSON floats printed with repr)."""
    sys.path.insert(0, REPO)
    from oracle import rpc_oracle as R

    g = np.random.default_rng(20)
    for k, (seed, h, w, lo, hi) in enumerate(IMAGES):
        rpc = R.synthetic_rpc(seed, height=h, width=w)
        d = {"img": f"img_{k:02d}.tif", "height": h, "width": w, "min_alt": lo, "max_alt": hi,
             "sun_elevation": float(g.uniform(35, 75)), "sun_azimuth": float(g.uniform(100, 220)),
             "rpc": {key: (v.tolist() if isinstance(v, np.ndarray) else float(v)) for key, v in rpc.items()}}
        with open(os.path.join(root, f"img_{k:02d}.json"), "w") as f:
            json.dump(d, f)
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("\n".join(f"img_{k:02d}.json" for k in range(N_TRAIN)))  # no trailing newline: the reference would read it as a file
    with open(os.path.join(root, "test.txt"), "w") as f:
        f.write("\n".join(f"img_{k:02d}.json" for k in range(N_TRAIN, len(IMAGES))))


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


def _has(mod):
    try:
        __import__(mod)
        return True
    except ImportError:
        return False


def run_reference(root):
    """SatelliteDataset.init_scaling_params on root at every downscale -> the dict it hands to write_dict_to_json, plus the extremes
    and sizes of the three vectors it hands to rpc_scaling_params."""
    import torch

    sys.path.insert(0, REPO)
    sys.path.insert(0, REF)
    from oracle import rpc_oracle as R

    class DuckRPC:  # rpcm.RPCModel(d, dict_format="rpcm"): the attributes sat_utils.rescale_rpc touches + localization
        def __init__(self, d, dict_format="rpcm"):
            assert dict_format == "rpcm"
            self.d = dict(d)
            for k in ("row_scale", "col_scale", "row_offset", "col_offset"):
                setattr(self, k, float(d[k]))

        def _dict(self):
            return dict(self.d, row_scale=self.row_scale, col_scale=self.col_scale, row_offset=self.row_offset, col_offset=self.col_offset)

        def localization(self, cols, rows, alts):
            return R.localization(self._dict(), cols, rows, alts)

    rpcm = types.ModuleType("rpcm")
    rpcm.RPCModel = DuckRPC
    stubs = {"rpcm": rpcm}
    for m in ("rasterio", "torchvision", "torchvision.transforms", "kornia") + (() if _has("PIL") else ("PIL", "PIL.Image")):
        stubs[m] = _Stub(m)
    saved = {m: sys.modules.get(m) for m in stubs}
    sys.modules.update(stubs)
    out = {}
    try:
        import datasets.satellite as sat

        torch.set_num_threads(1)
        real_write, real_params = sat.sat_utils.write_dict_to_json, sat.sat_utils.rpc_scaling_params
        for s in DOWNSCALES:
            rec = {"vectors": []}

            def write(d, output_path):
                rec["dict"], rec["path"] = dict(d), output_path
                return d

            def params(v):
                vec = np.array(v).ravel()
                rec["vectors"].append((vec.min(), vec.max(), vec.size, vec.dtype))
                return real_params(v)

            sat.sat_utils.write_dict_to_json, sat.sat_utils.rpc_scaling_params = write, params
            try:
                ds = object.__new__(sat.SatelliteDataset)
                ds.json_dir, ds.img_downscale = root, float(s)
                ds.init_scaling_params()
            finally:
                sat.sat_utils.write_dict_to_json, sat.sat_utils.rpc_scaling_params = real_write, real_params
            d = rec["dict"]
            assert rec["path"] == f"{root}/scene.loc" and len(rec["vectors"]) == 3
            assert all(type(d[a + b]) is np.float32 for a in "XYZ" for b in ("_scale", "_offset")), "the values json.dump refuses"
            assert all(v[3] == np.float32 for v in rec["vectors"])
            tag = f"s{int(s)}"
            out["scale_" + tag] = np.array([d[a + "_scale"] for a in "XYZ"], np.float32)
            out["offset_" + tag] = np.array([d[a + "_offset"] for a in "XYZ"], np.float32)
            out["min_" + tag] = np.array([v[0] for v in rec["vectors"]], np.float32)
            out["max_" + tag] = np.array([v[1] for v in rec["vectors"]], np.float32)
            out["n_points_" + tag] = np.array([v[2] for v in rec["vectors"]], np.int64)  # near + far points = 2 x pixels, per axis
    finally:
        for m, v in saved.items():
            if v is None:
                sys.modules.pop(m, None)
            else:
                sys.modules[m] = v
    return out


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
        assert not os.path.exists(os.path.join(tmp, "scene.loc"))
        blob = npz_bytes(ref)
        if a.check:
            bad = [f for f in FILES if open(os.path.join(tmp, f), "rb").read() != open(os.path.join(OUT, f), "rb").read()]
            z = np.load(os.path.join(OUT, "expected.npz"), allow_pickle=False)
            bad += sorted(set(z.files) ^ set(ref))
            for k in sorted(set(z.files) & set(ref)):
                x, y = np.asarray(ref[k]), z[k]
                if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
                    bad.append(k)
            print(f"scene_loc  {'OK: ' + str(len(FILES)) + ' files and ' + str(len(ref)) + ' arrays bit-equal' if not bad else 'MISMATCH: ' + ', '.join(bad)}")
            return 1 if bad else 0
        os.makedirs(OUT, exist_ok=True)
        for f in FILES:
            with open(os.path.join(tmp, f), "rb") as src, open(os.path.join(OUT, f), "wb") as dst:
                dst.write(src.read())
        with open(os.path.join(OUT, "expected.npz"), "wb") as f:
            f.write(blob)
    extra = sorted(set(os.listdir(OUT)) - set(FILES) - {"expected.npz"})
    assert not extra, f"files without a recipe: {extra}"
    print(f"scene_loc  {len(FILES)} files + expected.npz ({len(blob)} B), pixels " +
          ", ".join(f"{int(ref['n_points_s' + str(int(s))][0]) // 2} at downscale {int(s)}" for s in DOWNSCALES))
    return 0


if __name__ == "__main__":
    sys.exit(main())
