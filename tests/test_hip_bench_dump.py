"""bench.py --dump-outputs: the arrays of the last timed step, written after the timed region, with inputs that do not depend on the run
(a fixed-length warm-up; the dumped training step starts from the seeded initial weights): two runs with the same arguments dump the
same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _bench(out_dir, *extra):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2", "--no-extras", "--no-cpu-baseline",
                        "--dump-outputs", str(out_dir), *extra], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    files = sorted(os.listdir(out_dir))
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in files}
    assert all(f.endswith(".npy") for f in files) and d["dumped"]["files"] == len(files)
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in arrays.values())
    assert sum(v.nbytes for v in arrays.values()) <= 64 << 20 and d["steps"] == 3
    # the dumped step is the last timed one: prewarm + --warmup + the fixed warm-up + --steps steps into the leg
    assert d["dumped"]["step"] == bench.PREWARM + 2 + 50 * bench.DUMP_WARM_ROUNDS + 3
    return d, arrays


@pytest.mark.gpu
def test_train_dump_holds_the_loss_colours_and_every_updated_parameter(tmp_path):
    d, a = _bench(tmp_path / "train")
    assert d["phase"] == "train" and a["loss"].shape == () and a["loss"] > 0 and a["rgb"].shape == (1024, 3)
    params = [k for k in a if k.startswith("param.")]
    assert len(params) == 41 and a["param.t.weight"].shape == (30, 4) and a["param.coarse.fc_net.8.weight"].shape == (256, 259)
    assert sum(a[k].size for k in params) == 662537 + 120


@pytest.mark.gpu
def test_train_dump_is_the_same_on_every_run(tmp_path):
    # the dumped step starts from the seeded initial weights: only the float-atomic reductions of that one step may differ
    _, a = _bench(tmp_path / "a")
    _, b = _bench(tmp_path / "b")
    assert set(a) == set(b) and a["loss"] == b["loss"] and np.array_equal(a["rgb"], b["rgb"])
    for k in a:
        assert np.abs(a[k] - b[k]).max() <= 1e-6 * max(np.abs(a[k]).max(), 1e-30), k


@pytest.mark.gpu
def test_forward_dump_is_the_same_on_every_run(tmp_path):
    d, a = _bench(tmp_path / "a", "--phase", "forward")
    _, b = _bench(tmp_path / "b", "--phase", "forward")
    assert d["phase"] == "forward" and {"rgb_coarse", "depth_coarse", "weights_coarse"} <= set(a) and a["rgb_coarse"].shape == (1024, 3)
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_allclose(a[k], b[k], rtol=1e-6, atol=1e-7, err_msg=k)
