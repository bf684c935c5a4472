"""bench.py's two kinds of line at N = 1: a plain run prints the headline (set-up, warm-up, timed steps, the line) and nothing that takes
a run of its own; --full adds the eager roofline leg (here without the sub-records and the CPU baseline, which --full also runs)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("roofline", "forward", "forward_f16", "train_f16", "train_bf16_state16", "forward_width512", "train_width512",
             "train_width512_sc", "train_width512_ds", "forward_parity", "parity_mode", "parity_grade", "cpu_baseline")


def _bench(*extra):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2", *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_line_is_the_headline_only():
    d = _bench()
    assert d["metric"] == "training rays/sec (64 samples/ray)" and d["unit"] == "rays/s" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and d["steps"] == 5 and d["warmup"] == 2 and d["n_gpus"] == 1 and d["phase"] == "train"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 1024 * 5 / (d["ms_per_step"] * 5e-3)) < 1e-3 * d["value"]
    assert d["schedule"]["warming_up"] is False and "comm" not in d
    assert not set(FULL_ONLY) & set(d), sorted(set(FULL_ONLY) & set(d))


@pytest.mark.gpu
def test_full_line_adds_the_eager_roofline_leg():
    d = _bench("--full", "--no-extras", "--no-cpu-baseline")
    assert d["unit"] == "rays/s" and d["steps"] == 5 and d["ms_per_step"] > 0
    roof = d["roofline"]
    assert roof["bound"] == "mfma" and 0 < roof["frac"] < 1 and 0 < roof["step_frac"] < 1
    assert set(roof["all_kernels"]) == {"mlp_fwd", "mlp_bwd", "wgrad"} and roof["traffic_source"] == "profiles/r06_train_pmc.csv"
    assert not (set(FULL_ONLY) - {"roofline"}) & set(d)
