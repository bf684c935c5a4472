"""The kernels behind the A/B switches stay correct: SATNERF_FWD_V1=1 (the hipcc-scheduled forward kernels of mlp_fwd.inc instead of the
generated cores -- also the fallback when a workspace exceeds the generated streams' 32-bit offsets), r06: SATNERF_WGRAD_THIN=0 /
SATNERF_WGRAD_NORAW=0.  The switches are read once per process, so each case runs the relevant reference-golden
tests in a child interpreter with the variable set."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(env_extra, test_file, keyword):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", test_file), "-q", "-x", "-m", "gpu", "-k", keyword, "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "no tests ran" not in r.stdout, r.stdout[-500:]


@pytest.mark.gpu
def test_hipcc_scheduled_forward_kernels_match_the_goldens():
    # parity mode, throughput mode, f16, width 512, one-launch render: all through launch_fwd<...> of mlp_fwd.inc
    _run({"SATNERF_FWD_V1": "1"}, "test_hip_parity.py",
         "mlp_forward_points_golden or render_rays_golden_parity_mode or f16_mode_matches or width_512_fused or one_launch_render")


@pytest.mark.gpu
def test_hipcc_scheduled_training_forward_matches_the_gradient_goldens():
    _run({"SATNERF_FWD_V1": "1"}, "test_hip_backward.py", "gradients_match_reference_golden")


@pytest.mark.gpu
def test_full_streams_for_the_one_row_blocks_match_the_gradient_goldens():
    """r06 A/B switches of the 4-wave weight-gradient kernel: SATNERF_WGRAD_THIN=0 (the head blocks on the full stream with equal slices, as
    r05 ran them) and SATNERF_WGRAD_NORAW=0 (every full-stream wave runs its raw duty, dump or not): the paths the defaults replaced stay
    correct -- the reference's gradient goldens and the benched-shape gates through each."""
    _run({"SATNERF_WGRAD_THIN": "0"}, "test_hip_backward.py", "gradients_match_reference_golden or direct_step_matches_autograd")
    _run({"SATNERF_WGRAD_NORAW": "0"}, "test_hip_backward.py", "gradients_match_reference_golden")
    _run({"SATNERF_WGRAD_THIN": "0", "SATNERF_WGRAD_NORAW": "0"}, "test_hip_benched_shape.py", "bf16-256 or bf16-512")


@pytest.mark.gpu
def test_bench_contract_with_two_ranks_sharing_the_gpu():
    """bench.py's N > 1 path (per-rank bank shares, barrier + max over ranks, whole-job rays/s) launched as the driver launches it; the two
    ranks share the one GPU through the gloo test hook (measurements use nccl = RCCL, one rank per GPU).  The weak-scaling run is a --full
    one (roofline leg, timed all-reduce), the strong-scaling run a plain one (the headline only)."""
    import json

    env = dict(os.environ, SATNERF_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29533", "bench.py", "--gpus", "2", "--steps", "5", "--warmup", "2", "--full", "--no-cpu-baseline"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 5 and d["scaling"] == "weak" and d["config"]["parallelism"] == "dp2"
    assert abs(d["value"] - 2 * 1024 * 5 / (d["ms_per_step"] * 5e-3)) < 1e-3 * d["value"]  # whole-job rays/s = all ranks' rays / max-over-ranks time
    assert d["roofline"]["bound"] == "mfma" and 0 < d["roofline"]["frac"] < 1
    # the N > 1 line verifies itself: the ones all-reduce counted both ranks, the 2.65 MB gradient all-reduce was timed alone, and the line
    # says whether the collective rode inside the step's graph (gloo cannot be captured: eager here) or a capture failed
    c = d["comm"]
    assert c["rccl_ranks"] == 2 and c["backend"] == "gloo" and c["allreduce_us"] > 0 and c["allreduce_bytes"] == (662537 + 120) * 4
    assert c["in_graph"] is False and c["capture_failed"] is False
    assert c["update_repacks"] is True  # r06: the N > 1 step is the N = 1 step split at the collective (no sr_pack_all, one update launch)
    assert d["schedule"]["steps_per_epoch"] >= 1 and d["schedule"]["warming_up"] is False and d["schedule"]["epoch"] >= 2
    assert d["provenance"]["lib"].endswith("libsatrender.so") and d["config"]["global_batch"] == 2048
    # strong scaling: the same global batch split over the ranks; a plain line: the rank count, no roofline, no timed all-reduce
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29534", "bench.py", "--gpus", "2", "--steps", "5", "--warmup", "2", "--no-cpu-baseline", "--scaling", "strong"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert d["scaling"] == "strong" and d["config"]["rays_per_gpu"] == 512 and d["config"]["global_batch"] == 1024
    assert d["comm"]["rccl_ranks"] == 2 and "allreduce_us" not in d["comm"] and "roofline" not in d and "cpu_baseline" not in d
    assert abs(d["value"] - 1024 * 5 / (d["ms_per_step"] * 5e-3)) < 1e-3 * d["value"]
