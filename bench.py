#!/usr/bin/env python3
"""Headline benchmark: rays/s of the Sat-NeRF rendering hot path on N MI355X GPUs of one node.

    python bench.py --gpus 1 --steps 200 --warmup 50
    python bench.py --gpus 1 --steps 200 --warmup 50 --full
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Workload = BASELINE.json configs[1]: sat-nerf, fc_units 256, tau 4, 1024 rays x 64 samples PER GPU (weak scaling),
synthetic GPU-resident rays, reference init weights, noise_std 0, sc_lambda 0, single-pass bf16 MFMA.
A step = one pass of the hot path over one ray batch:
  --phase train   : render_rays with grad + SatNerf loss + backward + gradient all-reduce + Adam      (the metric)
  --phase forward : render_rays under no_grad (the batched_inference path)
Prints ONE JSON line (rank 0).  A plain run does what that line's headline needs and no more: set-up, warm-up, the timed steps,
the --dump-outputs arrays when asked for, the line.  `--full` adds everything else the benchmark measures (below: the eager
roofline leg, the sub-records, the CPU baseline, the timed all-reduce of an N > 1 run); --no-extras / --no-cpu-baseline trim it.
Timing discipline: the step is captured into a hipGraph and run PREWARM (50) untimed steps before the `--warmup` steps, so the
line does not depend on the CLI warm-up to reach steady clocks; the timed region is K graph replays bracketed by barrier +
synchronize.  With --full, `roofline` follows SURVEY.md 8(d): the bounding roofline of this path is MFMA, so `achieved` =
algorithmic FLOPs (1,318,912 per point and pass) / the dominant kernel's launch time against the dense bf16 peak, `step_frac` =
the same for the whole step (3 passes: forward, dX, dW); kernel times are HIP events around EAGER launches of the same step
right after the timed region (a graph replay cannot be bracketed per kernel from the host) -- the
rocprofv3 averages of the same command are committed under profiles/; `hbm_gbps` / `traffic` (PMC bytes per launch, read from
the committed profiles/*_train_pmc.csv named in `traffic_source`) are the secondary view.  At N=1 a --full line also carries
`forward` (render_rays under no_grad, the batched_inference path) and `parity_mode` (the same training step in bf16x3 with
16-bit saved state: the arithmetic that meets the 1e-4 output bar) sub-records, and `cpu_baseline` (the CPU oracle, a port of
the reference's PyTorch path, on the host cores for a bounded sample of the same workload).
"""
import argparse
import gc
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOP_PER_POINT = 1318912          # 2 x 659,456 MAC, every Linear layer of SatNeRF(feat 256, tau 4)
MFMA_PEAK_TFLOPS = 2500.0         # dense bf16 MFMA, /opt/skills/guides/MI355X_MICROARCH.md
HBM_PEAK_GBPS = 8000.0            # HBM3E spec, same guide (6.29 TB/s measured achievable)
WS_UNITS = {16: (185, 186), 8: (95, 101)}  # 1-KiB units per 32-point tile: activations saved / gradients written (tau <= 8; csrc/mlp_layout.h)
PREWARM = 50                      # untimed steps before --warmup: graph capture, clocks, caches
KERNEL_NAMES = {"mlp_fwd": "satnerf_fwd2_kernel (one-launch training forward: stratified depths, fused MLP on the generated core saving the 8-bit state, "
                           "compositing + loss + compositing backward)",
                "mlp_bwd": "satnerf_bwd_kernel (fused dX chain, generated trunk)", "wgrad": "wgrad9_kernel (weight-gradient GEMMs)"}
PMC_ROWS = {"mlp_fwd": "satnerf_fwd", "mlp_bwd": "satnerf_bwd_kernel", "wgrad": "wgrad"}
PMC_FILE = os.path.join("profiles", "r06_train_pmc.csv")
MIN_WARM_S = 0.05                 # wall time every leg keeps the device busy before its clock starts (clocks, caches)
DUMP_WARM_ROUNDS = 20             # --dump-outputs: the MIN_WARM_S loop runs this many rounds of 50 steps instead (the step count, hence the inputs of
                                  # the dumped step, must not depend on the build's speed); >= 90 ms of work on MI355X, longer than MIN_WARM_S
DUMP_MAX_BYTES = 64 << 20         # --dump-outputs: larger outputs are written as a fixed, seeded sample of their rows
MAX_CPU_WORKERS = 4               # cpu_baseline's sharded leg: each worker's first backward() starts the HIP runtime (autograd counts the devices
                                  # of every backend), so every worker holds the GPU open beside the bench process: at most 5 such processes


def pmc_counter(kernel_key, counter):
    """per-launch value of `counter` for a kernel from the committed PMC summary (kernel,counter,per_launch_value,launches); None if absent"""
    path = os.path.join(ROOT, PMC_FILE)
    if not os.path.exists(path):
        return None
    for line in open(path):
        if line.startswith("#") or PMC_ROWS[kernel_key] not in line:
            continue
        cols = line.strip().split(",")
        if len(cols) >= 3 and cols[-3] == counter:
            return float(cols[-2])
    return None


def pmc_traffic(kernel_key):
    """HBM bytes per launch of a kernel from the committed PMC summary (2 * FETCH_SIZE + WRITE_SIZE KiB: gfx950 counts a wide
    read at half its bytes, MI355X_MICROARCH.md); None when the file or the rows are missing."""
    fetch, write = pmc_counter(kernel_key, "FETCH_SIZE"), pmc_counter(kernel_key, "WRITE_SIZE")
    return None if fetch is None or write is None else (2.0 * fetch + write) * 1024.0


def pmc_mfma_busy(kernel_key):
    """MFMA-busy fraction of a kernel from the committed PMC summary: SQ_VALU_MFMA_BUSY_CYCLES summed over the chip's 1,024 SIMDs divided
    by 1,024 x the kernel's GPU cycles in the SAME pass (GRBM_GUI_ACTIVE is summed over the 8 XCDs); with the kernel's duration in that
    pass (tools/collect_profiles3.sh records it) -- north_star's "MFMA-busy against CDNA4 peak"."""
    busy, gui, dur = pmc_counter(kernel_key, "SQ_VALU_MFMA_BUSY_CYCLES"), pmc_counter(kernel_key, "GRBM_GUI_ACTIVE"), pmc_counter(kernel_key, "DURATION_US_IN_PMC_PASS")
    if busy is None or gui is None or gui <= 0:
        return None
    return {"frac": busy / 1024.0 / (gui / 8.0), "kernel_us_in_pmc_pass": dur,
            "definition": "SQ_VALU_MFMA_BUSY_CYCLES / 1024 SIMDs / (GRBM_GUI_ACTIVE / 8 XCDs), same rocprofv3 --pmc pass"}


def provenance():
    """What a stale `traffic` figure would be detected by: the git blob id of the committed PMC summary and the build time of the library
    the kernels of this run came from (the PMC file is regenerated with every kernel change; tools/collect_profiles3.sh)."""
    import hashlib

    from satnerf_amd import _lib

    out = {"lib": os.path.relpath(_lib.LIB_PATH, ROOT), "lib_built_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime(os.path.getmtime(_lib.LIB_PATH)))}
    path = os.path.join(ROOT, PMC_FILE)
    if os.path.exists(path):
        data = open(path, "rb").read()
        out["pmc_blob"] = hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest()
        out["pmc_mtime_utc"] = time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime(os.path.getmtime(path)))
    return out


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rays", type=int, default=1024, help="rays per GPU per step")
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--mode", default="bf16", choices=["bf16", "f16", "bf16x3"])
    ap.add_argument("--phase", default=None, choices=["train", "forward"])
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline does not need: the eager roofline leg, the sub-records (N = 1, train), the CPU "
                         "baseline and (N > 1) the timed gradient all-reduce")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the forward / parity_mode sub-records")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: --rays per GPU (the default, what the driver's N = 1, 2, 4, 8 curve measures); strong: --rays in total, rank r takes rays r::N")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the timed path computed in its last timed step (rank 0) as DIR/<name>.npy (float32 / float64, <= 64 MB in all); "
                         "the warm-up then runs a fixed number of steps and (train) the last step starts from the seeded initial weights, so the "
                         "same arguments give the same inputs on every run")
    return ap.parse_args()


def _cpu_pass(phase, n, n_samples):
    """one pass of the oracle over n synthetic rays (forward, or forward + backward of the colour loss)"""
    from oracle import satnerf_oracle as O

    args = O.default_args(n_samples=n_samples)
    rays, ts = O.synthetic_rays(n)
    params = O.procedural_satnerf_params(256, 4, seed=1)
    emb = O.procedural_uniform((30, 4), 1.0, 7)
    if phase == "train":
        for v in params.values():
            v.requires_grad_(True)
        emb.requires_grad_(True)
    target = torch.rand(n, 3)

    def one():
        if phase == "train":
            res = O.render_rays({"coarse": params, "t": emb}, args, rays, ts)
            O.satnerf_loss(res, target).backward()
        else:
            with torch.no_grad():
                O.render_rays({"coarse": params, "t": emb}, args, rays, ts)

    return one


def _cpu_worker(phase, n, n_samples, threads, budget_s):
    """child process of cpu_baseline's sharded leg: passes over its n rays with `threads` intra-op threads for ~budget_s; prints passes, seconds"""
    torch.set_num_threads(threads)
    one = _cpu_pass(phase, n, n_samples)
    one()
    t0, it = time.time(), 0
    while time.time() - t0 < budget_s and it < 200:
        one()
        it += 1
    print(json.dumps({"passes": it, "seconds": time.time() - t0, "rays": n}))


def cpu_baseline(phase, n_rays, n_samples, budget_s=10.0):
    """The oracle (port of the reference's CPU PyTorch path) on this box's host cores, the workload's 1024-ray batch, two ways:
    (a) ONE process, torch's intra-op pool swept over 16 / 32 / 64 threads -- the pool does not scale on these 5120 x 256 operators (r04:
    2.6 rays/s at 256 threads), so the best setting uses 16 of the host's threads;  (b) r06: the batch SHARDED over host_cpus / 16
    processes of 16 threads each (every process renders and back-propagates its slice of the rays, started together) -- all of the host's
    hardware threads at work on one batch (measured: SLOWER than (a), 882 against 2,028 rays/s on a 256-thread host: 64-ray shards are
    too small for 16 threads).  `value` is the better of the two; both are reported.  The fleet is capped at MAX_CPU_WORKERS processes: a
    worker's backward() opens the GPU, so an uncapped fleet put 17 processes on the device of a 256-thread host."""
    import subprocess

    cores = os.cpu_count() or 1
    n = n_rays
    one = _cpu_pass(phase, n, n_samples)
    sweep = {}
    for thr in sorted({min(cores, c) for c in (16, 32, 64)}):
        torch.set_num_threads(thr)
        one()
        t0 = time.time()
        one()
        sweep[thr] = n / (time.time() - t0)
    best_thr = max(sweep, key=sweep.get)
    torch.set_num_threads(best_thr)
    t0, it = time.time(), 0
    while time.time() - t0 < budget_s / 2 and it < 50:
        one()
        it += 1
    single = n / ((time.time() - t0) / it)
    out = {"value": single, "unit": "rays/s", "cores": best_thr, "host_cpus": cores, "kind": "port",
           "sample": f"{it} x {n} rays x {n_samples} samples, {phase}, torch {torch.__version__} CPU fp32",
           "single_process": {"value": single, "threads": best_thr, "sweep_rays_per_s": {str(k): round(v, 1) for k, v in sweep.items()}}}
    # (b) the batch sharded over processes
    per = 16 if cores >= 32 else max(cores // 2, 1)
    procs = max(min(cores // per, n // 8, MAX_CPU_WORKERS), 1)

    def fleet(rays_each, seconds):
        cmd = [sys.executable, os.path.abspath(__file__), "--cpu-worker", phase, str(rays_each), str(n_samples), str(per), str(seconds)]
        env = dict(os.environ, OMP_NUM_THREADS=str(per), MKL_NUM_THREADS=str(per), HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
        t0 = time.time()
        kids = [subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, env=env) for _ in range(procs)]
        rates = []
        for k in kids:
            try:
                txt, _ = k.communicate(timeout=seconds * 6 + 120)
                r = json.loads(txt.strip().splitlines()[-1])
                rates.append(r["rays"] * r["passes"] / r["seconds"])
            except Exception:  # noqa: BLE001  (a baseline leg must not take the bench line down)
                k.kill()
        return (sum(rates), round(time.time() - t0, 1)) if len(rates) == procs else (None, None)

    if procs > 1:
        # (a third leg -- the same fleet with one WHOLE batch per process, data-parallel replicas -- was measured once on the 256-thread host
        #  and dropped: 575 rays/s in all, 73 s of wall time for one timed pass per process; profiles/r06_bench_train.json keeps that record)
        for key, rays_each, what in (("sharded", n // procs, f"each {n // procs} of the batch's {n} rays"),):
            rate, wall = fleet(rays_each, budget_s * 0.6)
            if rate is None:
                continue
            out[key] = {"value": rate, "processes": procs, "threads_per_process": per, "rays_per_process": rays_each, "wall_s": wall}
            if rate > out["value"]:
                out.update(value=rate, cores=procs * per,
                           sample=f"{procs} processes x {per} threads, {what} x {n_samples} samples, {phase}, ~{budget_s * 0.6:.0f} s, "
                                  f"torch {torch.__version__} CPU fp32")
    return out


def measure(phase, mode, n_rays, n_samples, steps, warmup, world, rank, dev, want_kernels=True, bwd_fmt=None, fc_units=None, sc_lambda=0.0,
            ds_lambda=0.0, dump_dir=None):
    """Run one phase in one numeric mode: returns (seconds for `steps` steps on this rank, {kernel: mean ms} from the eager leg).
    `dump_dir`: a fixed-length warm-up, and rank 0 writes the outputs of the last timed step there (dump_outputs)."""
    from satnerf_amd import ops, rendering
    from satnerf_amd import train as train_mod
    from satnerf_amd.data import RayBank, default_args, synthetic_rays  # SURVEY.md 8d recipe; oracle/ is only used by cpu_baseline()
    from satnerf_amd.models import load_model

    args = default_args(n_samples=n_samples, mlp_mode=mode)
    if bwd_fmt is not None:
        args.bwd_fmt = bwd_fmt
    if fc_units is not None:
        args.fc_units = fc_units
    # the two other sat-nerf lines of run_all.sh: solar correction (--sc_lambda 0.1, :56-62) and depth supervision (--ds_lambda 1000, :76-83)
    args.sc_lambda, args.ds_lambda = float(sc_lambda), float(ds_lambda)
    torch.manual_seed(0)  # identical init on every rank
    model = load_model(args).to(dev)
    emb = torch.nn.Embedding(args.t_embbeding_vocab, args.t_embbeding_tau).to(dev)
    models = {"coarse": model, "t": emb}
    # GPU-resident synthetic ray bank (SURVEY.md 8d recipe) + on-device shuffled batch sampler; ranks draw disjoint shares
    n_bank = max(1 << 20, n_rays * 16 * world)  # 1 M rays (47 MB): an epoch is ~1000 steps, as with a real scene
    bank_rays, bank_ts = synthetic_rays(n_bank, seed=20240628)
    bank_rgb = torch.rand(n_bank, 3, generator=torch.Generator().manual_seed(7))
    bank = RayBank(bank_rays.to(dev), bank_rgb.to(dev), bank_ts.to(dev), n_rays, seed=11, rank=rank, world_size=world)
    torch.manual_seed(1234 + rank)  # per-rank sampling jitter

    reset_state = None  # (--dump-outputs, train: run before the last timed step)
    if phase == "train":
        # the reference's schedule is ON (main.py:86-94,128-131): StepLR per epoch and the SNerfLoss warm-up live in the device-side
        # schedule block of the captured step.  The measured steps are those of the main phase: the counter starts after the two
        # warm-up epochs (SatNerfLoss with the uncertainty term, rate decayed twice), an epoch = one pass over the ray bank
        spe = max(n_bank // (n_rays * world), 1)
        stepper = train_mod.Trainer(models, args, world_size=world, steps_per_epoch=spe)
        stepper.n_steps = 2 * spe
        measure.schedule = {"steps_per_epoch": spe, "first_measured_step": stepper.n_steps, "warming_up": bool(stepper.warming_up())}
        if dump_dir:
            # float-atomic gradient reductions make every step differ in its last bits from run to run, and Adam carries that far over a
            # thousand steps: the dumped step starts from the seeded initial weights and zero moments instead (batch, jitter and schedule
            # already follow from the step count), so its inputs are the same on every run and every build
            state0 = [t.clone() for t in (stepper.state.params, stepper.exp_avg, stepper.exp_avg_sq)]

            def reset_state():
                for dst, src in zip((stepper.state.params, stepper.exp_avg, stepper.exp_avg_sq), state0):
                    dst.copy_(src)
                for m in stepper.state.modules:
                    if hasattr(m, "mark_weights_changed"):
                        m.mark_weights_changed()

        depth_bank = None
        if ds_lambda > 0:  # main.py:103-109,134-141: a second shuffled loader of (ray, [target depth, weight]) items, one batch of it per step
            from satnerf_amd.data import DepthBank

            n_dbank = 1 << 18
            d_rays, d_ts = synthetic_rays(n_dbank, seed=20240629)
            gd = torch.Generator().manual_seed(8)
            depths = torch.stack([0.2 + 0.5 * torch.rand(n_dbank, generator=gd), 0.5 + torch.rand(n_dbank, generator=gd)], 1)
            depth_bank = DepthBank(d_rays.to(dev), depths.to(dev), d_ts.to(dev), n_rays, seed=12, rank=rank, world_size=world)

        def step():
            stepper.step_from_bank(bank, depth_bank)
    else:
        # one kernel per step: the render kernel walks this rank's share of the HBM-resident bank chunk by chunk (as
        # eval_satnerf.batched_inference walks an image) and draws the stratified jitter itself (Philox, per-rank seed)
        share = slice(rank, None, world)
        graphed = rendering.GraphedRenderer(models, args, n_rays, dev, seed=1234 + rank, bank=(bank.rays[share], bank.ts[share]))
        use_graph = [True]

        def step():
            if use_graph[0]:
                graphed.replay()  # the next n_rays rows of the bank
            else:
                rays_b, ts_b, _ = bank.next_batch()
                with torch.no_grad():
                    rendering.render_rays(models, args, rays_b, ts_b)

    def fence():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    # nothing of an earlier leg (its graph, its private memory pool, its ray bank) may be released in the middle of the timed
    # region: collect cyclic garbage now -- BEFORE the warm-up, the device must not idle between warm-up and the timed steps --
    # and keep the collector off while the clock runs
    gc.collect()
    gc.disable()
    for _ in range(PREWARM + warmup):
        step()
    fence()
    # ... and keeps the device busy for at least MIN_WARM_S of wall time before the clock starts: after release_leg()'s synchronize +
    # empty_cache the chip has idled and dropped its clocks, and a 4-ms warm-up of 0.09-ms steps timed a cold device (r04's driver-run
    # `forward` read 7.8 M rays/s where the same kernel sustains 12 M)
    t_warm, rounds = time.perf_counter(), 0
    while rounds < DUMP_WARM_ROUNDS if dump_dir else time.perf_counter() - t_warm < MIN_WARM_S:
        for _ in range(50):
            step()
        torch.cuda.synchronize()
        rounds += 1
    measure.warm_s = time.perf_counter() - t_warm
    n_before = PREWARM + warmup + 50 * rounds  # steps before the timed ones
    fence()
    prof = None
    if os.environ.get("BENCH_PROFILE"):  # diagnostic: where the host spends the enqueue time
        import cProfile

        prof = cProfile.Profile()
        prof.enable()
    t0 = time.perf_counter()
    for _ in range(steps - 1 if reset_state else steps):
        step()
    if reset_state:
        reset_state()
        step()
    measure.host_enqueue_s = time.perf_counter() - t0  # host time to enqueue the steps (the device runs behind)
    if prof is not None:
        import pstats

        prof.disable()
        pstats.Stats(prof, stream=sys.stderr).sort_stats("tottime").print_stats(12)
    fence()
    dt = time.perf_counter() - t0
    gc.enable()
    if dump_dir and rank == 0:
        # the last timed step, before the eager leg below steps on: what a caller of the step holds now
        if phase == "train":
            arrays = {"loss": torch.as_tensor(stepper.last_loss.detach()).double().sum(), "rgb": stepper.last_rgb}
            arrays.update({f"param.{key}.{name}": p for key in ("coarse", "t") for name, p in models[key].named_parameters()})
            done = stepper.n_steps - measure.schedule["first_measured_step"]
        else:
            arrays = {k: v for k, v in graphed.out.items() if torch.is_tensor(v) and v.is_floating_point()}
            done = graphed._launches
        assert done == n_before + steps, (done, n_before, steps)
        measure.dumped = dict(dump_outputs(dump_dir, arrays), step=done)
    kernels = {}
    if want_kernels:
        # roofline leg: the same step launched eagerly with HIP events around the hot kernels, same process, same data
        timer = ops.KernelTimer()
        ops.kernel_timer = timer
        if phase == "train":
            stepper.use_graph = False
        else:
            use_graph[0] = False
        for _ in range(min(steps, 30)):
            step()
        torch.cuda.synchronize()
        ops.kernel_timer = None
        kernels = {k: timer.mean_ms(k) for k in ("mlp_fwd", "mlp_bwd", "wgrad") if timer.mean_ms(k)}
    fmt = train_mod._fmt_of(args) if phase == "train" else None
    if phase == "train":
        measure.schedule.update(lr=float(stepper.lr), epoch=int(stepper.current_epoch()))
        measure.collective = {"in_graph": bool(getattr(stepper, "_adam_in_graph", False) and stepper._collective),
                              "capture_failed": bool(getattr(stepper, "_collective_capture_failed", False)),
                              # r06: the N > 1 step = the N = 1 step split at the collective (forward | dX | wgrad | sr_grad_tail, all-reduce,
                              # sr_adam_step_pack: no sr_pack_all, no separate Adam launch)
                              "update_repacks": bool(getattr(stepper, "_pack_in_tail", False))}
    return dt, kernels, fmt


def dump_outputs(out_dir, arrays):
    """Write {name: tensor} as out_dir/<name>.npy in float32 (float64 stays float64).  Past DUMP_MAX_BYTES in all, every array of more
    than one row keeps the same fraction of its rows, chosen by a fixed seed (sorted): the sample depends on the shapes only."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    host = {k: v.detach().cpu().numpy() for k, v in arrays.items() if v is not None}
    host = {k: v.astype(np.float64 if v.dtype == np.float64 else np.float32) for k, v in host.items()}
    total = sum(v.nbytes for v in host.values())
    frac = min(1.0, DUMP_MAX_BYTES / total) if total else 1.0
    sampled = []
    for name, v in sorted(host.items()):
        if frac < 1.0 and v.ndim >= 1 and v.shape[0] > 1:
            keep = max(1, int(v.shape[0] * frac))
            v = v[np.sort(np.random.default_rng(0).choice(v.shape[0], keep, replace=False))]
            sampled.append(name)
        np.save(os.path.join(out_dir, name + ".npy"), v)
        host[name] = v
    return {"dir": out_dir, "files": len(host), "bytes": sum(v.nbytes for v in host.values()), "sampled": sampled}


def release_leg():
    """Free what the previous leg left behind (graph, pools, bank) BEFORE the next leg starts."""
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()


def main():
    a = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}"
    # (before the first device call, i.e. before the HSA runtime starts: RCCL's cross-process buffers need dmabuf IPC on this driver)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # SATNERF_BENCH_BACKEND=gloo is a TEST hook: it lets two ranks share one GPU so the N>1 code path can be exercised on a
    # single-GPU box (gloo stages the all-reduce through the host; never use it for measurements)
    backend = os.environ.get("SATNERF_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist

        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    phase = a.phase or "train"
    if a.scaling == "strong":
        assert a.rays % world == 0, f"--scaling strong: --rays {a.rays} must divide by {world} ranks"
    rays_rank = a.rays // world if a.scaling == "strong" else a.rays
    comm = None
    if world > 1:
        # self-verification of the N > 1 line (nobody but the driver owns a multi-GPU node): every rank contributes a one, so the
        # reduced value is the number of ranks the collective really spanned (whole-job rays/s counts them); --full: then the step's
        # own collective -- one all-reduce of the flat fp32 gradient (662,537 + 120 floats = 2.65 MB) -- timed alone with HIP events
        import torch.distributed as dist

        ones = torch.ones(1, device=dev)
        dist.all_reduce(ones)
        comm = {"rccl_ranks": int(round(ones.item())), "backend": dist.get_backend()}
        if a.full:
            flat = torch.zeros(662537 + 120, device=dev)
            for _ in range(5):
                dist.all_reduce(flat)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                dist.all_reduce(flat)
            e1.record()
            torch.cuda.synchronize()
            comm.update(allreduce_us=e0.elapsed_time(e1) / 20 * 1e3, allreduce_bytes=flat.numel() * 4)
    dt, kernel_ms, fmt = measure(phase, a.mode, rays_rank, a.samples, a.steps, a.warmup, world, rank, dev, want_kernels=a.full,
                                 dump_dir=a.dump_outputs)
    host_enqueue_s = measure.host_enqueue_s
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = t.item()
    if rank != 0:
        return

    ms_step = dt / a.steps * 1e3
    value = rays_rank * world * a.steps / dt
    points = rays_rank * a.samples
    flop = points * FLOP_PER_POINT  # one pass (forward, dX or dW) over the batch
    out = {
        "metric": "training rays/sec (64 samples/ray)" if phase == "train" else "inference rays/sec (64 samples/ray, render_rays no_grad)",
        "value": value, "unit": "rays/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": ms_step,
        "higher_is_better": True, "scaling": a.scaling, "vs_baseline": None, "dtype": {"bf16": "bf16", "f16": "f16", "bf16x3": "bf16x3"}[a.mode],
        "data": "synthetic", "phase": phase, "prewarm_steps": PREWARM, "min_warm_s": MIN_WARM_S,
        "host_enqueue_ms_per_step": host_enqueue_s / a.steps * 1e3,
        "provenance": provenance(),
        # (the driver keeps the first 120 characters: arithmetic and saved-state format come first)
        "config": {"workload": f"BASELINE configs[1] sat-nerf 256/tau4, {rays_rank} rays x {a.samples} samples/GPU, mlp_mode={a.mode}"
                               + (f", saved state {fmt}-bit" if fmt else "") + ", noise_std=0 sc_lambda=0 n_importance=0"
                               + ", stratified jitter drawn in-kernel (Philox-4x32-10)"
                               + (", rays = consecutive chunks of the HBM-resident bank (one kernel per step)" if phase == "forward" else ""),
                   "rays_per_gpu": rays_rank, "global_batch": rays_rank * world,
                   "n_samples": a.samples, "parallelism": f"dp{world}"},
    }
    if a.full:
        # the eager leg's kernel times against the MFMA roofline
        passes = 3 if phase == "train" else 1
        tiles = (points + 31) // 32
        au, du = WS_UNITS.get(fmt, (0, 0))
        ws_bytes = {"mlp_fwd": tiles * au * 1024 if phase == "train" else points * 40, "mlp_bwd": tiles * (au + du) * 1024,
                    "wgrad": tiles * (au + du) * 1024}
        kernels = {k: {"ms": ms, "tflops": flop / (ms * 1e-3) / 1e12, "flop": flop, "workspace_bytes": ws_bytes[k],
                       "workspace_gbps": ws_bytes[k] / (ms * 1e-3) / 1e9} for k, ms in kernel_ms.items()}
        dom = max(kernels, key=lambda k: kernels[k]["ms"])
        traffic = pmc_traffic(dom) if phase == "train" and a.mode == "bf16" and rays_rank == 1024 and a.samples == 64 else None
        busy = {k: pmc_mfma_busy(k) for k in kernels} if phase == "train" and a.mode == "bf16" and rays_rank == 1024 and a.samples == 64 else {}
        out["roofline"] = {"bound": "mfma", "achieved": kernels[dom]["tflops"], "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                           "frac": kernels[dom]["tflops"] / MFMA_PEAK_TFLOPS, "kernel": KERNEL_NAMES[dom], "kernel_ms": kernels[dom]["ms"],
                           "mfma_busy": (busy.get(dom) or {}).get("frac"), "mfma_busy_all": {k: v for k, v in busy.items() if v},
                           "algorithmic_flop_per_launch": flop,
                           "step_achieved": passes * flop / (ms_step * 1e-3) / 1e12, "step_frac": passes * flop / (ms_step * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS,
                           "traffic": traffic, "traffic_source": PMC_FILE if traffic is not None else None,
                           "hbm_gbps": None if traffic is None else traffic / (kernels[dom]["ms"] * 1e-3) / 1e9, "hbm_peak_gbps": HBM_PEAK_GBPS,
                           "timing": "HIP events around eager launches of the same step, right after the timed region", "all_kernels": kernels}
    if a.dump_outputs:
        out["dumped"] = measure.dumped  # (step = the dumped step's index in the leg, counting from 1)
    if phase == "train":
        out["schedule"] = measure.schedule      # StepLR + SNerfLoss warm-up are part of the measured step (main.py:86-94,128-131)
    if comm is not None:
        out["comm"] = dict(comm, **(measure.collective if phase == "train" else {}))
    if a.full and world == 1 and not a.no_extras and phase == "train":
        # driver-timed numbers for the other two claims: the >= 40 % forward kernel and the tolerance-passing arithmetic
        n_sub = max(100, min(a.steps, 200))  # (>= 40 ms windows behind the MIN_WARM_S warm-up)
        n_fwd = 2000  # (0.09-ms steps: a window of 170 ms; a 20-step one would mostly time the fences around it)
        release_leg()
        fdt, fk, _ = measure("forward", a.mode, a.rays, a.samples, n_fwd, 0, 1, 0, dev)
        out["forward"] = {"metric": "inference rays/sec (render_rays no_grad)", "value": a.rays * n_fwd / fdt, "ms_per_step": fdt / n_fwd * 1e3,
                          "steps": n_fwd, "kernel_ms": fk.get("mlp_fwd"),
                          "mlp_tflops": flop / (fk["mlp_fwd"] * 1e-3) / 1e12 if fk.get("mlp_fwd") else None,
                          "mlp_frac_of_mfma_peak": flop / (fk["mlp_fwd"] * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS if fk.get("mlp_fwd") else None}
        if a.mode == "bf16":  # the same forward with fp16 operands (mlp_mode='f16': ~1.3e-4 of the reference instead of ~1.1e-3)
            release_leg()
            hdt, _, _ = measure("forward", "f16", a.rays, a.samples, n_fwd, 0, 1, 0, dev, want_kernels=False)
            out["forward_f16"] = {"metric": "inference rays/sec, mlp_mode=f16 (fp16 MFMA operands, fp32 accumulate)",
                                  "value": a.rays * n_fwd / hdt, "ms_per_step": hdt / n_fwd * 1e3, "steps": n_fwd}
            release_leg()
            tdt, _, tfmt = measure("train", "f16", a.rays, a.samples, n_sub, 0, 1, 0, dev, want_kernels=False)
            out["train_f16"] = {"metric": f"training rays/sec, mlp_mode=f16 (fp16 forward, bf16 backward, saved state {tfmt}-bit)",
                                "value": a.rays * n_sub / tdt, "ms_per_step": tdt / n_sub * 1e3, "steps": n_sub}
            release_leg()
            sdt, _, sfmt = measure("train", "bf16", a.rays, a.samples, n_sub, 0, 1, 0, dev, want_kernels=False, bwd_fmt=16)
            out["train_bf16_state16"] = {"metric": f"training rays/sec, mlp_mode=bf16, saved state {sfmt}-bit (gradients <= 1.4e-2 of the reference)",
                                         "value": a.rays * n_sub / sdt, "ms_per_step": sdt / n_sub * 1e3, "steps": n_sub}
        if a.mode == "bf16":  # the reference's own sat-nerf width (opt.py:50 fc_units = 512; run_all.sh trains with it), same workload
            release_leg()
            wdt, wk, _ = measure("forward", "bf16", a.rays, a.samples, n_fwd, 0, 1, 0, dev, fc_units=512)
            flop512 = 5259264.0 * a.rays * a.samples  # SURVEY.md 8(d) at width 512
            out["forward_width512"] = {"metric": "inference rays/sec at fc_units=512 (render_rays no_grad)", "value": a.rays * n_fwd / wdt,
                                       "ms_per_step": wdt / n_fwd * 1e3, "steps": n_fwd, "kernel_ms": wk.get("mlp_fwd"),
                                       "mlp_frac_of_mfma_peak": flop512 / (wk["mlp_fwd"] * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS if wk.get("mlp_fwd") else None}
            release_leg()
            n512 = max(a.steps // 2, 50)
            vdt, _, vfmt = measure("train", "bf16", a.rays, a.samples, n512, 0, 1, 0, dev, want_kernels=False, fc_units=512)
            out["train_width512"] = {"metric": f"training rays/sec at fc_units=512, mlp_mode=bf16, saved state {vfmt}-bit",
                                     "value": a.rays * n512 / vdt, "ms_per_step": vdt / n512 * 1e3, "steps": n512}
            # ... and the two other configurations run_all.sh trains sat-nerf in, at that width: + solar correction (a second MLP pass
            # along the sun rays, sigma and sun visibility only: forward + dX + dW again) and + depth supervision (a second batch of
            # n rays rendered for depth, sigma gradient only).  passes = MLP passes (forward, dX or dW over one batch) per step
            for key, kw, note in (("train_width512_sc", dict(sc_lambda=0.1), "sc_lambda=0.1 (run_all.sh:56-62)"),
                                  ("train_width512_ds", dict(ds_lambda=1000.0), f"ds_lambda=1000 + {a.rays} depth rays per step (run_all.sh:76-83, main.py:134-141)")):
                release_leg()
                xdt, _, xfmt = measure("train", "bf16", a.rays, a.samples, n512, 0, 1, 0, dev, want_kernels=False, fc_units=512, **kw)
                xms = xdt / n512 * 1e3
                out[key] = {"metric": f"training rays/sec at fc_units=512, {note}, mlp_mode=bf16, saved state {xfmt}-bit",
                            "value": a.rays * n512 / xdt, "ms_per_step": xms, "steps": n512, "mlp_passes_per_step": 6,
                            "algorithmic_flop_per_step": 6 * flop512, "step_frac": 6 * flop512 / (xms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS}
            out["train_width512"].update(mlp_passes_per_step=3, algorithmic_flop_per_step=3 * flop512,
                                         step_frac=3 * flop512 / (out["train_width512"]["ms_per_step"] * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS)
        if a.mode != "bf16x3":
            release_leg()
            qdt, qk, _ = measure("forward", "bf16x3", a.rays, a.samples, n_fwd, 0, 1, 0, dev)
            out["forward_parity"] = {"metric": "inference rays/sec, mlp_mode=bf16x3 (rgb / depth / weights <= 1e-4 of the reference)",
                                     "value": a.rays * n_fwd / qdt, "ms_per_step": qdt / n_fwd * 1e3, "steps": n_fwd, "kernel_ms": qk.get("mlp_fwd")}
            release_leg()
            pdt, pk, pfmt = measure("train", "bf16x3", a.rays, a.samples, n_sub, 0, 1, 0, dev)
            out["parity_mode"] = {"metric": "training rays/sec, mlp_mode=bf16x3 (outputs <= 1e-4 of the reference), saved state "
                                            f"{pfmt}-bit", "value": a.rays * n_sub / pdt, "ms_per_step": pdt / n_sub * 1e3, "steps": n_sub,
                                  "kernel_ms": pk}
            # ... and with parity-grade GRADIENTS as well (bwd_fmt = 32: fp32 saved state, 3-pass GEMMs layer by layer through autograd, eager):
            # what exists today for "gradients <= 2e-4 of the reference's"; a fused kernel for it is not built
            release_leg()
            n_pg = 30
            gdt, _, gfmt = measure("train", "bf16x3", a.rays, a.samples, n_pg, 0, 1, 0, dev, want_kernels=False, bwd_fmt=32)
            out["parity_grade"] = {"metric": "training rays/sec, mlp_mode=bf16x3 with bwd_fmt=32 (outputs <= 1e-4 AND gradients <= 2e-4 of the reference; "
                                             "layer-by-layer path, eager autograd)", "value": a.rays * n_pg / gdt, "ms_per_step": gdt / n_pg * 1e3, "steps": n_pg,
                                   "saved_state_bits": gfmt}
    if a.full and not a.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(phase, a.rays, a.samples)
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--cpu-worker":
        _cpu_worker(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), float(sys.argv[6]))
    else:
        main()
