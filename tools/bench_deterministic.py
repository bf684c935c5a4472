"""What deterministic training steps cost (Trainer(deterministic=True): sr_grad_tail_adam_det in place of sr_grad_tail_adam), on HIP events:

1. the tail launch stand-alone, on the arguments of a real captured step (recorded once, as tools/ab_tail.py does): sr_grad_tail_adam beside
   sr_grad_tail_adam_det, back to back, the two interleaved round by round on the same box;
2. the replayed 1024 x 64 step of two trainers (bench.py's shape) with and without ``deterministic=True``, interleaved likewise.

Prints one JSON line.  AB_RAYS / AB_WIDTH change the batch and the width."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from satnerf_amd import data, ops  # noqa: E402
from satnerf_amd.models import load_model  # noqa: E402
from satnerf_amd.train import Trainer  # noqa: E402

dev = "cuda:0"
n = int(os.environ.get("AB_RAYS", "1024"))
ROUNDS, LAUNCHES, STEPS = 7, 200, 300


def trainer(deterministic):
    args = data.default_args(mlp_mode="bf16")
    if os.environ.get("AB_WIDTH"):
        args.fc_units = int(os.environ["AB_WIDTH"])
    torch.manual_seed(0)
    models = {"coarse": load_model(args).to(dev), "t": torch.nn.Embedding(30, 4).to(dev)}
    return Trainer(models, args, use_graph=True, steps_per_epoch=1000, deterministic=deterministic)


def timed(fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / count * 1e3  # us


def interleaved(fns, count):
    """Per variant: (best, median) us over ROUNDS rounds, the variants alternating within each round."""
    for fn in fns.values():
        timed(fn, 20)
    t = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            t[name].append(timed(fn, count))
    return {name: (round(min(v), 2), round(sorted(v)[len(v) // 2], 2)) for name, v in t.items()}


rays, ts = data.synthetic_rays(n)
rays, ts, tgt = rays.to(dev), ts.to(dev), torch.rand(n, 3, device=dev)

# 1. the tail launch, stand-alone
tr = trainer(False)
seen = {}
real = ops.grad_tail_adam


def spy(*a, **k):
    seen["a"], seen["k"] = a, k
    return real(*a, **k)


ops.grad_tail_adam = spy
for _ in range(3):
    tr.step(rays, ts, tgt, validate=False)
torch.cuda.synchronize()
ops.grad_tail_adam = real
a, k = seen["a"], seen["k"]
scratch = ops.late_grad_scratch(n, a[6].shape[0], a[19], dev)
tail = interleaved({"sr_grad_tail_adam": lambda: real(*a, **k), "sr_grad_tail_adam_det": lambda: ops.grad_tail_adam_det(*a, scratch, **k)}, LAUNCHES)

# 2. the replayed step
trainers = {"default": tr, "deterministic": trainer(True)}
step = interleaved({name: (lambda t=t: t.step(rays, ts, tgt, validate=False)) for name, t in trainers.items()}, STEPS)
assert trainers["deterministic"]._graph is not None and "sr_grad_tail_adam_det" in trainers["deterministic"]._plan().names
print(json.dumps({"rays": n, "width": tr.models["coarse"].feat, "tail_us_best_median": tail, "step_us_best_median": step,
                  "rounds": ROUNDS, "launches_per_round": LAUNCHES, "steps_per_round": STEPS}))
