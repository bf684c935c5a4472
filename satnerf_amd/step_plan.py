"""Launch plan of the training step: which launches make up ``Trainer``'s colour pass, decided in ONE place.  Pure functions of plain
facts (booleans, ints, strings) and a mapping of environment switches -- no torch, no library, never a ``Trainer`` -- so that the plan
can be tabulated and checked without a GPU (tests/test_step_plan_host.py)."""
# Every switch of the step is read here and nowhere else in train.py, at the moment a function is called (``capture_state`` at capture,
# ``launches`` wherever the step takes a decision):
#   SATNERF_FORCE_ALLREDUCE=1   a 1-rank process group issues the gradient all-reduce too                      (collective)
#   SATNERF_TRAIN_FUSED=0       the r04 three-launch training forward (sr_ray_setup, MLP, sr_render_loss)      (fused_forward)
#   SATNERF_FWD_V1=1            the hipcc-scheduled forward kernels: they have no one-launch training forward  (fused_forward)
#   SATNERF_GRAPH_ALLREDUCE=1   capture the RCCL all-reduce and the update into the step's graph               (capture_state)
#   SATNERF_TAIL_PACK=0         sr_pack_all opens the step instead of the update launch re-packing the streams (capture_state)
#   SATNERF_DP_PACK=0           the same for steps with a collective only: the r05 N > 1 step                  (capture_state)
#   SATNERF_TAIL_ADAM=0         sr_grad_tail + sr_adam_step_graph instead of sr_grad_tail_adam                 (capture_state, launches)
#   SATNERF_GATHER_IN_FWD=0     sr_gather_batch in front of the forward instead of the forward's own gather    (launches)
#   SATNERF_GRAPH_SAMPLER=0|1   whether a captured step samples its batches itself                             (launches)
from __future__ import annotations

import os
from collections import namedtuple


def _on(env, name):  # a default-on A/B switch: only "0" turns it off
    return env.get(name, "1") != "0"


# the gradient all-reduce runs when there is more than one rank -- or, with SATNERF_FORCE_ALLREDUCE=1, also on a 1-rank process group
# (how a single-GPU box exercises the captured RCCL path)
def collective(world_size, pg_initialised, env=os.environ):
    return world_size > 1 or (env.get("SATNERF_FORCE_ALLREDUCE", "0") == "1" and pg_initialised)


def fused_forward(fmt, n_samples, render_fused_ok, env=os.environ):
    """True when the colour pass's forward is ONE launch (sr_satnerf_render_train): 8-bit saved state, <= 64 samples dividing a
    workgroup's points and a generated-core build for (width, mode) -- ``render_fused_ok`` = ops.render_fused_ok(feat, mode, n_samples)."""
    return bool(fmt == 8 and n_samples <= 64 and render_fused_ok and _on(env, "SATNERF_TRAIN_FUSED") and env.get("SATNERF_FWD_V1", "0") != "1")


# What a capture decides; ``Trainer`` keeps three of them as ``_kernel_rng``, ``_adam_in_graph`` and ``_pack_in_tail``:
#   kernel_rng          the kernels draw the stratified jitter themselves (Philox keyed by the seed and the device step counter)
#   capture_collective  the all-reduce is captured into the step's graph
#   adam_in_graph       the update is part of the captured pass, not issued after the replay
#   pack_in_tail        the update launch re-packs the weight streams and the forward opens the step: no sr_pack_all
CaptureState = namedtuple("CaptureState", "kernel_rng capture_collective adam_in_graph pack_in_tail")


def capture_state(*, noise_zero, collective, pg_initialised, backend, capture_failed, late_idx, fused_forward, env=os.environ):
    """``pg_initialised`` / ``backend``: torch.distributed's process group and its backend name (None without one); ``capture_failed``: an
    earlier capture of the collective failed on some rank; ``late_idx``: the trainer has the index of the parameters whose gradients
    arrive by float atomics (sr_grad_tail_adam needs it); ``collective`` / ``fused_forward``: what the functions above return."""
    # data parallel: with the RCCL backend ("nccl") the gradient all-reduce and the Adam update CAN be captured into the step's graph
    # (NCCL / RCCL collectives are capturable): a step is then one replay, no eager launches between steps.  It is OPT-IN
    # (SATNERF_GRAPH_ALLREDUCE=1) until a job with two or more GPUs has run it: so far it has only executed on a 1-rank group
    # (tests/test_hip_training.py), and a collective that misbehaves inside a replayed graph hangs the job instead of raising
    # (ADVICE r03).  Default, other backends (gloo cannot be captured), or a capture that fails on any rank: the eager all-reduce +
    # Adam issued after the replay.
    capture_collective = bool(collective and env.get("SATNERF_GRAPH_ALLREDUCE", "0") == "1" and pg_initialised and backend == "nccl"
                              and not capture_failed)
    kernel_rng = bool(noise_zero)  # (a noisy step still draws randn from torch's generator)
    # the launch that updates the parameters re-packs the weight streams and the forward opens the step (no sr_pack_all launch): on a
    # single GPU that launch is the gradient tail (sr_grad_tail_adam), with a collective it is sr_adam_step_pack behind the all-reduce
    # (in the graph when the collective is captured, eagerly after the replay otherwise).  SATNERF_DP_PACK=0: the r05 N > 1 step (A/B)
    pack_in_tail = bool(late_idx and kernel_rng and fused_forward and _on(env, "SATNERF_TAIL_ADAM") and _on(env, "SATNERF_TAIL_PACK")
                        and (not collective or _on(env, "SATNERF_DP_PACK")))
    return CaptureState(kernel_rng, capture_collective, (not collective) or capture_collective, pack_in_tail)


# The colour pass of one step under the current state:
#   fused_forward        the forward is ONE launch (sr_satnerf_render_train), not sr_ray_setup + MLP + sr_render_loss
#   tick                 2: the forward opens the step (advances the step counter and draws for the advanced value); 0: it does not
#   pack_first           sr_pack_all (model.repack) opens the pass: "ticks" (it advances the step counter) | "quiet"; False: no sr_pack_all
#   sampler              a captured step's colour batch: "forward" (sampled by the forward launch), "setup" (sr_gather_setup: gather +
#                        depths + sky colour), "gather" (sr_gather_batch); None without a bank
#   graph_sampler        step_from_bank lets the captured step sample for itself (SATNERF_GRAPH_SAMPLER; default: sampler in forward)
#   tail                 "tail_adam" (sr_grad_tail_adam: reduction + Adam [+ re-pack] in one launch) | "tail" (sr_grad_tail)
#   update               behind a "tail": "adam_graph" (sr_adam_step_graph) | "adam_pack" (sr_adam_step_pack), both inside the pass when
#                        adam_in_graph, else "adam_pack" | "adam_eager" (sr_adam_step, host-side step count and rate), issued by step()
#                        behind the pass / the replay and the eager all-reduce; "none" behind "tail_adam"
#   update_after_replay  [all-reduce +] update are issued by step() behind the pass / the replay, not inside it (= not adam_in_graph)
#   names                the kernel-launching C-ABI entry points in issue order, "all_reduce" where the collective sits; the sampler's
#                        launch only when the captured step samples for itself (graph_sampler)
Launches = namedtuple("Launches", "fused_forward tick pack_first sampler graph_sampler tail update update_after_replay names")


def launches(*, collective, fmt, n_samples, render_fused_ok, kernel_rng=False, adam_in_graph=False, pack_in_tail=False, snerf=False, bank=False,
             ray_bank=False, late_idx=True, deterministic=False, env=os.environ):
    """The three state flags are ``Trainer``'s (a capture's ``CaptureState``, or what a caller assigned by hand; none before a capture);
    ``bank``: the colour batch comes from a ray bank, ``ray_bank``: that bank is a ``RayBank`` (the forward launch can read its rows);
    ``deterministic`` (``Trainer(deterministic=True)``, not an environment switch): the tail launch is its fixed-order twin -- ``names``
    carries sr_grad_tail_det / sr_grad_tail_adam_det, every other field is what it is without it."""
    fused = fused_forward(fmt, n_samples, render_fused_ok, env)
    ticking = bool(kernel_rng or adam_in_graph)
    # r05, single-GPU captured step: no sr_pack_all launch -- the launch that updates the parameters (sr_grad_tail_adam) also writes
    # them into the weight streams, and the forward, now the step's first launch, ticks the step counter itself ("tick first")
    pit = bool(pack_in_tail and ticking)
    tail_adam = bool(adam_in_graph and not collective and late_idx and _on(env, "SATNERF_TAIL_ADAM"))
    # two combinations no capture produces (tests/test_step_plan_host.py walks every capture): pack_in_tail is only set with the fused
    # forward available, and without a collective only with sr_grad_tail_adam as the tail.  They take flags assigned by hand or a
    # switch flipped between a capture and a later eager pass -- checks of a developer's mistake, which ``python -O`` drops
    assert fused or not pit, "pack-in-tail steps need the one-launch training forward (it ticks the step counter)"
    assert tail_adam or collective or not pit, "single-GPU pack-in-tail steps end in sr_grad_tail_adam"
    # the colour batch of a captured step: sampled INSIDE the forward launch (sr_satnerf_render_train's gather over the bank's shuffled
    # rows); or gather + stratified depths + sky colour in ONE launch (sr_gather_setup) when the forward is not the one-launch render,
    # which sets the rays up itself; or a plain sr_gather_batch
    in_forward = bool(fused and not snerf and ray_bank and _on(env, "SATNERF_GATHER_IN_FWD"))
    sampler = None if not bank else "forward" if kernel_rng and in_forward else "setup" if kernel_rng and not fused else "gather"
    # ON by default when the forward launch can do the sampling itself; otherwise opt-in (SATNERF_GRAPH_SAMPLER=1) -- as separate gather
    # launches in the graph it is exactly as fast as the eager gather in front of the replay (r02: 0.420-0.425 ms either way)
    graph_sampler = env.get("SATNERF_GRAPH_SAMPLER", "1" if in_forward else "0") == "1"
    # the update rides in the same graph (the RCCL all-reduce captured with it, or SATNERF_TAIL_ADAM=0), or step() issues it behind the
    # (eager) all-reduce
    in_graph, behind = "adam_pack" if pit else "adam_graph", "adam_pack" if pack_in_tail else "adam_eager"
    update = "none" if tail_adam else in_graph if adam_in_graph else behind
    launched = graph_sampler and {"setup": "sr_gather_setup", "gather": "sr_gather_batch"}.get(sampler)
    names = ([launched] if launched else []) + ([] if pit else ["sr_pack_all"])
    if fused:
        names.append("sr_satnerf_render_train")
    else:
        names += ([] if launched == "sr_gather_setup" else ["sr_ray_setup_rng" if kernel_rng else "sr_ray_setup"]) + ["sr_satnerf_mlp_fwd"]
        names += ["sr_render_loss"] if n_samples <= 64 else ["sr_composite_fwd", "sr_satnerf_loss", "sr_composite_bwd"]
    # data parallel (r06): the N > 1 step is the N = 1 step split at the collective -- sr_grad_tail (the reduction) | all-reduce of the flat
    # gradient | sr_adam_step_pack (Adam + the re-pack of the weight streams): no sr_pack_all, no separate Adam launch
    names += ["sr_satnerf_mlp_bwd", "sr_satnerf_wgrad8" if fmt == 8 else "sr_satnerf_wgrad", ("sr_grad_tail_adam" if tail_adam else "sr_grad_tail") + ("_det" if deterministic else "")]
    if not tail_adam:
        names += (["all_reduce"] if collective else []) + ["sr_adam_step" + {"adam_graph": "_graph", "adam_pack": "_pack", "adam_eager": ""}[update]]
    return Launches(fused, 2 if pit else 0, False if pit else "ticks" if ticking else "quiet", sampler, graph_sampler,
                    "tail_adam" if tail_adam else "tail", update, not adam_in_graph, tuple(names))
