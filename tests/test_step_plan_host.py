"""satnerf_amd/step_plan.py against the conditions it replaced, without a GPU.

The oracle is TEXT: the boolean expressions of ``Trainer`` as they stood in satnerf_amd/train.py before the plan existed (commit c9f48fa,
"Test the training forward against an fp64 chain of the inputs it reads"), copied literally with ``self.``'s attributes as local names
and ``os.environ`` as ``env``; every one cites its line there as ``# L<n>``.  The expected launch names follow from walking those
conditions in the order the old code issued its calls, each ``ops`` function standing for the entry point it launches (ops.py).  Then the
invariants the old code guarded with two RuntimeErrors, over every state a capture can produce; then the launch sequences README.md,
DESIGN.md and INTEGRATION.md advertise, written out by hand."""
import itertools

import pytest

from satnerf_amd import step_plan

B = (False, True)
SWITCH = (None, "0", "1")  # unset, and the two values every switch is compared with


def envs(*names):
    for values in itertools.product(SWITCH, repeat=len(names)):
        yield {k: v for k, v in zip(names, values) if v is not None}


# ---- the old text ----------------------------------------------------------------------------------------------------------------------
def old_fused_forward(fmt, s, render_fused_ok, env):
    return (fmt == 8 and s <= 64 and render_fused_ok                                                                              # L370
            and env.get("SATNERF_TRAIN_FUSED", "1") != "0" and env.get("SATNERF_FWD_V1", "0") != "1")                              # L371


def old_capture(noise_std, _collective, is_initialized, backend, _collective_capture_failed, _late_idx, _fused_forward, env):
    """Trainer._capture L568-577 -> (_kernel_rng, capture_collective, _adam_in_graph, _pack_in_tail); ``_fused_forward``: a callable"""
    capture_collective = (_collective and env.get("SATNERF_GRAPH_ALLREDUCE", "0") == "1" and is_initialized                       # L568
                          and backend == "nccl" and not _collective_capture_failed)                                                # L569
    _adam_in_graph = (not _collective) or capture_collective                                                                       # L570
    _kernel_rng = float(noise_std) == 0.0                                                                                          # L571
    _pack_in_tail = (_late_idx is not None and _kernel_rng and _fused_forward()                                                    # L575
                     and env.get("SATNERF_TAIL_ADAM", "1") != "0" and env.get("SATNERF_TAIL_PACK", "1") != "0"                     # L576
                     and (not _collective or env.get("SATNERF_DP_PACK", "1") != "0"))                                              # L577
    return bool(_kernel_rng), bool(capture_collective), bool(_adam_in_graph), bool(_pack_in_tail)


def old_step(_kernel_rng, _adam_in_graph, _pack_in_tail, _collective, fmt, s, render_fused_ok, _snerf, bank, _late_idx, env):
    """What step_from_bank (bank: "RayBank", another bank class's name, or None: step) -> [_capture's run() ->] _gather_from_banks ->
    _forward_backward -> the end of step did, as a dict of the plan's fields; or the message of the RuntimeError it raised.  The conjuncts
    of L681 that are not the plan's business (direct, use_graph, noise_std == 0, drop_last) are taken as true."""
    _fused_forward = lambda: old_fused_forward(fmt, s, render_fused_ok, env)  # noqa: E731
    names, sampler, _pre_setup, _gather_in_fwd = [], None, None, None
    _sampler_in_forward = (_fused_forward() and not _snerf and bank == "RayBank"                                                   # L668
                           and env.get("SATNERF_GATHER_IN_FWD", "1") != "0")                                                       # L669
    graph_sampler = env.get("SATNERF_GRAPH_SAMPLER", "1" if _sampler_in_forward else "0") == "1"                                   # L682
    if bank is not None:  # _gather_from_banks, k == 0; it runs inside the captured step when step_from_bank took the L681 branch
        if (_kernel_rng and _fused_forward() and not _snerf and bank == "RayBank"                                                  # L540
                and env.get("SATNERF_GATHER_IN_FWD", "1") != "0"):                                                                 # L541
            sampler, _gather_in_fwd = "forward", True                                                                              # L543
        elif _kernel_rng and not _fused_forward():                                                                                 # L544
            sampler, _pre_setup = "setup", True                                                                                    # L553-555
        else:
            sampler = "gather"                                                                                                     # L557
        if not graph_sampler:  # the graph was captured by step(): no _gather_from_banks in it (L582: _graph_banks is None)
            _pre_setup = _gather_in_fwd = None
        else:
            names += {"setup": ["sr_gather_setup"], "gather": ["sr_gather_batch"], "forward": []}[sampler]
    ticking = _kernel_rng or _adam_in_graph                                                                                        # L264
    pit = _pack_in_tail and ticking                                                                                                # L267
    if not pit:                                                                                                                    # L268
        names.append("sr_pack_all")                                                                                                # L271
    pack_first = False if pit else "ticks" if ticking else "quiet"            # L268, L271: tick=self.adam_state if ticking else None
    fused = _pre_setup is None and _fused_forward()                                                                                # L287
    if pit and not fused:                                                                                                          # L289
        return "pack-in-tail steps need the one-launch training forward (it ticks the step counter)"                               # L290
    if fused:                                                                                                                      # L291
        names.append("sr_satnerf_render_train")                                                                                    # L295
    else:
        if _pre_setup is None:                                                                                                     # L304
            names.append("sr_ray_setup_rng" if _kernel_rng else "sr_ray_setup")                              # L277, L307, ops.py L685-691
        names.append("sr_satnerf_mlp_fwd")                                                                                         # L309
        if s <= 64:                                                                                                                # L311
            names.append("sr_render_loss")                                                                                         # L312
        else:
            names += ["sr_composite_fwd", "sr_satnerf_loss", "sr_composite_bwd"]                                                   # L316-318
    names += ["sr_satnerf_mlp_bwd", "sr_satnerf_wgrad8" if int(fmt) == 8 else "sr_satnerf_wgrad"]                    # L321-322, ops.py L602
    out = dict(fused_forward=bool(fused), tick=2 if pit else 0, pack_first=pack_first, sampler=sampler,        # L297
               graph_sampler=graph_sampler)
    if _adam_in_graph and not _collective and _late_idx is not None and env.get("SATNERF_TAIL_ADAM", "1") != "0":                  # L334
        return dict(out, tail="tail_adam", update="none", update_after_replay=False, names=tuple(names + ["sr_grad_tail_adam"]))   # L336
    if pit and not _collective:                                                                                                    # L339
        return "single-GPU pack-in-tail steps end in sr_grad_tail_adam"                                                            # L340
    names.append("sr_grad_tail")                                                                                                   # L343
    if _adam_in_graph:                                                                                                             # L344
        if _collective:                                                                                                            # L345
            names.append("all_reduce")                                                                                             # L346
        update = "adam_pack" if pit else "adam_graph"                                                                              # L347-350
    # ... back in step(), behind the pass or the replay
    if _collective and not _adam_in_graph:                                                                                         # L747
        names.append("all_reduce")                                                                                                 # L748
    if not _adam_in_graph:                                                       # L750 (in_graph, L746, implies _adam_in_graph: one test)
        update = "adam_pack" if _pack_in_tail else "adam_eager"                                                                    # L751-754
    names.append({"adam_graph": "sr_adam_step_graph", "adam_pack": "sr_adam_step_pack", "adam_eager": "sr_adam_step"}[update])
    return dict(out, tail="tail", update=update, update_after_replay=not _adam_in_graph, names=tuple(names))


# ---- the tables ------------------------------------------------------------------------------------------------------------------------
# (process group, backend) pairs: a backend name exists only with an initialised process group (dist.get_backend raises without one)
GROUPS = ((False, None), (True, "gloo"), (True, "nccl"))


def test_collective_is_the_old_condition():
    for world, pg in itertools.product((1, 2), B):
        for env in envs("SATNERF_FORCE_ALLREDUCE"):
            is_available = is_initialized = pg
            old = world > 1 or (env.get("SATNERF_FORCE_ALLREDUCE", "0") == "1" and is_available and is_initialized)               # L200
            assert step_plan.collective(world, pg, env) == old, (world, pg, env)


def test_fused_forward_is_the_old_condition():
    for fmt, s, ok in itertools.product((8, 16, 32), (64, 65), B):
        for env in envs("SATNERF_TRAIN_FUSED", "SATNERF_FWD_V1"):
            assert step_plan.fused_forward(fmt, s, ok, env) == old_fused_forward(fmt, s, ok, env), (fmt, s, ok, env)


def test_capture_state_is_the_old_conditions_on_every_row():
    rows = 0
    for noise_zero, coll, (pg, backend), failed, late, fused in itertools.product(B, B, GROUPS, B, B, B):
        for env in envs("SATNERF_GRAPH_ALLREDUCE", "SATNERF_TAIL_ADAM", "SATNERF_TAIL_PACK", "SATNERF_DP_PACK"):
            want = old_capture(0.0 if noise_zero else 0.25, coll, pg, backend, failed, object() if late else None, lambda: fused, env)
            got = step_plan.capture_state(noise_zero=noise_zero, collective=coll, pg_initialised=pg, backend=backend, capture_failed=failed,
                                          late_idx=late, fused_forward=fused, env=env)
            assert tuple(got) == want, (noise_zero, coll, pg, backend, failed, late, fused, env)
            rows += 1
    assert rows == 2 * 2 * 3 * 2 * 2 * 2 * 3 ** 4


def test_launches_are_the_old_conditions_on_every_row():
    """Every combination of the three state flags (a test may assign them by hand), the facts and the switches ``launches`` reads: the
    record equals what the old code did -- and where the old code raised one of its two RuntimeErrors, ``launches`` fails its assertion
    with the same message.  Such rows exist HERE, with free flags; test_no_capture_reaches_the_old_runtime_errors shows no capture gives one."""
    rows, raised = 0, 0
    # (a bank's class name only exists with a bank: None, a RayBank, or something else, e.g. a depth-supervision bank)
    for flags in itertools.product(B, B, B, B, (8, 16, 32), (64, 65), B, B, (None, "RayBank", "DepthBank"), B):
        kr, aig, pit, coll, fmt, s, ok, snerf, bank, late = flags
        kw = dict(kernel_rng=kr, adam_in_graph=aig, pack_in_tail=pit, collective=coll, fmt=fmt, n_samples=s, render_fused_ok=ok, snerf=snerf,
                  bank=bank is not None, ray_bank=bank == "RayBank", late_idx=late)
        # (the two switches of fused_forward: unset or at the value they are compared with -- test_fused_forward_is_the_old_condition has
        # their third value -- which keeps the table at a quarter of a million rows)
        for env, fwd in itertools.product(envs("SATNERF_TAIL_ADAM", "SATNERF_GATHER_IN_FWD", "SATNERF_GRAPH_SAMPLER"),
                                          ({}, {"SATNERF_TRAIN_FUSED": "0"}, {"SATNERF_FWD_V1": "1"}, {"SATNERF_TRAIN_FUSED": "0", "SATNERF_FWD_V1": "1"})):
            env = dict(env, **fwd)
            want = old_step(kr, aig, pit, coll, fmt, s, ok, snerf, bank, object() if late else None, env)
            rows += 1
            if isinstance(want, str):
                raised += 1
                with pytest.raises(AssertionError, match=want[:40]):
                    step_plan.launches(env=env, **kw)
                continue
            got = step_plan.launches(env=env, **kw)
            assert got._asdict() == want, (flags, env)
            # invariants of the record itself
            assert (got.sampler != "forward" or (got.fused_forward and kr)) and (("sr_pack_all" in got.names) == bool(got.pack_first))
            assert bool(got.pack_first) == (got.tick == 0) and (got.tail == "tail_adam") == (got.update == "none")
            assert ("all_reduce" in got.names) == (coll and got.tail == "tail")
    assert rows == 2 ** 4 * 3 * 2 * 2 * 2 * 3 * 2 * 3 ** 3 * 4 and 0 < raised < rows


def test_no_capture_reaches_the_old_runtime_errors():
    """A capture's state, handed to ``launches`` under the environment it was captured in: ``pack_in_tail`` implies the one-launch forward
    that opens the step (tick == 2) and, without a collective, sr_grad_tail_adam as the tail -- the conditions of the two RuntimeErrors of
    the old _forward_backward (L289, L339) are unreachable, so they are assertions in ``launches`` now.  The sampler's facts (s-nerf, the
    bank) and its two switches are left at one value: they enter none of these conditions (old_capture and L264-L340 do not name them).
    Every switch is unset or at the value it is compared with: the tables above have shown that its other value reads as unset."""
    rows = packs = 0
    flipped = {"SATNERF_FORCE_ALLREDUCE": "1", "SATNERF_GRAPH_ALLREDUCE": "1", "SATNERF_TAIL_ADAM": "0", "SATNERF_TAIL_PACK": "0",
               "SATNERF_DP_PACK": "0", "SATNERF_TRAIN_FUSED": "0", "SATNERF_FWD_V1": "1"}
    for noise_zero, world, (pg, backend), failed, late, fmt, s, ok in itertools.product(B, (1, 2), GROUPS, B, B, (8, 16, 32), (64, 65), B):
        for chosen in itertools.product(B, repeat=len(flipped)):
            env = {k: v for (k, v), on in zip(flipped.items(), chosen) if on}
            coll = step_plan.collective(world, pg, env)
            st = step_plan.capture_state(noise_zero=noise_zero, collective=coll, pg_initialised=pg, backend=backend, capture_failed=failed,
                                         late_idx=late, fused_forward=step_plan.fused_forward(fmt, s, ok, env), env=env)
            plan = step_plan.launches(kernel_rng=st.kernel_rng, adam_in_graph=st.adam_in_graph, pack_in_tail=st.pack_in_tail, collective=coll,
                                      fmt=fmt, n_samples=s, render_fused_ok=ok, bank=True, ray_bank=True, late_idx=late, env=env)
            # what a replay may ask (Trainer._plan(captured=False)) never depends on a capture's flags -- and never trips the assertions
            free = step_plan.launches(collective=coll, fmt=fmt, n_samples=s, render_fused_ok=ok, bank=True, ray_bank=True, late_idx=late, env=env)
            assert (free.fused_forward, free.graph_sampler) == (plan.fused_forward, plan.graph_sampler)
            rows += 1
            if st.pack_in_tail:
                packs += 1
                assert plan.fused_forward and plan.tick == 2 and not plan.pack_first and "sr_pack_all" not in plan.names
                assert coll or plan.tail == "tail_adam"
                assert plan.update == ("adam_pack" if coll else "none")
            assert st.capture_collective <= (coll and st.adam_in_graph) and plan.update_after_replay == (not st.adam_in_graph)
    assert rows == 2 * 2 * 3 * 2 * 2 * 3 * 2 * 2 * 2 ** 7 and 0 < packs < rows


# ---- the advertised sequences -----------------------------------------------------------------------------------------------------------
def captured(env=None, world=1, backend=None, fmt=8, bank="RayBank"):
    """The plan of a captured step of the benchmarked model (width 256, bf16, 64 samples, sat-nerf, noise_std 0) under ``env``."""
    env = env or {}
    pg = backend is not None
    coll = step_plan.collective(world, pg, env)
    st = step_plan.capture_state(noise_zero=True, collective=coll, pg_initialised=pg, backend=backend, capture_failed=False, late_idx=True,
                                 fused_forward=step_plan.fused_forward(fmt, 64, True, env), env=env)
    return step_plan.launches(kernel_rng=st.kernel_rng, adam_in_graph=st.adam_in_graph, pack_in_tail=st.pack_in_tail, collective=coll, fmt=fmt,
                              n_samples=64, render_fused_ok=True, bank=bank is not None, ray_bank=bank == "RayBank", env=env)


FWD3 = ("sr_satnerf_mlp_fwd", "sr_render_loss")  # behind the ray set-up: the r04 three-launch training forward
BWD = ("sr_satnerf_mlp_bwd", "sr_satnerf_wgrad8")
ADVERTISED = {
    # README.md "A captured single-GPU step is FOUR launches"; INTEGRATION.md "The captured single-GPU step is four launches (r05)"
    "single GPU": (dict(), ("sr_satnerf_render_train",) + BWD + ("sr_grad_tail_adam",)),
    # README.md "the r04 six-launch step"; INTEGRATION.md "the r04 launch sequence (sr_gather_batch, sr_pack_all, ...)"
    "r04 six launches": (dict(env={"SATNERF_TAIL_PACK": "0", "SATNERF_GATHER_IN_FWD": "0", "SATNERF_GRAPH_SAMPLER": "1"}),
                         ("sr_gather_batch", "sr_pack_all", "sr_satnerf_render_train") + BWD + ("sr_grad_tail_adam",)),
    # DESIGN.md section 1 "r04 ran sr_grad_tail and sr_adam_step_graph back to back" (SATNERF_TAIL_ADAM=0 also takes the re-pack out of
    # the tail: sr_pack_all opens the step)
    "tail then Adam": (dict(env={"SATNERF_TAIL_ADAM": "0"}), ("sr_pack_all", "sr_satnerf_render_train") + BWD + ("sr_grad_tail", "sr_adam_step_graph")),
    # DESIGN.md section 1 "bit-identical to sr_ray_setup + MLP + sr_render_loss".  Without the one-launch forward the captured step does not
    # sample for itself by default (the eager gather runs in front of the replay) ...
    "three-launch forward, bank": (dict(env={"SATNERF_TRAIN_FUSED": "0"}), ("sr_pack_all", "sr_ray_setup_rng") + FWD3 + BWD + ("sr_grad_tail_adam",)),
    # ... with SATNERF_GRAPH_SAMPLER=1 its gather launch sets the rays up as well
    "three-launch forward, bank, graph sampler": (dict(env={"SATNERF_TRAIN_FUSED": "0", "SATNERF_GRAPH_SAMPLER": "1"}),
                                                  ("sr_gather_setup", "sr_pack_all") + FWD3 + BWD + ("sr_grad_tail_adam",)),
    "three-launch forward, no bank": (dict(env={"SATNERF_TRAIN_FUSED": "0"}, bank=None),
                                      ("sr_pack_all", "sr_ray_setup_rng") + FWD3 + BWD + ("sr_grad_tail_adam",)),
    # the 16-bit saved state has no one-launch forward; Trainer's docstring "pass args.bwd_fmt = 16"
    "bwd_fmt=16": (dict(fmt=16, bank=None), ("sr_pack_all", "sr_ray_setup_rng") + FWD3 + ("sr_satnerf_mlp_bwd", "sr_satnerf_wgrad", "sr_grad_tail_adam")),
    # DESIGN.md section 6 / INTEGRATION.md "the N > 1 step is the N = 1 step split at the collective"
    "two ranks, gloo": (dict(world=2, backend="gloo"), ("sr_satnerf_render_train",) + BWD + ("sr_grad_tail", "all_reduce", "sr_adam_step_pack")),
    # INTEGRATION.md "SATNERF_DP_PACK=0: the r05 sequence (sr_pack_all first, sr_adam_step last)"
    "two ranks, gloo, r05": (dict(world=2, backend="gloo", env={"SATNERF_DP_PACK": "0"}),
                             ("sr_pack_all", "sr_satnerf_render_train") + BWD + ("sr_grad_tail", "all_reduce", "sr_adam_step")),
    # DESIGN.md section 6 "captured INTO the step's hipGraph" (tests/test_hip_training.py's 1-rank nccl group)
    "one rank, nccl, captured collective": (dict(backend="nccl", env={"SATNERF_FORCE_ALLREDUCE": "1", "SATNERF_GRAPH_ALLREDUCE": "1"}),
                                            ("sr_satnerf_render_train",) + BWD + ("sr_grad_tail", "all_reduce", "sr_adam_step_pack")),
}
IN_GRAPH = {"two ranks, gloo": False, "two ranks, gloo, r05": False, "one rank, nccl, captured collective": True}


@pytest.mark.parametrize("row", list(ADVERTISED))
def test_advertised_launch_sequences(row):
    kw, names = ADVERTISED[row]
    plan = captured(**kw)
    assert plan.names == names
    if row in IN_GRAPH:  # the collective and the update: inside the replayed graph, or issued behind it
        assert plan.update_after_replay == (not IN_GRAPH[row])
    if row == "single GPU":
        assert len(plan.names) == 4 and plan.sampler == "forward" and plan.graph_sampler and plan.tick == 2
    if row == "r04 six launches":
        assert len(plan.names) == 6
