"""The five C entries of the fused forward (sr_satnerf_mlp_fwd, sr_satnerf_mlp_sigma, sr_satnerf_render_fwd, sr_satnerf_render_train,
sr_satnerf_render_depth) refuse a bad request with the status and the sr_last_error() text recorded in
tests/golden/fwd_entry_errors.json (tests/golden/make_fwd_entry_errors.py wrote it from this case table, before the entries' host code
was folded into one request path).  No GPU: every request is EMPTY (n_points = 0 / n_rays = 0) and every argument check runs before
the empty return, so a case that a broken check lets through returns 0 and fails its assertion -- the made-up pointers are never
dereferenced and nothing is ever launched."""
import ctypes as C
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fwd_entry_errors.json")

P = 0x10000  # a made-up non-null pointer
BF16, F16, BF16X3 = 1, 2, 3

_STREAM = dict(feat=256, tau=4, mode=BF16, stream_hi=P, stream_lo=None, l0=P)
_POINT_IN = dict(org=P, org_stride=3, dir=P, dir_stride=3, sun=P, sun_stride=3, z=None, temb=P, ts=P, n_points=0, n_samples=1)
_RENDER_IN = dict(rays=P, ray_stride=11, ts=P, temb=P, n_rays=0, n_samples=64, z_in=None, u=None, seed=0, step_counter=None, tick=0,
                  noise=None, noise_std=0.0, sky_hidden=8, sky_w1=P, sky_b1=P, sky_w2=P, sky_b2=P, bank_chunks=0)
_OUT = ("z_vals", "albedo", "sigma", "sun_v", "beta", "sky", "weights", "transparency", "depth", "rgb")
_TRAIN = dict(target=P, sched=None, beta_min=0.05, loss_parts=P, rgb=P, d_sigma=P, d_albedo=P, d_sun_v=P, g_beta=P, d_sky=P, gather_idx=None,
              cursor=None, batches=0, out_rays=None, out_rgbs=None, out_ts=None)
_SAMPLER = {"train.gather_idx": P, "train.cursor": P, "train.batches": 4, "train.out_rays": P, "train.out_rgbs": P, "train.out_ts": P}

# entry -> (its valid, empty request: block name -> fields, "" = the scalar arguments; the order of the C arguments)
BASE = {
    "sr_satnerf_mlp_fwd": ({"in": _POINT_IN, "": dict(_STREAM, albedo=P, sigma=P, sun_v=P, beta=P, acts=None, act_fmt=0)},
                           ("in", "feat", "tau", "mode", "stream_hi", "stream_lo", "l0", "albedo", "sigma", "sun_v", "beta", "acts", "act_fmt")),
    "sr_satnerf_mlp_sigma": ({"in": _POINT_IN, "": dict(_STREAM, sigma=P)}, ("in", "feat", "tau", "mode", "stream_hi", "stream_lo", "l0", "sigma")),
    "sr_satnerf_render_fwd": ({"in": _RENDER_IN, "out": dict.fromkeys(_OUT, P), "": _STREAM},
                              ("in", "feat", "tau", "mode", "stream_hi", "stream_lo", "l0", "out")),
    "sr_satnerf_render_depth": ({"in": _RENDER_IN, "out": dict.fromkeys(_OUT, P), "": _STREAM},
                                ("in", "feat", "tau", "mode", "stream_hi", "stream_lo", "l0", "out")),
    "sr_satnerf_render_train": ({"in": _RENDER_IN, "out": dict.fromkeys(_OUT, P), "train": _TRAIN, "": dict(_STREAM, acts=P, act_fmt=8)},
                                ("in", "feat", "tau", "mode", "stream_hi", "stream_lo", "l0", "out", "train", "acts", "act_fmt")),
}
POINT = ("sr_satnerf_mlp_fwd", "sr_satnerf_mlp_sigma")
RENDER = ("sr_satnerf_render_fwd", "sr_satnerf_render_depth", "sr_satnerf_render_train")
FWD, SIGMA, PLAIN, DEPTH, TRAIN = POINT + RENDER


def _cases():
    """(entry, case name, {"block.field" or scalar or block name: value}): one fault per case."""
    c = []

    def add(entries, name, **kw):
        c.extend((e, name, {k.replace("__", "."): v for k, v in kw.items()}) for e in entries)

    def add_d(entries, name, changes):
        c.extend((e, name, dict(changes)) for e in entries)

    # ---- every entry
    add(POINT + RENDER, "null in", **{"in": None})
    add(RENDER, "null out", out=None)
    add([SIGMA], "null sigma", sigma=None)
    add([TRAIN], "null train", train=None)
    add(POINT + RENDER, "feat 384", feat=384)
    add(POINT + RENDER, "mode 0", mode=0)
    add(POINT + RENDER, "mode 4", mode=4)
    add(POINT + RENDER, "tau 0", tau=0)
    add(POINT + RENDER, "tau 25", tau=25)
    add(POINT + RENDER, "null stream_hi", stream_hi=None)
    add(POINT + RENDER, "null l0", l0=None)
    add(POINT + RENDER, "null temb", in__temb=None)
    add(POINT, "null org", in__org=None)
    add(POINT, "null sun", in__sun=None)
    add(RENDER, "null rays", in__rays=None)
    add(RENDER, "null ts", in__ts=None)
    add(POINT + RENDER, "bf16x3 without lo", mode=BF16X3)
    add(POINT + RENDER, "feat 512 bf16x3", feat=512, mode=BF16X3, stream_lo=P)
    add(POINT + RENDER, "n_samples 0", in__n_samples=0)
    add(RENDER, "n_samples 1", in__n_samples=1)
    add(RENDER, "n_samples 50", in__n_samples=50)
    add(RENDER, "n_samples 50 feat 512", feat=512, in__n_samples=50)
    # ---- the point entries
    add([FWD], "act_fmt 7", acts=P, act_fmt=7)
    add([FWD], "feat 512 saving fmt16", feat=512, acts=P, act_fmt=16)
    add([FWD], "feat 512 f16 saving fmt16", feat=512, mode=F16, acts=P, act_fmt=16)
    # ---- the render entries
    add(RENDER, "ray_stride 10", in__ray_stride=10)
    for k in ("sky_w1", "sky_b1", "sky_w2", "sky_b2"):
        add_d([PLAIN, TRAIN], "null " + k, {"in." + k: None})
        add_d([DEPTH], "bf16x3 null " + k, {"mode": BF16X3, "stream_lo": P, "in." + k: None})
    add([PLAIN, TRAIN], "sky_hidden 0", in__sky_hidden=0)
    add([DEPTH], "bf16x3 sky_hidden 0", mode=BF16X3, stream_lo=P, in__sky_hidden=0)
    add_d([DEPTH], "bf16x3 without sky", {"mode": BF16X3, "stream_lo": P, "in.sky_hidden": 0, **{"in." + k: None for k in ("sky_w1", "sky_b1", "sky_w2", "sky_b2")}})
    add([PLAIN, DEPTH], "null weights", out__weights=None)
    add([PLAIN, DEPTH], "null transparency", out__transparency=None)
    add([DEPTH], "null depth", out__depth=None)
    add(RENDER, "tick 1 without counter", in__tick=1)
    add(RENDER, "tick 3", in__tick=3, in__step_counter=P)
    add(RENDER, "tick -1", in__tick=-1, in__step_counter=P)
    add([PLAIN, DEPTH], "tick 2", in__tick=2, in__step_counter=P)
    add([TRAIN], "tick 2 with bank_chunks", in__tick=2, in__step_counter=P, in__bank_chunks=2)
    add(RENDER, "bank_chunks -1", in__bank_chunks=-1, in__step_counter=P)
    add(RENDER, "bank_chunks 2 without counter", in__bank_chunks=2)
    # ---- the training launch
    add([TRAIN], "bf16x3", mode=BF16X3, stream_lo=P)
    add([TRAIN], "without acts", acts=None)
    add([TRAIN], "fmt16", act_fmt=16)
    add([TRAIN], "n_samples 128", in__n_samples=128)
    for k in ("target", "loss_parts", "d_sigma", "d_albedo", "d_sun_v", "g_beta", "d_sky"):
        add_d([TRAIN], "null train " + k, {"train." + k: None})
    for k in ("sky", "albedo", "sigma", "sun_v", "beta"):
        add_d([TRAIN], "null out " + k, {"out." + k: None})
    add_d([TRAIN], "sampler without cursor", {**_SAMPLER, "train.cursor": None})
    add_d([TRAIN], "sampler batches 0", {**_SAMPLER, "train.batches": 0})
    add_d([TRAIN], "sampler batches 1 << 24", {**_SAMPLER, "train.batches": 1 << 24})
    for k in ("out_rays", "out_rgbs", "out_ts"):
        add_d([TRAIN], "sampler without " + k, {**_SAMPLER, "train." + k: None})
    add_d([TRAIN], "sampler ray_stride 12", {**_SAMPLER, "in.ray_stride": 12})
    add_d([TRAIN], "sampler with u", {**_SAMPLER, "in.u": P})
    add_d([TRAIN], "sampler with z_in", {**_SAMPLER, "in.z_in": P})
    add_d([TRAIN], "sampler with noise", {**_SAMPLER, "in.noise": P})
    add_d([TRAIN], "sampler with bank_chunks", {**_SAMPLER, "in.bank_chunks": 2, "in.step_counter": P})
    return c


CASES = _cases()


def case_id(entry, name):
    return f"{entry}: {name}"


def call(lib, entry, changes=()):
    """The entry's valid empty request with ``changes`` applied -> (status, sr_last_error() text)."""
    from satnerf_amd import _lib

    blocks, order = BASE[entry]
    blocks = {k: dict(v) if v is not None else None for k, v in blocks.items()}
    for key, value in dict(changes).items():
        block, _, field = key.rpartition(".")
        if not block and key in blocks:
            blocks[key] = value  # a whole argument block (None)
        else:
            assert field in blocks[block], key
            blocks[block][field] = value
    types = {"in": _lib.MlpInputs if entry in POINT else _lib.RenderArgs, "out": _lib.RenderOutputs, "train": _lib.TrainArgs}
    structs = {k: types[k](**v) for k, v in blocks.items() if k and v is not None}  # kept alive over the call
    args = [(C.byref(structs[a]) if a in structs else None) if a in types else blocks[""][a] for a in order]
    status = getattr(lib, entry)(*args, None)
    return status, lib.sr_last_error().decode()


def load_lib():
    from satnerf_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def lib():
    assert os.environ.get("SATNERF_FWD_V1", "") != "1", "the recorded texts are those of a process without SATNERF_FWD_V1"
    return load_lib()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_case_table_is_the_recorded_one(golden):
    ids = [case_id(e, n) for e, n, _ in CASES]
    assert len(set(ids)) == len(ids) and sorted(ids) == sorted(golden)
    for rec in golden.values():  # conditions of the recording: every faulty request was refused with a message
        assert rec["status"] != 0 and rec["error"]


@pytest.mark.parametrize("entry", POINT + RENDER)
def test_a_valid_empty_request_returns_zero(lib, entry):
    assert call(lib, entry)[0] == 0, lib.sr_last_error().decode()


@pytest.mark.parametrize("entry,name,changes", CASES, ids=[case_id(e, n) for e, n, _ in CASES])
def test_one_fault_gives_the_recorded_status_and_text(lib, golden, entry, name, changes):
    status, error = call(lib, entry, changes)
    want = golden[case_id(entry, name)]
    assert status == want["status"] and status != 0
    assert error == want["error"]
