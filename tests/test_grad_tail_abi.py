"""The gradient tail's C ABI on the host: struct layout against the header, and every argument check of the four entries, each of which
returns before any launch (CPU only: the addresses are dummies that nothing dereferences on these paths)."""
import ctypes as C
import os
import re

import pytest

from satnerf_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sr_grad_tail", "sr_grad_tail_det", "sr_grad_tail_adam", "sr_grad_tail_adam_det")
ADDR = 0x10000  # a 16-byte aligned non-null dummy
N_RAYS, HIDDEN, TAU = 100, 64, 4


def header_fields(struct):
    """[(name, size, alignment, is_pointer)] of a struct of include/satrender.h, read from its text."""
    text = open(os.path.join(REPO, "include", "satrender.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    scalar = {"int": 4, "float": 4, "int64_t": 8, "uint64_t": 8}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)(?:\[(\d+)\])?", decl)
        assert m, decl
        base, star, name, count = m.groups()
        fields.append((name, (8 if star else scalar[base]) * int(count or 1), 8 if star else scalar[base], bool(star)))
    return fields


def natural_layout(fields):
    """({name: offset}, sizeof) under natural alignment (each member at a multiple of its element size, the struct padded to its widest)."""
    offsets, at, widest = {}, 0, 1
    for name, size, align, _ in fields:
        at = -(-at // align) * align
        offsets[name] = at
        at += size
        widest = max(widest, align)
    return offsets, -(-at // widest) * widest


@pytest.mark.parametrize("struct, mirror", [("sr_grad_tail_args", _lib.GradTailArgs), ("sr_tail_adam_args", _lib.TailAdamArgs),
                                            ("sr_pack_scatter", _lib.PackScatter)])
def test_struct_layout_matches_header(struct, mirror):
    fields = header_fields(struct)
    offsets, size = natural_layout(fields)
    assert [f[0] for f in mirror._fields_] == [f[0] for f in fields]
    assert C.sizeof(mirror) == size
    for name, fsize, _, _ in fields:
        assert getattr(mirror, name).offset == offsets[name] and getattr(mirror, name).size == fsize, name


def test_header_lists_the_issue_fields():
    assert [f[0] for f in header_fields("sr_grad_tail_args")] == (
        "partial gidx gscale n_params blocks n_blocks grad accumulate sun sun_stride n_rays hidden w1 b1 w2 sky d_sky "
        "g_w1 g_b1 g_w2 g_b2 d_t ts n_samples tau g_emb").split()
    assert [f[0] for f in header_fields("sr_tail_adam_args")] == (
        "params exp_avg exp_avg_sq late_idx n_late state lr beta1 beta2 eps grad_scale pack").split()


TAIL_POINTERS = [f[0] for f in header_fields("sr_grad_tail_args") if f[3]]
ADAM_POINTERS = ["params", "exp_avg", "exp_avg_sq", "late_idx", "state"]  # `pack` may be NULL


@pytest.fixture(scope="module")
def handle():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.lib()


def tail_args(n_rays=N_RAYS, **over):
    a = _lib.GradTailArgs(n_params=1000, n_blocks=14, accumulate=1, sun_stride=3, n_rays=n_rays, hidden=HIDDEN, n_samples=64, tau=TAU)
    for name in TAIL_POINTERS:
        setattr(a, name, ADDR)
    for name, value in over.items():
        setattr(a, name, value)
    return a


def adam_args(**over):
    o = _lib.TailAdamArgs(n_late=8, lr=-1.0, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0)
    for name in ADAM_POINTERS:
        setattr(o, name, ADDR)
    for name, value in over.items():
        setattr(o, name, value)
    return o


def run(handle, entry, args, adam=None, scratch=None, scratch_bytes=0):
    """(status, error text) of one entry; `args` / `adam`: a struct or None (a NULL pointer)."""
    argv = [C.byref(args) if args is not None else None]
    if "adam" in entry:
        argv.append(C.byref(adam) if adam is not None else None)
    if entry.endswith("_det"):
        argv += [scratch, scratch_bytes]
    rc = getattr(handle, entry)(*argv, None)
    return rc, handle.sr_last_error().decode()


def names_entry(msg, entry):
    return msg.startswith(entry + ":")


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_struct_pointers(handle, entry):
    rc, msg = run(handle, entry, None, adam_args(), ADDR, 1 << 30)
    assert rc == 1 and names_entry(msg, entry), msg
    if "adam" in entry:
        rc, msg = run(handle, entry, tail_args(), None, ADDR, 1 << 30)
        assert rc == 1 and names_entry(msg, entry), msg


@pytest.mark.parametrize("field", TAIL_POINTERS)
def test_null_field(handle, field):
    assert len(TAIL_POINTERS) == 18
    for entry in ENTRIES:
        rc, msg = run(handle, entry, tail_args(**{field: None}), adam_args(), ADDR, 1 << 30)
        assert rc == 1 and names_entry(msg, entry) and "null pointer" in msg, (entry, msg)


@pytest.mark.parametrize("entry", ("sr_grad_tail_adam", "sr_grad_tail_adam_det"))
def test_optimizer_checks(handle, entry):
    for field in ADAM_POINTERS:
        rc, msg = run(handle, entry, tail_args(), adam_args(**{field: None}), ADDR, 1 << 30)
        assert rc == 1 and names_entry(msg, entry) and "null optimizer pointer" in msg, (field, msg)
    rc, msg = run(handle, entry, tail_args(), adam_args(n_late=-1), ADDR, 1 << 30)
    assert rc == 1 and names_entry(msg, entry), msg
    # no late parameters: late_idx may be NULL (n_rays = 0, so the call ends behind the checks)
    assert run(handle, entry, tail_args(n_rays=0), adam_args(late_idx=None, n_late=0), ADDR, 1 << 30)[0] == 0
    # a pack with a map needs the stream and the fc_net.0 table; pack->map == NULL means none (checked with the launch's parameters,
    # behind the n_rays <= 0 return: the scratch of the _det entry is then refused, which shows the pack passed)
    bad = _lib.PackScatter(map=ADDR, hi=None, lo=None, l0=ADDR, n_f16=0)
    rc, msg = run(handle, entry, tail_args(), adam_args(pack=C.pointer(bad)), ADDR, 1 << 30)
    assert rc == 1 and names_entry(msg, entry) and "pack needs" in msg, msg
    if entry.endswith("_det"):
        none = _lib.PackScatter()
        rc, msg = run(handle, entry, tail_args(), adam_args(pack=C.pointer(none)), None, 0)
        assert rc == 1 and "scratch" in msg, msg


@pytest.mark.parametrize("entry", ENTRIES)
def test_n_blocks_zero(handle, entry):
    rc, msg = run(handle, entry, tail_args(n_blocks=0), adam_args(), ADDR, 1 << 30)
    assert rc == 1 and names_entry(msg, entry) and "n_blocks = 0" in msg, msg


@pytest.mark.parametrize("entry", ENTRIES)
def test_no_rays_returns_before_the_scratch_check(handle, entry):
    assert run(handle, entry, tail_args(n_rays=0), adam_args(), None, 0)[0] == 0
    # ... but behind the argument checks
    assert run(handle, entry, tail_args(n_rays=0, n_blocks=0), adam_args(), None, 0)[0] == 1


@pytest.mark.parametrize("entry", ("sr_grad_tail_det", "sr_grad_tail_adam_det"))
def test_scratch_checks(handle, entry):
    need = handle.sr_late_grad_scratch_bytes(N_RAYS, HIDDEN, TAU)
    assert need == 4 * (4 + -(-N_RAYS // 32) * (7 * HIDDEN + 3) + N_RAYS * TAU + N_RAYS)
    rc, msg = run(handle, entry, tail_args(), adam_args(), ADDR, need - 4)
    assert rc == 1 and names_entry(msg, entry) and f"need {need}" in msg and f"holds {need - 4}" in msg, msg
    rc, msg = run(handle, entry, tail_args(), adam_args(), ADDR + 4, need)
    assert rc == 1 and names_entry(msg, entry) and "16-byte aligned" in msg, msg
    rc, msg = run(handle, entry, tail_args(), adam_args(), None, need)
    assert rc == 1 and names_entry(msg, entry), msg
