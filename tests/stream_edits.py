"""One-place edits of a generated instruction list (csrc/gen/stream_common.py ``Ins`` records), shared by the mutation tests of
tests/test_fwd_core.py and tests/test_bwd_core.py: each breaks one rule the lane model checks."""
import copy


def _nth(ins, op, n, start=0):
    """index of the n-th (from 0) instruction of kind `op` at or after `start`"""
    return [i for i in range(start, len(ins)) if ins[i].op == op][n]


def _moved(ins, src, dst):
    """the list with instruction `src` taken out and put back so that it stands directly in front of what was instruction `dst`"""
    out = list(ins)
    x = out.pop(src)
    out.insert(dst - (src < dst), x)
    return out


def _with_args(ins, i, a):
    out = list(ins)
    out[i] = copy.copy(ins[i])
    out[i].a = a
    return out


def _without(ins, i):
    return ins[:i] + ins[i + 1:]


def _steady(ins):
    """where the edits are made: behind the third rendezvous, in the regular part of the stream"""
    return _nth(ins, "barrier", 2)


def _mut_lgkmcnt(ins):
    i = _nth(ins, "waitl", 0, _steady(ins))
    return _with_args(ins, i, (ins[i].a[0] + 1,))


def _mut_vmcnt(ins):
    i = _nth(ins, "sync", 0, _steady(ins))
    return _with_args(ins, i, (ins[i].a[0] + 8, ins[i].a[1]))


def _mut_m0_nop(ins):
    i = _nth(ins, "m0", 0, _steady(ins))
    assert ins[i + 1].op == "nop" and ins[i + 2].op == "dma"
    return _without(ins, i + 1)


def _mut_barriers(ins):
    s = _steady(ins)
    return [x for i, x in enumerate(ins) if i <= s or x.op != "barrier"]


def _mut_sync_rows(ins):
    i = _nth(ins, "sync", 0, _steady(ins))
    return _with_args(ins, i, (ins[i].a[0], ins[i].a[1] - 2))


def _mut_b_operand(ins):
    """the cvt_pk / v_accvgpr_write closest to the MFMA that reads the B operand it writes, moved to directly in front of that MFMA"""
    writer, best = {}, None
    for i in range(_steady(ins), len(ins)):
        x = ins[i]
        if x.op in ("pk", "accw"):
            writer[x.a[0]] = i
        elif x.op == "mfma":
            w = max(writer.get(r, -1) for r in range(x.a[2], x.a[2] + 4))
            if w >= 0 and (best is None or i - w < best[1] - best[0]):
                best = (w, i)
    return _moved(ins, *best)


def _mut_voff(ins):
    return _without(ins, _nth(ins, "voff", 0, _steady(ins)))


def _mut_soff(ins):
    return _without(ins, _nth(ins, "soff", 2))
