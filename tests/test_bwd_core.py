"""The generated instruction stream of the dX kernel's trunk (csrc/gen/bwd_core.py -> csrc/mlp_bwd_trunk_a*.inc): the committed files are
current, and the instruction list -- executed on a lane-accurate numpy model of the VGPR file, the LDS ring fed by LDS-DMA rows, the
in-order vmcnt / lgkmcnt queues and v_mfma_f32_32x32x16_bf16 -- reproduces seven transposed trunk layers computed directly from the
packed transposed weight stream: the MX8 bytes and scale bytes it stores, the bf16 fragments it hands from layer to layer, the wave maxima
it leaves in the LDS cells.  Validates register allocation, piece / unit addressing, operand order, every wait count (a register or ring
slot is never read while its load is still in the queue), the ring protocol and the hazards the assembler does not pad inside inline
asm, without a GPU: the model is csrc/gen/stream_common.py's ``LaneModel`` with the trunk's own ops (``bwd_core.TrunkMachine``), so the
trunk is held to every check the forward cores are, and the mutation tests at the end break the committed width-256 stream in one
place per check and expect the model to name that check.  (On the GPU, tests/test_hip_backward.py holds the stream's workspace bytes
bit for bit to the compiler-scheduled kernel.)"""
import copy
import functools
import importlib.util
import os
import re

import numpy as np
import pytest

from satnerf_amd import packing
from tests.stream_edits import (_moved, _mut_b_operand, _mut_barriers, _mut_lgkmcnt, _mut_m0_nop, _mut_soff, _mut_sync_rows, _mut_vmcnt,
                                _mut_voff, _nth, _steady, _with_args, _without)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "satnerf_amd", "csrc", "gen", "bwd_core.py")
LANE = np.arange(64)


@functools.lru_cache(maxsize=None)
def _gen():
    spec = importlib.util.spec_from_file_location("bwd_core_gen", GEN)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("feat", [256, 512])
@pytest.mark.parametrize("auxs", [1, 2])
def test_generated_files_are_current(auxs, feat):
    g = _gen()
    name, cname = g.file_names(feat, auxs)
    with open(os.path.join(ROOT, "satnerf_amd", "csrc", name)) as f:
        assert f.read() == g.Trunk(auxs, feat=feat).inc_file(), "re-run satnerf_amd/csrc/gen/bwd_core.py"
    with open(os.path.join(ROOT, "satnerf_amd", "csrc", cname)) as f:
        assert f.read() == g.clobber_file(feat)


@pytest.mark.parametrize("feat,tau", [(256, 4), (256, 16), (512, 4)])
def test_instruction_stream_computes_the_trunk(feat, tau):
    gen = _gen()
    auxs = packing.aux_steps(tau)
    # (SR_BWD_ABLATE: run the lane model on an experimental ordering of the same stream, e.g. storelate, before it goes to the GPU)
    trunk = gen.Trunk(auxs, feat=feat, ablate=tuple(x for x in os.environ.get("SR_BWD_ABLATE", "").split(",") if x))
    G = trunk.g
    KS, MT = G.KS, G.MT
    bm = packing.backward_maps(feat, tau)
    rng = np.random.default_rng(11)
    n_params = bm["n_params"]
    flat = rng.uniform(-0.06, 0.06, n_params).astype(np.float32)
    vals = np.where(bm["idx"] >= 0, flat[np.maximum(bm["idx"], 0)] * bm["scale"], np.float32(0)).astype(np.float32)
    bits = gen.bf16_bits(vals).reshape(-1, 64, 8)
    # the trunk's part of the transposed stream: everything behind bG1 (mlp_layout.h BwdStream: bH | bS3 | bS2 | bG2 | bDT | bG1)
    hs, mth = KS // 2, MT // 2
    first = 3 * mth + 2 * (mth * hs) + MT * 3 * hs + hs + (0 if G.g1 else MT * (KS + 1))   # (Geo.g1: the stream starts at bG1)
    bits = bits[first:]
    n_mfma = 7 * MT * KS + (MT * (KS + 1) if G.g1 else 0)
    assert bits.shape[0] == n_mfma
    stream_bits = (bits[:, :, 0::2] | (bits[:, :, 1::2] << 16)).astype(np.uint32)          # [piece, lane, 4]
    acts = {u: rng.integers(0, 2 ** 32, (64, 4), dtype=np.uint64).astype(np.uint32) for u in range(auxs, auxs + 8 * MT)}   # PHASE8 units of a0..a7
    d7 = (rng.normal(size=(feat, 32)) * 1e-3).astype(np.float32)                          # d pre_7 [feature slot][point]
    x0 = []
    for k in range(KS):                                                                     # B fragment k: lane (p, h) holds slots 16 k + 8 h + j
        fr = np.zeros((64, 8), np.float32)
        for lane in range(64):
            fr[lane] = d7[16 * k + 8 * (lane >> 5): 16 * k + 8 * (lane >> 5) + 8, lane & 31]
        b = gen.bf16_bits(fr)
        x0.append(np.stack([b[:, 2 * q] | (b[:, 2 * q + 1] << 16) for q in range(4)]))
    m = gen.TrunkMachine(trunk, stream_bits, acts, x0)
    xs_mat = (rng.normal(size=(16, 32)) * 1e-3).astype(np.float32)                         # bG1's 17th k-step: the d sigma_pre fragment
    if G.g1:
        fr = np.zeros((64, 8), np.float32)
        for lane in range(64):
            fr[lane] = xs_mat[8 * (lane >> 5): 8 * (lane >> 5) + 8, lane & 31]
        b = gen.bf16_bits(fr)
        m.v[G.XS:G.XS + 4] = np.stack([b[:, 2 * q] | (b[:, 2 * q + 1] << 16) for q in range(4)])
    xs_q = gen.bf16_to_f32(gen.bf16_bits(xs_mat)).astype(np.float64)
    m.run()
    assert trunk.stats["mfma"] == n_mfma and not m.vmq["full"] and not m.pending   # every load and LDS operation retired

    # ---- reference: the seven layers straight from the pieces, float64 contraction, float32 element-wise as the kernel ------------------
    cur = gen.bf16_to_f32(gen.bf16_bits(d7)).astype(np.float64)                                      # [slot, point]
    piece = 0
    for l in range(G.L0, 0, -1):
        nxt = np.zeros((feat, 32), np.float32)
        ebytes = np.zeros((MT, 64), np.uint32)
        grp = l - 1
        sc = m.scale_stores[(G.D8_SCALE + grp // G.GROUPS_PER_UNIT, MT * (grp % G.GROUPS_PER_UNIT))]   # NEB dwords per lane: bytes = E of the layer's tiles
        got_e = np.stack([(sc[:, t_ >> 2] >> (8 * (t_ & 3))) & 0xFF for t_ in range(MT)]).astype(np.int64)
        for t in range(MT):
            D = np.zeros((32, 32))
            for k in range(KS + (1 if l == 8 else 0)):
                A = gen.bf16_to_f32(bits[piece]).astype(np.float64).reshape(2, 32, 8)            # [h, row, j] = W^T rows of this tile, k-slots 16 k + 8 h + j
                piece += 1
                for h in range(2):
                    D += A[h] @ (cur[16 * k + 8 * h: 16 * k + 8 * h + 8] if k < KS else xs_q[8 * h: 8 * h + 8])
            unit = auxs + MT * (l - 1) + t
            ph = acts[unit]                                                                  # [lane, 4 dwords]: value g = byte g & 3 of dword g >> 2
            u = np.stack([(ph[:, gg >> 2] >> (8 * (gg & 3))) & 0xFF for gg in range(16)], 1).astype(np.float64)   # [lane, g]
            c = np.cos(2 * np.pi * (u / 256.0)).astype(np.float32)
            rows = (np.arange(16)[None, :] & 3) + 8 * (np.arange(16)[None, :] >> 2) + 4 * (LANE[:, None] >> 5)
            v = D[rows, (LANE & 31)[:, None]].astype(np.float32) * c                        # [lane, g]
            # next layer's B fragments 2 t, 2 t + 1: slot 32 t + 16 s + 8 h + j holds value g = 8 s + j of lane (p, h)
            for lane in range(64):
                p, h = lane & 31, lane >> 5
                for gg in range(16):
                    nxt[32 * t + 16 * (gg >> 3) + 8 * h + (gg & 7), p] = v[lane, gg]
            mx = np.abs(v).max(1).astype(np.float64)
            e = np.clip(((mx * 0.0078125 + mx).astype(np.float32).view(np.uint32) >> 23).astype(np.int64), 6, 254)
            ebytes[t] = e
            got_q = m.stores[MT * (l - 1) + t].T                                              # [lane, 4 dwords]
            got = np.stack([(got_q[:, gg >> 2] >> (8 * (gg & 3))) & 0xFF for gg in range(16)], 1).astype(np.int64)
            # dequantised with the exponent the stream itself stored (a lane whose largest magnitude sits on a binade boundary may take
            # the neighbouring exponent: fp32 accumulation order of the contraction; a bf16 rounding that falls the other way in an
            # earlier layer moves a later value by a fraction of a code): within 2.5 codes of the coarser scale -- any addressing,
            # operand-order or register mix-up is off by the full range
            deq = (got - 128).astype(np.float64) * (2.0 ** (got_e[t] - 133))[:, None]
            tol = (2.0 ** (np.maximum(got_e[t], e) - 133))[:, None]
            assert (np.abs(deq - v.astype(np.float64)) <= 2.5 * tol).all(), (l, t)
        assert np.abs(got_e - ebytes.astype(np.int64)).max() <= 1
        assert m.cells[grp] == int(got_e.max()), (l, m.cells[grp], int(got_e.max()))      # the wave maximum of exactly the bytes it stored
        cur = gen.bf16_to_f32(gen.bf16_bits(nxt)).astype(np.float64)
    # the last layer's output vector (d pre_0, bf16 B fragments) sits in Y (in X when the stream has an even number of layers)
    out = np.zeros((feat, 32), np.float32)
    last = G.Y if G.LAYERS % 2 else G.X
    for k in range(KS):
        fr = gen.frag_to_f32(m.v[last + 4 * k:last + 4 * k + 4])
        for lane in range(64):
            out[16 * k + 8 * (lane >> 5): 16 * k + 8 * (lane >> 5) + 8, lane & 31] = fr[lane]
    assert np.abs(out - cur).max() <= 2.0 ** -7 * np.abs(cur).max()


# ---- the lane model's checks on the trunk, each provoked by ONE edit of the committed width-256 stream --------------------------------------
def _mut_waitv(ins):
    i = _nth(ins, "waitv", 0, _steady(ins))
    return _with_args(ins, i, (ins[i].a[0] + 1,))


def _mut_pkmul_early(ins):
    """the first pk_mul of a tile, moved to directly behind the tile's last MFMA"""
    i = _nth(ins, "pkmul", 0, _steady(ins))
    last = max(k for k in range(i) if ins[k].op == "mfma" and ins[k].a[0] == ins[i].a[0])
    return _moved(ins, i, last + 1)


def _mut_trans(ins):
    """a pk_mul, moved to directly behind the v_cos of its second source"""
    cos_at = {}
    for i in range(_steady(ins), len(ins)):
        x = ins[i]
        if x.op == "cos":
            cos_at[x.a[0]] = i
        elif x.op == "pkmul" and x.a[1] + 1 in cos_at:
            return _moved(ins, i, cos_at[x.a[1] + 1] + 1)


def _mut_poff(ins):
    return _without(ins, _nth(ins, "poff", 0, _steady(ins)))


def _without_nop_before(op):
    def mutate(ins):
        i = _nth(ins, op, 0, _steady(ins))
        assert ins[i - 1].op == "nop"
        return _without(ins, i - 1)
    return mutate


def _mut_read_under_exec1(ins):
    """the next A-fragment ds_read, moved between the narrowing of EXEC and the cell write"""
    i = _nth(ins, "exec1", 0, _steady(ins))
    assert ins[i + 1].op == "cell"
    return _moved(ins, _nth(ins, "dsread", 0, i), i + 1)


MUTATIONS = {
    "lgkmcnt raised by one": (_mut_lgkmcnt, "MFMA reads an A fragment still in flight"),
    "a rendezvous' vmcnt raised by 8": (_mut_vmcnt, "vmcnt lets a needed request stay in flight"),
    "a phase wait's vmcnt raised by one": (_mut_waitv, "register read while its load is in flight"),
    "no s_nop between the M0 write and its LDS-DMA": (_mut_m0_nop, "M0 write -> LDS-DMA needs one wait state"),
    "no barrier after the third": (_mut_barriers, "DMA overwrites a unit not yet consumed by every wave"),
    "rendezvous covers two rows fewer": (_mut_sync_rows, "unit read before the rendezvous that covers its row"),
    "first pk_mul right behind its tile's last MFMA": (_mut_pkmul_early, "VALU reads an MFMA result too early"),
    "cvt_pk right in front of the MFMA that reads it": (_mut_b_operand, "VALU write -> MFMA operand hazard"),
    "pk_mul right behind the v_cos of its second source": (_mut_trans, "trans result used by the next instruction"),
    "VOFF step removed": (_mut_voff, "VOFF does not address row j of the stream"),
    "POFF step removed": (_mut_poff, "POFF does not address the unit loaded"),
    "SOFF step removed": (_mut_soff, "SOFF does not address the unit stored"),
    "no s_nop in front of a DPP maximum": (_without_nop_before("dppmax"), "VALU write -> DPP read needs two wait states"),
    "no s_nop in front of the v_readlane": (_without_nop_before("readlane"), "VALU write -> v_readlane needs one wait state"),
    "A-fragment read between exec1 and the cell write": (_mut_read_under_exec1, "instruction issued with EXEC narrowed to one lane"),
}


def _run_on_zeros(trunk, ins):
    """the model on an all-zero stream, phases and input (the checks do not depend on the data)"""
    t = copy.copy(trunk)
    t.ins = ins
    G = trunk.g
    acts = {u: np.zeros((64, 4), np.uint32) for u in range(trunk.auxs, trunk.auxs + 8 * G.MT)}
    with np.errstate(all="ignore"):
        _gen().TrunkMachine(t, np.zeros((trunk.n_pieces, 64, 4), np.uint32), acts, np.zeros((G.KS, 4, 64), np.uint32)).run()


@functools.lru_cache(maxsize=None)
def _default_trunk():
    """the committed width-256 stream (auxs = 1), which passes every check unmutated"""
    trunk = _gen().Trunk(1)
    _run_on_zeros(trunk, trunk.ins)
    return trunk


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_lane_model_names_the_broken_rule(mutation):
    trunk = _default_trunk()  # (runs the unmutated stream first: a mutation cannot "fire" because the harness is wrong)
    mutate, message = MUTATIONS[mutation]
    ins = mutate(list(trunk.ins))
    assert [(x.text, x.a) for x in ins] != [(x.text, x.a) for x in trunk.ins]
    with pytest.raises(AssertionError, match=re.escape(message)):
        _run_on_zeros(trunk, ins)
