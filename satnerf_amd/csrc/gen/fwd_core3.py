#!/usr/bin/env python3
"""Generator of the hand-placed gfx950 instruction stream of the PARITY-mode (bf16x3) forward core (csrc/mlp_fwd3.inc).

Same method as fwd_core.py, same scheduler and lane model (stream_common.py: read that docstring first), other machine shape: in the parity mode every operand is a pair of bf16
planes (hi = RNE(v), lo = RNE(v - hi)) and every k-step is three MFMAs -- A_lo x B_hi, A_hi x B_lo, A_hi x B_hi, small terms first --
so a wave's activations are 4 x 64 registers.  The wave therefore runs alone on its SIMD with the unified 512-register file:
  * architectural VGPRs: the hi planes of both activation vectors (VALU writes them), the two tile accumulators (VALU reads them),
    epilogue temporaries;
  * accumulation VGPRs (a0..a255, numbered 256.. here): the lo planes (written by v_accvgpr_write), the A-fragment ring (ds_read_b128
    straight into AGPRs), the aux fragments, the head accumulator.  MFMA takes A / B / C / D from either file.
  * 4 waves per workgroup; a "unit" = one k-step of one output tile = 1 KiB of the hi stream + 1 KiB of the lo stream (the two packed
    streams of packing.py, same piece order); LDS ring of R units (2 KiB slots: hi, lo) fed by rows of 4 units, two 1-KiB requests per
    wave and row; one rendezvous per output tile (51 MFMAs), placed PF k-steps before the first read that needs it.
  * epilogue of tile t-1 in the gaps of tile t: v_fract + v_sin (the hardware sine on the exact fraction: 1.6e-6 of the reference end
    to end, profiles/r03_ab_variants.txt), hi = cvt_pk, lo = cvt_pk(v - float(hi)) -> v_accvgpr_write: 88 VALU per 51 MFMAs.
  * save = 16 (training in the parity mode, SR_FMT16 workspaces of mlp_layout.h): the phase of every sin stage's pre-activation as
    unorm16 (v_cvt_pknorm_u16 of the exact fractions, before the in-place sine) and the bf16 hi plane of feats, two non-temporal
    1-KiB-per-wave stores per tile in the MFMA gaps.
``python fwd_core3.py`` writes csrc/mlp_fwd3_core_a{1,2}.inc and mlp_fwd3_core_clobbers.inc; tests/test_fwd_core.py checks they are
current and executes the list on the lane-accurate model against the fp64 emulator.
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stream_common import A0, CoreBase, LaneModel, Tile, aux_steps, bf16_bits, bf16_to_f32, main, rn  # noqa: E402,F401

# ---- register map (unified numbering: 0..255 = v, A0 + 0..255 = a)
XH, YH = 0, 64                # hi planes (VGPR)
ACC = (128, 144)
TMP = (160, 164)              # two sets of epilogue temporaries (3 used of each)
SIG = 168
VL0, VL1, VOFF = 169, 170, 171
N_VGPR = 172
SV = (172, 180)               # save = 16: two sets of two store quads (unorm16 phases of a tile)
SOFF = 188                    # this lane's workspace offset (tile base + lane * 16, advanced fragment by fragment)
N_VGPR_SAVE = 189
XL, YL = A0 + 0, A0 + 64      # lo planes (AGPR)
AR0, NA = A0 + 128, 4         # A-fragment ring: NA k-steps x (lo quad, hi quad)
AUXH, AUXL = A0 + 160, A0 + 168
HEAD = A0 + 176
N_AGPR = 192
# operands arrive in VGPRs and are moved by the stream's first instructions: X lo plane in v[64:127], aux hi / lo in v[144:151] / v[152:159]
IN_XL, IN_AUXH, IN_AUXL = 64, 144, 152
OUT_HEAD = 128                # the head accumulator is copied to v[128:143] at the end
KS, HS, NW = 16, 8, 4

MFMA = "v_mfma_f32_32x32x16_bf16"   # the parity mode's operands are always bf16: the opcode is spelled out


def stage_list(auxs):
    tiles, p, tno = [], 0, 0
    auxh = [AUXH + 4 * a for a in range(auxs)]
    auxl = [AUXL + 4 * a for a in range(auxs)]

    def dense(ih, il, ks, ntiles, epi, oh, ol, name, frag0=None):
        nonlocal p, tno
        for t in range(ntiles):
            bh = [ih + 4 * k for k in range(ks)] + auxh
            bl = [il + 4 * k for k in range(ks)] + auxl
            out_h = [oh + 8 * t + q for q in range(8)] if oh is not None else None
            out_l = [ol + 8 * t + q for q in range(8)] if ol is not None else None
            # save_unit: SR_FMT16 workspace fragment (1 KiB per tile of 32 points) of this tile's values 0..7; 8..15 go to the next one
            tiles.append(Tile(p, list(zip(bh, bl)), auxs, ACC[tno & 1], True, epi, (out_h, out_l), f"{name}.{t}",
                              None if frag0 is None else auxs + frag0 + 2 * t, MFMA))
            p += len(bh)
            tno += 1

    started = [False]

    def head(ih, il, with_aux, name):
        nonlocal p
        bh = [ih + 4 * k for k in range(HS)] + (auxh if with_aux else [])
        bl = [il + 4 * k for k in range(HS)] + (auxl if with_aux else [])
        tiles.append(Tile(p, list(zip(bh, bl)), auxs if with_aux else 0, HEAD, not started[0], None, None, name, op=MFMA))
        started[0] = True
        p += len(bh)

    for l in range(7):
        a, b = ((XH, XL), (YH, YL)) if l % 2 == 0 else ((YH, YL), (XH, XL))
        dense(a[0], a[1], KS, 8, "sin", b[0], b[1], f"L{l + 1}", 16 * (l + 1))   # mlp_layout.h: a_l at fragment 16 l (+ auxs)
    dense(YH, YL, KS, 8, "id", XH, XL, "feats", 128)
    dense(YH, YL, KS, 1, "sigma", None, None, "sigma")
    H0, H1 = (YH, YL), (YH + 32, YL + 32)
    dense(XH, XL, KS, 4, "sin", H0[0], H0[1], "rgbh", 144)
    head(H0[0], H0[1], False, "Hr")
    dense(XH, XL, KS, 4, "sin", H1[0], H1[1], "s1", 152)
    dense(H1[0], H1[1], HS, 4, "sin", H0[0], H0[1], "s2", 168)
    dense(H0[0], H0[1], HS, 4, "sin", H1[0], H1[1], "s3", 176)
    head(H1[0], H1[1], False, "Hs")
    dense(XH, XL, KS, 4, "sin", H0[0], H0[1], "e1", 160)
    head(H0[0], H0[1], True, "Hb")
    return tiles, p


class Core3(CoreBase):
    NW, SRC, VOFF_STEP, LABEL, SYNC_AHEAD, PK = NW, ("sh", "sl"), 0x1000, "3", True, "v_cvt_pk_bf16_f32"
    SAVE, NA, OUT_HEAD = 16, NA, OUT_HEAD
    VL, VOFF, HEAD, SIG, SOFF = (VL0, VL1), VOFF, HEAD, SIG, SOFF
    stage_list = staticmethod(stage_list)

    def __init__(self, auxs, R=64, PF=2, FILL=2, ablate=(), save=0):
        super().__init__(auxs, R, PF, 1, FILL, ablate, save)  # one rendezvous per output tile
        self.n_units = self.n_pieces

    def a_frags(self, i):
        """(register quad, plane) of the A fragments of k-step i, in read order: lo first (the first MFMA of a k-step takes A_lo)"""
        base = AR0 + 8 * (i % NA)
        return [(base, 1), (base + 4, 0)]

    def mfmas(self, t, k, aregs):
        (alo, ahi), (bh, bl) = aregs, t.bregs[k]
        return [(alo, bh), (ahi, bl), (ahi, bh)]  # small terms first

    def preamble(self):
        for i in range(64):
            self._e("accw", (XL + i, IN_XL + i), f"v_accvgpr_write_b32 {rn(XL + i)}, v{IN_XL + i}")
        for a in range(self.auxs):
            for i in range(4):
                self._e("accw", (AUXH + 4 * a + i, IN_AUXH + 4 * a + i), f"v_accvgpr_write_b32 {rn(AUXH + 4 * a + i)}, v{IN_AUXH + 4 * a + i}")
                self._e("accw", (AUXL + 4 * a + i, IN_AUXL + 4 * a + i), f"v_accvgpr_write_b32 {rn(AUXL + 4 * a + i)}, v{IN_AUXL + 4 * a + i}")

    def queue_dense(self, ti, g0):
        """fract + sin on the exact fraction, hi = cvt_pk, lo = cvt_pk(v - float(hi)) -> v_accvgpr_write; unorm16 phase / bf16 feats saves"""
        t = self.tiles[ti]
        epi_q, a, sin, (out_h, out_l) = self.epi_q, t.acc, t.epi == "sin", t.out
        saving = self.save and t.save_unit is not None
        sv = None
        if saving and sin:
            sv = SV[self.n_saves & 1]
            self.n_saves += 1

        def phase(q):  # unorm16 phases of values 2 q, 2 q + 1 (exact fractions) -> word q of the tile's two store quads
            if sv is not None:
                epi_q.append([g0, "pknorm", (sv + q, a + 2 * q, a + 2 * q + 1), set(), a])
                if q in (3, 7):
                    epi_q.append([g0, "store", (sv + (q - 3), t.save_unit + (q >> 2)), set(), None])
        if sin:
            for g in range(16):  # the exact fraction first: v_sin's own range reduction is not trusted at parity tolerances
                epi_q.append([g0, "fract", (a + g,), set(), a])
            phase(0)
            epi_q.append([g0, "sin", (a + 0,), set(), a])
            epi_q.append([g0, "sin", (a + 1,), set(), a])
        for q in range(8):
            v0, v1 = a + 2 * q, a + 2 * q + 1
            t0, t1, t2 = (TMP[q & 1] + j for j in range(3))
            if sin and q < 7:
                phase(q + 1)
                epi_q.append([g0, "sin", (v0 + 2,), set(), a])
            epi_q.append([g0, "pk", (out_h[q], v0, v1), {out_h[q]}, a])
            if saving and not sin and q in (3, 7):  # identity stage: the bf16 hi plane itself
                epi_q.append([g0, "store", (out_h[q - 3], t.save_unit + (q >> 2)), set(), None])
            if sin and q < 7:
                epi_q.append([g0, "sin", (v1 + 2,), set(), a])
            epi_q.append([g0, "shl", (t0, out_h[q]), set(), None])
            epi_q.append([g0, "and", (t1, out_h[q]), set(), None])
            epi_q.append([g0, "sub", (v0, v0, t0), set(), a])
            epi_q.append([g0, "sub", (v1, v1, t1), set(), a])
            epi_q.append([g0, "pk", (t2, v0, v1), set(), a])
            epi_q.append([g0, "accw", (out_l[q], t2), {out_l[q]}, None])

    def emit_epi(self, kind, args):
        if kind == "fract":
            self._e("fract", args, f"v_fract_f32 v{args[0]}, v{args[0]}")
        elif kind == "shl":
            self._e("shl", args, f"v_lshlrev_b32 v{args[0]}, 16, v{args[1]}")
        elif kind == "and":
            self._e("and", args, f"v_and_b32 v{args[0]}, 0xffff0000, v{args[1]}")
        elif kind == "sub":
            self._after_trans(args[1])
            self._e("sub", args, f"v_sub_f32 v{args[0]}, v{args[1]}, v{args[2]}")
        elif kind == "pknorm":
            self._e("pknorm", args, f"v_cvt_pknorm_u16_f32 v{args[0]}, v{args[1]}, v{args[2]}")
        else:
            super().emit_epi(kind, args)

    def header(self):
        s = self.stats
        return ["// GENERATED by csrc/gen/fwd_core3.py -- do not edit (tests/test_fwd_core.py checks it is current).",
                f"// parity-mode (bf16x3) forward core, AUXS = {self.auxs}: {s['mfma']} MFMAs, {s['instructions']} instructions, "
                f"{s['barriers']} rendezvous, {s['rows']} LDS-DMA rows, ring of {self.R} units, A fragments {self.PF} k-steps ahead.",
                "// Operands: %[sh] / %[sl] hi / lo stream base (SGPR pairs), %[wb] LDS ring address + wave * 2048, %[wave], %[m0save]"]

    @staticmethod
    def clobber_file(save=0):
        # operands: v[0:127] (X hi, X lo in), v[128:143] (head out), v[144:159] (aux in), SIG, VL0, VL1, VOFF[, SOFF]
        regs = [f"v{r}" for r in range(TMP[0], TMP[1] + 4)]
        if save:
            regs += [f"v{r}" for r in range(SV[0], SV[1] + 8)]
        regs += [f"a{r}" for r in range(N_AGPR)]
        return ("// GENERATED by csrc/gen/fwd_core3.py: clobber list of the parity-mode forward core\n" + ", ".join(f'"{r}"' for r in regs)
                + ', "memory", "scc"\n')


class Machine3(LaneModel):
    """the parity core on the shared lane model: Machine3(core, hi_bits, lo_bits), two planes per ring slot, three MFMAs per unit"""


if __name__ == "__main__":
    sys.exit(main(Core3, "mlp_fwd3_core", __doc__, PF=2, FILL=2))
