#!/usr/bin/env python3
"""Generator of the hand-placed gfx950 instruction stream of the fused Sat-NeRF forward MLP core (csrc/mlp_fwd2.inc).

Why a generator: profiles/r03_coissue.txt shows that v_mfma_f32_32x32x16_bf16 and the SIREN epilogue's VALU work (v_sin_f32,
v_cvt_pk_bf16_f32) overlap completely on one SIMD when the stream is placed by hand -- 32.3-32.8 cycles per MFMA with the A fragment
read from LDS -- while hipcc's schedule of the same work (csrc/mlp_fwd.inc) runs at ~75.  The stream is long (1,406 MFMAs per 32-point
tile, every register named) and regular, so it is emitted by this script: ``python fwd_core.py`` writes csrc/mlp_fwd_core_a{1,2}.inc
(string literals #included into one ``asm volatile`` statement).  tests/test_fwd_core.py re-generates the files (they must match what
is committed) and EXECUTES the instruction list on a lane-accurate numpy model of the register file / LDS ring / MFMA against the
packed weight stream, so register allocation, piece addressing, operand order and the DMA ring protocol are validated on the CPU.

The scheduler and the lane model are stream_common.py's (read that docstring first), shared with fwd_core3.py and fwd_core512.py;
this file states what is particular to the width-256 core (one wave = 32 points, 8 waves per workgroup, 2 per SIMD, <= 256 VGPRs):
  * rows of 8 pieces, one 1-KiB request per wave and row, ring of R = 128 pieces, one rendezvous per GROUP = 2 tiles;
  * the epilogue of tile t-1 is 16 v_sin in place on its accumulator and 8 v_cvt_pk into the next stage's B fragments (VGPRs);
  * fc_net.0 (K = 3, fp32 inputs) rides the matrix pipe too: the kernel prologue splits x, y, z and the fc_net.0 rows three ways into
    bf16 (h + m + l = 24 bits) and lays the 21 significant cross products over two k-steps (``l0_terms``), so pieces 0..15 of the ring
    are written by the prologue (not by LDS-DMA) and the stream starts with 8 two-MFMA tiles (always the bf16 opcode, MF0);
  * ``Core(auxs, heads=False)`` is the geometry variant (depth-only rendering): L0..L7 and the sigma tile of the SAME packed stream -- the
    DMA source offset jumps over the feats rows (stream_common.py SRC_JUMP) -- written to csrc/mlp_fwd_core_a{1,2}g.inc by the build, their
    text pinned by the committed digests of gen/variant_streams.sha256 (stream_common.py variant_files), checked by
    tests/test_fwd_core_geometry.py.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stream_common import (CoreBase, LaneModel, Tile, aux_steps, bf16_bits, bf16_to_f32, f32_to_frag, feats_jump, file_digest, main, read_digests,  # noqa: E402,F401
                           variant_files, write_variants)

# ---- register map (VGPR numbers) ------------------------------------------------------------------------------------------------
X, Y = 0, 64            # the two 64-register activation vectors (16 B fragments of 4 registers)
ACC = (128, 144)        # double-buffered tile accumulators
AR0, NA = 160, 6        # ring of A-fragment register quads (PF + 1 entries)
AUX = 184               # aux B fragment(s): 184..187 (and 188..191 when AUXS = 2)
HEAD = 192              # 16 registers: the 5-row output head accumulator
SIG = 208               # sigma pre-activation
VL0, VL1, VOFF = 209, 210, 211  # LDS read bases (ring, ring + 64 KiB) + lane * 16; DMA source offset wave * 1024 + lane * 16 (advanced per row)
N_VGPR = 212
# SAVE8 (training forward, 8-bit workspaces of mlp_layout.h): two quads of store data, the PHASE8 magic constant, the workspace offset
# of this lane (tile base + lane * 16, advanced to the unit being stored), the feats scale bytes, MX8 temporaries
SV = (212, 216)
KMAGIC, SOFF, EB, MXT, K128 = 220, 221, 222, 224, 228   # EB: 2 registers, MXT: 4 (max, exponent, 1/scale, scaled value); K128 = 128.0f
N_VGPR_SAVE = 229
L0B = 232               # two quads: the B fragments of fc_net.0's two k-steps (split coordinates, l0_terms)
L0_PIECES = 16          # ring pieces 0..15: fc_net.0's A fragments, written by the kernel prologue
H0, H1 = 64, 96         # the two 32-register head hidden vectors (in Y once the trunk is done)

KS, HS = 16, 8          # k-steps of a 256-wide / 128-wide input
NW = 8                  # waves per workgroup = pieces per DMA row


def stage_list(auxs, heads=True):
    """The chunk list of FwdStream<AUXS> (mlp_layout.h) with the register assignment of this kernel.  heads=False: the geometry
    variant, L0..L7 and the sigma tile (its units are numbered on from L7's: the feats pieces between them are jumped over)."""
    tiles, p, tno = [], 0, 0
    auxb = [AUX + 4 * a for a in range(auxs)]

    def dense(inp, ks, ntiles, epi, outbase, name, unit0=None, first=False):
        nonlocal p, tno
        for t in range(ntiles):
            # fc_net.0 (first): two k-steps of split operands, no aux k-step; the small cross terms (k-step 1) go first
            b = [inp + 4 * k for k in range(ks)] + ([] if first else auxb)
            out = [outbase + 8 * t + q for q in range(8)] if outbase is not None else None
            tiles.append(Tile(p, b, 1 if first else auxs, ACC[tno & 1], True, epi, out, f"{name}.{t}", None if unit0 is None else auxs + unit0 + t,
                              "MF0" if first else "MF"))
            p += len(b)
            tno += 1

    head_started = [False]

    def head(inp, with_aux, name):
        nonlocal p
        b = [inp + 4 * k for k in range(HS)] + (auxb if with_aux else [])
        tiles.append(Tile(p, b, auxs if with_aux else 0, HEAD, not head_started[0], None, None, name))
        head_started[0] = True
        p += len(b)

    # workspace units (mlp_layout.h SR_FMT8, after the aux fragments): a_l at 8 l + t, feats 64 + t, rgbh 72, s1 76, e1 80, s2 84, s3 88
    dense(L0B, 2, 8, "sin", X, "L0", 0, first=True)
    assert p == L0_PIECES
    for l in range(7):
        dense(X if l % 2 == 0 else Y, KS, 8, "sin", Y if l % 2 == 0 else X, f"L{l + 1}", 8 * (l + 1))
    if heads:
        dense(Y, KS, 8, "id", X, "feats", 64)  # a7 (in Y) -> feats (in X)
    dense(Y, KS, 1, "sigma", None, "sigma")
    if not heads:
        return tiles, p
    dense(X, KS, 4, "sin", H0, "rgbh", 72)
    head(H0, False, "Hr")
    dense(X, KS, 4, "sin", H1, "s1", 76)
    dense(H1, HS, 4, "sin", H0, "s2", 84)
    dense(H0, HS, 4, "sin", H1, "s3", 88)
    head(H1, False, "Hs")
    dense(X, KS, 4, "sin", H0, "e1", 80)
    head(H0, True, "Hb")
    return tiles, p


class Core(CoreBase):
    NW, PRE_ROWS, SRC, VOFF_STEP, LABEL = NW, L0_PIECES // NW, ("sb",), 0x2000, ""
    MT, MTH, SAVE, AR0, NA, SCALE_DWORDS = 8, 4, 8, AR0, NA, 2
    VL, VOFF, HEAD, SIG, SV, SOFF, KMAGIC, EB, MXT, K128 = (VL0, VL1), VOFF, HEAD, SIG, SV, SOFF, KMAGIC, EB, MXT, K128
    stage_list = staticmethod(stage_list)
    VARIANTS = ((dict(heads=False), "g"),)

    def __init__(self, auxs, R=128, PF=5, GROUP=2, FILL=None, ablate=(), save=0, heads=True):
        self.heads = heads
        if not heads:  # sigma's rows are fed from behind the feats rows of the one packed forward stream
            assert save == 0, "the geometry core saves nothing"
            self.stage_list = lambda a: stage_list(a, heads=False)
            self.SRC_JUMP = feats_jump(stage_list(auxs)[0], NW)
        super().__init__(auxs, R, PF, GROUP, FILL, ablate, save)

    def text(self):
        if "empty" in self.ablate:
            return ["s_mov_b32 %[m0save], m0", f"v_mov_b32 v{SIG}, 0"] + [f"v_mov_b32 v{HEAD + g}, 0" for g in range(16 if self.heads else 0)]
        return super().text()

    def header(self):
        if not self.heads:
            row, rows = self.SRC_JUMP
            return ["// GENERATED by csrc/gen/fwd_core.py by the build -- do not edit (its text is pinned by csrc/gen/variant_streams.sha256; tests/test_fwd_core_geometry.py).",
                    f"// geometry (trunk + sigma) forward core, AUXS = {self.auxs}: {self.stats['mfma']} MFMAs, {self.stats['instructions']} instructions, "
                    f"{self.stats['barriers']} rendezvous, {self.stats['rows']} LDS-DMA rows, ring of {self.R} pieces, A fragments {self.PF} ahead.",
                    f"// Reads the packed forward stream of the full core unchanged: behind ring row {row - 1} (L7's last) the source offset jumps over the",
                    f"// {rows} rows of feats pieces, so ring rows {row}.. are the sigma tile's.  No head accumulator: the one output is v{SIG}.",
                    f"// Ring pieces 0..{L0_PIECES - 1} (fc_net.0) are written by the kernel prologue; stream piece p is ring piece p + {L0_PIECES}.",
                    "// Operands: %[sb] stream base (SGPR pair), %[wb] LDS ring address + wave * 1024, %[wave] wave index, %[m0save] scratch SGPR"]
        return ["// GENERATED by csrc/gen/fwd_core.py -- do not edit (tests/test_fwd_core.py checks it is current).",
                f"// fused forward core, AUXS = {self.auxs}: {self.stats['mfma']} MFMAs, {self.stats['instructions']} instructions, "
                f"{self.stats['barriers']} rendezvous, {self.stats['rows']} LDS-DMA rows, ring of {self.R} pieces, A fragments {self.PF} ahead.",
                f"// Ring pieces 0..{L0_PIECES - 1} (fc_net.0) are written by the kernel prologue; stream piece p is ring piece p + {L0_PIECES}.",
                "// Operands: %[sb] stream base (SGPR pair), %[wb] LDS ring address + wave * 1024, %[wave] wave index, %[m0save] scratch SGPR"]

    @staticmethod
    def clobber_file(save=0):
        """registers the statement writes besides its operands (the aux and fc_net.0 fragments, v[192:211], KMAGIC, K128 and SOFF are operands)"""
        regs = list(range(X, AUX))
        if save:
            regs += [r for r in range(SV[0], N_VGPR_SAVE) if r not in (KMAGIC, SOFF, K128)]
        return ("// GENERATED by csrc/gen/fwd_core.py: clobber list of the forward core\n" + ", ".join(f'"v{r}"' for r in regs)
                + ', "memory", "scc"\n')


# =================================================================================================================================
# fc_net.0 on the matrix pipe (what the kernel prologue prepares), and the lane-accurate model
# =================================================================================================================================
def split3(v):
    """fp32 -> three bf16-representable fp32 terms h + m + l = v to 24 bits (each RNE of the remainder; the remainders are exact)"""
    v = np.asarray(v, np.float32)
    h = bf16_to_f32(bf16_bits(v))
    r = (v - h).astype(np.float32)
    m = bf16_to_f32(bf16_bits(r))
    l = bf16_to_f32(bf16_bits((r - m).astype(np.float32)))
    return h, m, l


def l0_terms():
    """fc_net.0 as two bf16 k-steps: slot k of k-step s multiplies part A[s][k] of a table entry with part B[s][k] of a coordinate.
    Entries (column of the (w_x, w_y, w_z, b) table row, part of it, coordinate or None = 1.0, part of it); part 0 / 1 / 2 = h / m / l.
    k-step 0 carries w_h (x_h + x_m + x_l) + w_m x_h per coordinate and the bias, k-step 1 the remaining 2^-16 terms w_m x_m + w_l x_h."""
    Z = None
    s0 = []
    for c in range(3):
        s0 += [(c, 0, c, 0), (c, 0, c, 1), (c, 1, c, 0), (c, 0, c, 2)]
    s0 += [(3, 0, Z, 0), (3, 1, Z, 0), (3, 2, Z, 0), Z]
    s1 = []
    for c in range(3):
        s1 += [(c, 1, c, 1), (c, 2, c, 0)]
    s1 += [Z] * 10
    return s0, s1


def l0_b_frags(xyz):
    """B fragments of the two k-steps for 32 points: [2][64 lanes, 8] fp32 (lane = 32 h + point holds slots 8 h .. 8 h + 7)"""
    parts = [split3(xyz[:, c]) for c in range(3)]
    out = []
    for terms in l0_terms():
        f = np.zeros((64, 8), np.float32)
        for k, t in enumerate(terms):
            if t is None:
                continue
            _, _, c, xp = t
            f[32 * (k >> 3):32 * (k >> 3) + 32, k & 7] = 1.0 if c is None else parts[c][xp]
        out.append(f)
    return out


def l0_pieces(l0_table):
    """A fragments of fc_net.0: [16 pieces = (tile t, k-step s)][64 lanes = 32 (k >> 3) + row][8] fp32 from the (slot-ordered, scaled)
    table [256, 4]; row r of tile t is slot 16 (2 t + (g >> 3)) + 8 hh + (g & 7) with g = (r & 3) + 4 (r >> 3), hh = (r >> 2) & 1 -- the
    accumulator layout that makes tile t the B fragments 2 t, 2 t + 1 of the next layer (what the VALU prologue of r02 produced)."""
    r = np.arange(32)
    g, hh = (r & 3) + 4 * (r >> 3), (r >> 2) & 1
    out = np.zeros((16, 64, 8), np.float32)
    for t in range(8):
        slot = 16 * (2 * t + (g >> 3)) + 8 * hh + (g & 7)
        parts = [split3(l0_table[slot, c]) for c in range(4)]
        for s, terms in enumerate(l0_terms()):
            for k, tm in enumerate(terms):
                if tm is not None:
                    out[2 * t + s, 32 * (k >> 3):32 * (k >> 3) + 32, k & 7] = parts[tm[0]][tm[1]]
    return out


class Machine(LaneModel):
    """the width-256 core on the shared lane model: ring pieces 0..15 (fc_net.0) are in the ring when the stream starts"""


STEM = "mlp_fwd_core"  # csrc/<STEM>_a<auxs>[s<save> | g].inc

if __name__ == "__main__":
    sys.exit(main(Core, STEM, __doc__, R=128, PF=5, GROUP=2, FILL=None))
