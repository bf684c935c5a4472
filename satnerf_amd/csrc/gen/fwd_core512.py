#!/usr/bin/env python3
"""Generator of the hand-placed gfx950 instruction stream of the WIDTH-512 forward core (csrc/mlp_fwd512g.inc), inference and the
one-launch render pass in the single-pass modes (bf16 / f16 operands).

Same method as fwd_core.py, same scheduler and lane model (stream_common.py: read that docstring first); the machine shape is fwd_core3.py's: at width 512 one activation vector of a
32-point wave is 128 registers, so the wave runs alone on its SIMD with the unified 512-register file --
  * VGPRs: activation vector X (the trunk's even layers' input, feats), the two tile accumulators, temporaries;
  * AGPRs (numbered 256.. here): activation vector Y (odd layers' input, the two 256-wide head hidden vectors; written by
    v_accvgpr_write behind the cvt_pk), the A-fragment ring (ds_read_b128 straight into AGPRs), aux fragments, head accumulator;
  * 4 waves per workgroup, LDS ring of 144 pieces (1 KiB = one k-step of one 32-row output tile) fed by rows of 4 (one request per
    wave), one rendezvous per output tile (33 MFMAs; two tiles per rendezvous would need a ring of 5 tiles), A fragments PF MFMAs
    ahead, the epilogue of tile t-1 (16 v_sin, 8 v_cvt_pk, 8 v_accvgpr_write when the output vector lives in AGPRs) in the gaps of tile t.
save = 8 (the training forward): the PHASE8 byte of every sin stage's pre-activation (SDWA add into its byte of the store quad before
the in-place sine), MX8 feats + scale bytes, non-temporal stores in the MFMA gaps -- fwd_core.py's scheme with the unit numbers of
width 512 (mlp_layout.h: a_l at 16 l + t, feats 128, rgbh 144, s1 152, e1 160, s2 168, s3 176, scale unit 184, all + auxs).
5,370 MFMAs per 32 points (tau <= 8).  ``python fwd_core512.py`` writes csrc/mlp_fwd512_core_a{1,2}.inc and the clobber list;
tests/test_fwd_core.py checks they are current and executes the list on the lane-accurate model against the emulator.
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stream_common import A0, CoreBase, LaneModel, Tile, aux_steps, bf16_bits, f32_to_frag, feats_jump, file_digest, main, read_digests, rn, variant_files, write_variants  # noqa: E402,F401

FEAT = 512
KS, HS, MT, MTH, NW = FEAT // 16, FEAT // 32, FEAT // 32, FEAT // 64, 4
X = 0                         # 128 VGPRs
ACC = (128, 144)
TMP = (160, 161, 162, 163)    # cvt_pk results on their way to AGPRs
SIG = 168
VL = (169, 170, 171)          # LDS read bases: ring + lane * 16 (+ 64 KiB, + 128 KiB)
VOFF = 172
N_VGPR = 173
SV = (174, 178)               # save = 8: two quads of store data (register tuples are 64-bit aligned on gfx950)
SOFF, KMAGIC, EB, MXT, K128 = 182, 183, 184, 188, 192   # workspace offset, PHASE8 constant, feats scale bytes (4 regs), MX8 temporaries (4), 128.0f
N_VGPR_SAVE = 193
Y = A0 + 0                    # 128 AGPRs; the head hidden vectors H0 / H1 are its halves
AR0, NA = A0 + 128, 6
AUX = A0 + 152                # 2 quads
HEAD = A0 + 160
N_AGPR = 176
IN_AUX, OUT_HEAD = 144, 128   # operands arrive / leave in VGPRs: aux fragments in v[144:151], head accumulator out in v[128:143]


def stage_list(auxs, heads=True):
    """the chunk list of FwdStream<AUXS> at SR_FEAT = 512 (mlp_layout.h) with this kernel's register assignment.  heads=False: the
    geometry variant, L1..L7 and the sigma tile (its units are numbered on from L7's: the feats pieces between them are jumped over)."""
    tiles, p, tno = [], 0, 0
    auxb = [AUX + 4 * a for a in range(auxs)]

    def dense(inp, ks, ntiles, epi, outbase, name, unit0=None):
        nonlocal p, tno
        for t in range(ntiles):
            b = [inp + 4 * k for k in range(ks)] + auxb
            out = [outbase + 8 * t + q for q in range(8)] if outbase is not None else None
            tiles.append(Tile(p, b, auxs, ACC[tno & 1], True, epi, out, f"{name}.{t}", None if unit0 is None else auxs + unit0 + t))
            p += len(b)
            tno += 1

    started = [False]

    def head(inp, with_aux, name):
        nonlocal p
        b = [inp + 4 * k for k in range(HS)] + (auxb if with_aux else [])
        tiles.append(Tile(p, b, auxs if with_aux else 0, HEAD, not started[0], None, None, name))
        started[0] = True
        p += len(b)

    H0, H1 = Y, Y + 4 * HS
    for l in range(7):
        dense(X if l % 2 == 0 else Y, KS, MT, "sin", Y if l % 2 == 0 else X, f"L{l + 1}", MT * (l + 1))
    if heads:
        dense(Y, KS, MT, "id", X, "feats", 8 * MT)
    dense(Y, KS, 1, "sigma", None, "sigma")
    if not heads:
        return tiles, p
    dense(X, KS, MTH, "sin", H0, "rgbh", 9 * MT)
    head(H0, False, "Hr")
    dense(X, KS, MTH, "sin", H1, "s1", 9 * MT + MTH)
    dense(H1, HS, MTH, "sin", H0, "s2", 9 * MT + 3 * MTH)
    dense(H0, HS, MTH, "sin", H1, "s3", 9 * MT + 4 * MTH)
    head(H1, False, "Hs")
    dense(X, KS, MTH, "sin", H0, "e1", 9 * MT + 2 * MTH)
    head(H0, True, "Hb")
    return tiles, p


class Core512(CoreBase):
    NW, SRC, VOFF_STEP, LABEL = NW, ("sb",), 0x1000, "5"
    MT, MTH, SAVE, AR0, NA, OUT_HEAD, SCALE_DWORDS = MT, MTH, 8, AR0, NA, OUT_HEAD, 4
    VL, VOFF, HEAD, SIG, TMP, SV, SOFF, KMAGIC, EB, MXT, K128 = VL, VOFF, HEAD, SIG, TMP, SV, SOFF, KMAGIC, EB, MXT, K128
    stage_list = staticmethod(stage_list)
    VARIANTS = ((dict(heads=False), "g"),)

    def __init__(self, auxs, R=144, PF=5, GROUP=1, FILL=None, ablate=(), save=0, heads=True):
        self.heads = heads
        if not heads:  # sigma's rows are fed from behind the feats rows of the one packed forward stream; no head accumulator to copy out
            assert save == 0, "the geometry core saves nothing"
            self.stage_list = lambda a: stage_list(a, heads=False)
            self.SRC_JUMP = feats_jump(stage_list(auxs)[0], NW)
            self.OUT_HEAD = None
        super().__init__(auxs, R, PF, GROUP, FILL, ablate, save)

    def preamble(self):
        for i in range(4 * self.auxs):
            self._e("accw", (AUX + i, IN_AUX + i), f"v_accvgpr_write_b32 {rn(AUX + i)}, v{IN_AUX + i}")

    def header(self):
        s = self.stats
        if not self.heads:
            row, rows = self.SRC_JUMP
            return ["// GENERATED by csrc/gen/fwd_core512.py by the build -- do not edit (its text is pinned by csrc/gen/variant_streams.sha256; tests/test_fwd_core_geometry.py).",
                    f"// width-512 geometry (trunk + sigma) forward core, AUXS = {self.auxs}: {s['mfma']} MFMAs, {s['instructions']} instructions, "
                    f"{s['barriers']} rendezvous, {s['rows']} LDS-DMA rows, ring of {self.R} pieces, A fragments {self.PF} ahead.",
                    f"// Reads the packed forward stream of the full core unchanged: behind ring row {row - 1} (L7's last) the source offset jumps over the",
                    f"// {rows} rows of feats pieces, so ring rows {row}.. are the sigma tile's.  No head accumulator: the one output is v{SIG}.",
                    "// Operands: %[sb] stream base (SGPR pair), %[wb] LDS ring address + wave * 1024, %[wave] wave index, %[m0save] scratch SGPR"]
        return ["// GENERATED by csrc/gen/fwd_core512.py -- do not edit (tests/test_fwd_core.py checks it is current).",
                f"// width-512 forward core, AUXS = {self.auxs}: {s['mfma']} MFMAs, {s['instructions']} instructions, {s['barriers']} rendezvous, "
                f"{s['rows']} LDS-DMA rows, ring of {self.R} pieces, A fragments {self.PF} ahead.",
                "// Operands: %[sb] stream base (SGPR pair), %[wb] LDS ring address + wave * 1024, %[wave] wave index, %[m0save] scratch SGPR"]

    @staticmethod
    def clobber_file(save=0):
        # operands: v[0:127] (X in), v[128:143] (head out), v[144:151] (aux in), SIG, VL, VOFF[, KMAGIC, SOFF, K128]
        regs = [f"v{r}" for r in list(range(ACC[1], ACC[1] + 16)) + list(TMP) if not IN_AUX <= r < IN_AUX + 8]
        if save:
            regs += [f"v{r}" for r in range(SV[0], N_VGPR_SAVE) if r not in (KMAGIC, SOFF, K128)]
        regs += [f"a{r}" for r in range(N_AGPR)]
        return ("// GENERATED by csrc/gen/fwd_core512.py: clobber list of the width-512 forward core\n" + ", ".join(f'"{r}"' for r in regs)
                + ', "memory", "scc"\n')


class Machine512(LaneModel):
    """the width-512 core on the shared lane model"""


STEM = "mlp_fwd512_core"  # csrc/<STEM>_a<auxs>[s<save> | g].inc

if __name__ == "__main__":
    sys.exit(main(Core512, STEM, __doc__, PF=5, GROUP=1, FILL=None))
