#!/usr/bin/env python3
"""Generator of the hand-placed gfx950 instruction stream of the dX kernel's TRUNK (csrc/mlp_bwd.inc, 8-bit workspaces, both widths).

The seven transposed trunk layers bL7 .. bL1 are two thirds of the data-gradient kernel (896 of its 1,308 MFMAs per 32-point tile):
    d a_{l-1} = W_l^T d pre_l  (8 output tiles x 16 k-steps),      d pre_{l-1} = d a_{l-1} * cos(2 pi phase_{l-1}),
d pre_{l-1} handed on in registers as bf16 B fragments and written to the dpre workspace as MX8 (codec8.h) for the weight-gradient kernel.
= autograd's backward through fc_net.2 .. fc_net.14 of SatNeRF.forward (models/satnerf.py:156-180) for every sample point.

Why now.  r03 tried this (tools/experiments/bwd_trunk_gen.py, last held by commit a4fc281) and measured no gain: its epilogue -- cvt +
scale + v_cos, multiply, pack, fma + cvt_pk_u8 per value: ~120 VALU per 16-MFMA tile -- costs ~556 cycles of VALU issue per tile against
512 matrix cycles, so two waves per SIMD were VALU-bound at ~70 cycles per MFMA however the stream was placed.  r04 shortened the codecs
(one v_perm per phase byte, v_max3 tree, one-rounding MX8 encode in v_pk_fma_f32 + byte gathers: 84 VALU, ~470 cycles per tile), which
moved the VALU time UNDER the matrix time -- but hipcc's schedule of that code (1,336 instructions per layer: 10.4 per MFMA, 26 SALU and
11 waits per tile, the epilogue of tile t - 1 in one lump after tile t's chain) gained 3 %.  With the epilogue spread over the MFMA gaps
the two pipes overlap, as they do in the forward cores.

The scheduler and the lane model are stream_common.py's (read that docstring first), shared with the three forward cores: ring, DMA
rows, rendezvous, A-fragment prefetch, the tagged load queue, the epilogue queue, text and command line.  This file states what is
particular to the trunk:
  * one plane, no ragged row, no prologue rows; 8 waves (width 256: two per SIMD) or 4 (512: one per SIMD, Y and the A ring in AGPRs);
  * the tile's saved phases (one 16-byte load per lane) are fetched two tiles ahead straight into registers (``gap_loads``); they sit in
    the same in-order queue as the DMA rows, and the epilogue waits for them by tag;
  * the epilogue of tile t - 1 sits in the gaps of tile t's MFMAs, FILL INSTRUCTIONS per gap, producers first so that no instruction
    waits for the transcendental unit: 16 perm | 16 cos | 8 pk_mul | 8 cvt_pk | max tree | exponent | 8 pk_fma | byte gathers | store;
  * per layer: the eight MX8 exponent bytes of a lane go to the scale unit, and their maximum over the wave (SDWA byte maxima, six DPP
    steps, one readlane) to the wave's cell of the exponent-maxima table (mlp_layout.h; the weight-gradient kernel's fp16 range fit);
  * at a layer boundary the whole queue is emptied, not only up to the operand's producers (``flush_producers``).
The arithmetic per value is exactly mlp_bwd.inc's (bpack / mx8_exponent / mx8_encode): the workspace bytes are bit-identical to the
compiler-scheduled kernel's, which tests/test_hip_backward.py asserts on the GPU; tests/test_bwd_core.py executes the stream on
``TrunkMachine`` (below), which also holds the hazards the assembler does not pad inside inline asm: trans -> VALU use (1 state), VALU
write -> MFMA operand (2), MFMA D -> VALU read, M0 write -> LDS-DMA (1), VALU write -> DPP read (2), VALU write -> v_readlane (1).

``python bwd_core.py`` writes csrc/mlp_bwd{,512}_trunk_a{1,2}.inc and csrc/mlp_bwd{,512}_trunk_clobbers.inc.

Registers (width 256): v[0:63] X, v[64:127] Y (d pre vectors, ping-pong: X is the statement's in/out operand), v[128:159] two accumulators,
v[160:183] A ring, v[184:199] phase ring (4 tiles), v[204:211] two store quads, v[212:213] scale bytes,
v214 max, v215 exponent, v[216:217] 2^(133-E) (low register used), v[218:219] the rounding constant, v220 = 0x43000000, v221 / v222 LDS
read bases, v223 stream offset, v224 phase offset, v225 dpre offset, v[226:229] temporaries, v230 LDS address of the wave's maxima cells, v[232:247] the tile's sixteen cosines / rounded MX8 values.
Scalar operands: %[sb] trunk part of the stream, %[wb] ring + wave * 1024, %[ab] activation workspace, %[db] dpre workspace, %[m0save].
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stream_common import A0, LANE, CoreBase, LaneModel, Tile, bf16_bits, bf16_to_f32, frag_to_f32, main, rn  # noqa: E402,F401


class Geo:
    """register map and sizes of one trunk width.  256: 8 waves x <= 256 VGPRs, both d pre vectors in VGPRs.  512: 4 waves x (256 VGPRs + 256
    AGPRs): a 32-point vector is 128 registers -- X in v[0:127], Y and the A-fragment ring in AGPRs (MFMA reads A / B from either file,
    ds_read_b128 writes either); what an epilogue produces for Y goes through v_accvgpr_write (as in gen/fwd_core512.py)."""

    def __init__(self, feat):
        assert feat in (256, 512)
        self.feat = feat
        self.KS, self.MT, self.NW = feat // 16, feat // 32, (8 if feat == 256 else 4)
        # g1: the stream starts one stage earlier, at bG1 ([d feats | d sigma_pre] -> d a_7: MT tiles of KS + 1 k-steps, the last reading the
        # d sigma_pre fragment XS).  Built, tested (tests/test_bwd_core.py runs either setting) and OFF: at width 256 the compiler cannot keep
        # the hand-over (68 pinned registers at two waves per SIMD) out of scratch -- 103 spilled registers in the stages before it, the
        # kernel 6 % SLOWER; at width 512 (no spills) 440 us against 426 with the trunk alone (r05, interleaved on one box)
        self.g1 = False
        self.LAYERS = 8 if self.g1 else 7
        self.R, self.GROUP, self.FILL = (96, 2, 6) if feat == 256 else (128, 1, 4)
        self.NEB = self.MT // 4                      # registers of a layer's exponent bytes
        if feat == 256:
            self.X, self.Y = 0, 64
            self.ACC = (128, 144)
            self.AR0 = 160
            self.PH0 = 184
            self.SV = (204, 208)
            self.EB = 212
            self.M, self.E, self.INV, self.MAGIC, self.K43 = 214, 215, 216, 218, 220
            self.VL0, self.VL1, self.VOFF, self.POFF, self.SOFF = 221, 222, 223, 224, 225
            self.T1 = 226
            self.VCELL = 230
            self.TT = 232
            self.N_VGPR, self.N_AGPR = 248, 0
            self.D8_SCALE, self.GROUPS_PER_UNIT = 94, 2
        else:
            self.X, self.Y = 0, A0
            self.ACC = (128, 144)
            self.AR0 = A0 + 128
            self.PH0 = 160
            self.TT = 176
            self.T1 = 192
            self.SV = (196, 200)
            self.EB = 204
            self.M, self.E, self.INV, self.MAGIC, self.K43 = 208, 209, 210, 212, 214
            self.VL0, self.VL1, self.VOFF, self.POFF, self.SOFF = 215, 216, 217, 218, 219
            self.VCELL = 220
            self.N_VGPR, self.N_AGPR = 222, 152
            self.D8_SCALE, self.GROUPS_PER_UNIT = 186, 1
        self.NA, self.NPH = 6, 4
        self.IN_REGS = (self.MAGIC, self.K43, self.VL0, self.VL1, self.VOFF, self.POFF, self.SOFF, self.VCELL)   # operands (wired by mlp_bwd.inc)
        self.XREGS = self.KS * 4                     # registers of a d pre vector
        # g1: the d sigma_pre B fragment = an in/out operand in the LAST quad of Y, which bG1's own last tile's epilogue overwrites only
        # after the layer's last MFMA has read it
        self.XS = self.Y + self.XREGS - 4
        self.L0 = 8 if self.g1 else 7                # `l` of the stream's first layer (8 = bG1)


S_SEL = ("s84", "s85", "s86", "s87")     # v_perm selectors of phase byte k: the byte lands in bits 8..15 of 0x43000000 (codec8.h phase8_rev)
S_B4A, S_B4B, S_MAX = "s88", "s89", "s90"  # bytes4() selectors (codec8.h), the wave maximum
STEM = {256: "mlp_bwd_trunk", 512: "mlp_bwd512_trunk"}


class Trunk(CoreBase):
    FEAT, SRC, SAVE, LABEL, WS, KEEP_FIRST = 256, ("sb",), 0, "", "db", ()
    ABLATIONS = {**CoreBase.ABLATIONS,   # (timing experiments, results wrong; the trunk's cvt_pk stay under noepi: the next layer reads them)
                 "noepi": {"perm", "cos", "pkmul", "max3", "max3r", "max3m", "max2", "mx", "pkfma", "b4a", "b4b"},
                 "nophase": {"phload", "poff"},
                 "nostore": {"store", "store2", "soff"},
                 "storelate": set()}     # (correct results) an ordering experiment, see emit_epi

    def __init__(self, auxs, feat=None, PF=5, ablate=(), save=0):
        self.g = g = Geo(feat or self.FEAT)
        self.NW, self.VOFF_STEP, self.AR0, self.NA, self.VL, self.VOFF, self.SOFF = g.NW, g.NW * 1024, g.AR0, g.NA, (g.VL0, g.VL1), g.VOFF, g.SOFF
        super().__init__(auxs, g.R, PF, g.GROUP, g.FILL, ablate, save)

    def stage_list(self, auxs):
        g, tiles, p = self.g, [], 0
        for ti in range(g.LAYERS * g.MT):    # layer l (8 = bG1, 7..1 = bL_l), tile t: X -> Y -> X ...; bG1's tiles end on the d sigma_pre fragment
            l, t = g.L0 - ti // g.MT, ti % g.MT
            inp, out = (g.X, g.Y) if (g.L0 - l) % 2 == 0 else (g.Y, g.X)
            b = [inp + 4 * k for k in range(g.KS)] + ([g.XS] if l == 8 else [])
            tiles.append(Tile(p, b, 0, g.ACC[ti & 1], True, "cos", out + 8 * t, f"bL{l}.{t}", g.MT * (l - 1) + t, "v_mfma_f32_32x32x16_bf16"))
            p += len(b)
        assert p % g.NW == 0                 # no ragged row: the statement has no %[wave] operand
        return tiles, p

    # ---- the phase loads: the same in-order queue as the DMA rows, tagged ("ph", tile) -----------------------------------------------
    def phase_load(self, ti):
        g = self.g
        unit = self.auxs + self.tiles[ti].save_unit   # layer l multiplies by cos(phase a_{l-1}): unit AUXS + MT (l - 1) + t
        delta = (unit - self.p_unit) * 1024
        self.p_unit = unit
        if delta:
            self._e("poff", (delta,), f"v_add_u32 v{g.POFF}, 0x{delta & 0xffffffff:x}, v{g.POFF}")
        r = g.PH0 + 4 * (ti % g.NPH)
        self._e("phload", (r, unit), f"global_load_dwordx4 v[{r}:{r + 3}], v{g.POFF}, %[ab] nt")
        self.vm.append(("ph", ti))

    def preamble(self):
        for k in range(4):
            self._e("sconst", (S_SEL[k],), f"s_mov_b32 {S_SEL[k]}, 0x{0x070c000c | (k << 8):08x}")
        self._e("sconst", (S_B4A,), f"s_mov_b32 {S_B4A}, 0x0c0c0400")
        self._e("sconst", (S_B4B,), f"s_mov_b32 {S_B4B}, 0x05040100")
        self.p_unit, self.late = 0, []       # unit POFF points at (the workspace offsets start at the tile's base); (storelate) held stores
        self.phase_load(0)
        self.phase_load(1)

    def gap_loads(self, ti, k):
        while self.late and self.late[0][0] <= self._barriers():   # (storelate) behind the next counted wait
            super().emit_epi("store", self.late.pop(0)[1])
        if k == 0 and ti + 2 < len(self.tiles):
            self.phase_load(ti + 2)

    # ---- the epilogue of one tile on the shared queue; an item is one instruction, or a group that must stay together ------------------
    def queue_epilogue(self, ti, g0):
        """tile ti: accumulator ACC[ti & 1], phases PH[ti % 4]; d pre = acc * cos(2 pi u / 256) -> two bf16 B fragments of the next
        layer's input vector, MX8 bytes -> the dpre workspace (codec8.h: bit for bit what bpack / mx8_exponent / mx8_encode compute)"""
        g, tile = self.g, self.tiles[ti]
        MT, TT, K43, EB, E, M, INV, MAGIC, T1 = g.MT, g.TT, g.K43, g.EB, g.E, g.M, g.INV, g.MAGIC, g.T1
        t, a, out, ph, sv = ti % MT, tile.acc, tile.out, g.PH0 + 4 * (ti % g.NPH), g.SV[ti & 1]

        def V(op, args, text, writes=()):
            self.epi_q.append([g0, "raw", ((op, args, text),), set(writes), a])

        def group(*parts):
            self.epi_q.append([g0, "raw", parts, set(), a])

        self.epi_q.append([g0, "waitph", (ti,), set(), a])
        # sixteen phase bytes -> sixteen temporaries (v_perm), sixteen cosines in place, eight packed multiplies into the accumulator, eight
        # packs: every consumer sits >= 8 instructions behind its producer -- the wave issues in order, so an instruction waiting for the
        # transcendental unit (or for a packed-fp32 result) also holds back the wave's next MFMA (measured: the pair-wise pipelined order
        # perm perm cos cos perm perm pk_mul ... ran the trunk at 58 cycles per MFMA slot against 40 without the epilogue)
        for gg in range(16):
            V("perm_ph", (TT + gg, ph + (gg >> 2), gg & 3), f"v_perm_b32 v{TT + gg}, v{K43}, v{ph + (gg >> 2)}, {S_SEL[gg & 3]}")
        for gg in range(16):
            V("cos", (TT + gg,), f"v_cos_f32 v{TT + gg}, v{TT + gg}")
        for gg in range(0, 16, 2):
            V("pkmul", (a + gg, TT + gg), f"v_pk_mul_f32 v[{a + gg}:{a + gg + 1}], v[{a + gg}:{a + gg + 1}], v[{TT + gg}:{TT + gg + 1}]")
        # the output vector in AGPRs: pack into the (now dead) cosine temporaries, then eight v_accvgpr_write
        pk = [out + q if out < A0 else TT + q for q in range(8)]
        for q in range(8):
            V("pk", (pk[q], a + 2 * q, a + 2 * q + 1), f"v_cvt_pk_bf16_f32 v{pk[q]}, v{a + 2 * q}, v{a + 2 * q + 1}", {pk[q]} if out < A0 else ())
        if out >= A0:
            for q in range(8):
                V("accw", (out + q, TT + q), f"v_accvgpr_write_b32 {rn(out + q)}, v{TT + q}", {out + q})
        # maximum of the 16 magnitudes (exact whatever the order): 8 instructions
        m, t1, t2 = M, T1, T1 + 1
        ab = lambda k: f"|v{a + k}|"  # noqa: E731
        V("max3", (m, a + 0, a + 1, a + 2), f"v_max3_f32 v{m}, {ab(0)}, {ab(1)}, {ab(2)}")
        V("max3", (t1, a + 3, a + 4, a + 5), f"v_max3_f32 v{t1}, {ab(3)}, {ab(4)}, {ab(5)}")
        V("max3", (t2, a + 6, a + 7, a + 8), f"v_max3_f32 v{t2}, {ab(6)}, {ab(7)}, {ab(8)}")
        V("max3r", (m, m, t1, t2), f"v_max3_f32 v{m}, v{m}, v{t1}, v{t2}")
        V("max3", (t1, a + 9, a + 10, a + 11), f"v_max3_f32 v{t1}, {ab(9)}, {ab(10)}, {ab(11)}")
        V("max3", (t2, a + 12, a + 13, a + 14), f"v_max3_f32 v{t2}, {ab(12)}, {ab(13)}, {ab(14)}")
        V("max3m", (t1, t1, t2, a + 15), f"v_max3_f32 v{t1}, v{t1}, v{t2}, {ab(15)}")
        V("max2", (m, m, t1), f"v_max_f32 v{m}, v{m}, v{t1}")
        # E = exponent of 1.0079 max|v| clamped to [6, 254]; 2^(133 - E)
        V("mx_e1", (m,), f"v_fmac_f32 v{m}, 0x3c000000, v{m}")
        V("mx_e2", (E, m), f"v_lshrrev_b32 v{E}, 23, v{m}")
        V("mx_e3a", (E,), f"v_max_u32 v{E}, 6, v{E}")
        V("mx_e3", (E,), f"v_min_u32 v{E}, 0xfe, v{E}")
        V("mx_e4", (INV, E), f"v_sub_u32 v{INV}, 0x104, v{E}")
        V("mx_e5", (INV,), f"v_lshlrev_b32 v{INV}, 23, v{INV}")
        if t & 3:
            V("mx_e6", (EB + (t >> 2), E, 8 * (t & 3), False), f"v_lshl_or_b32 v{EB + (t >> 2)}, v{E}, {8 * (t & 3)}, v{EB + (t >> 2)}")
        else:
            V("mx_e6", (EB + (t >> 2), E, 0, True), f"v_mov_b32 v{EB + (t >> 2)}, v{E}")
        # u = low mantissa byte of v * 2^(133 - E) + (1.5 * 2^23 + 128): two values per v_pk_fma_f32, three v_perm per four bytes; again
        # producers first (eight fmas into the sixteen temporaries), then the byte gathers
        for gg in range(0, 16, 2):
            V("pkfma", (TT + gg, a + gg), f"v_pk_fma_f32 v[{TT + gg}:{TT + gg + 1}], v[{a + gg}:{a + gg + 1}], v[{INV}:{INV + 1}], v[{MAGIC}:{MAGIC + 1}] op_sel_hi:[1,0,0]")
        for gg in range(0, 16, 4):
            V("b4a", (TT + gg, TT + gg + 1, TT + gg), f"v_perm_b32 v{TT + gg}, v{TT + gg + 1}, v{TT + gg}, {S_B4A}")
            V("b4a", (TT + gg + 2, TT + gg + 3, TT + gg + 2), f"v_perm_b32 v{TT + gg + 2}, v{TT + gg + 3}, v{TT + gg + 2}, {S_B4A}")
        for gg in range(0, 16, 4):
            V("b4b", (sv + gg // 4, TT + gg + 2, TT + gg), f"v_perm_b32 v{sv + gg // 4}, v{TT + gg + 2}, v{TT + gg}, {S_B4B}")
        self.epi_q.append([g0, "store", (sv, tile.save_unit, 4), set(), a])
        if t == MT - 1:
            grp = tile.save_unit // MT   # = l - 1.  The layer's MT scale bytes, then the largest of the lane's MT bytes and of the wave
            self.epi_q.append([g0, "scale", (grp,), set(), a])   # (lane 63 after the row broadcasts) -> cell `grp` of the wave's maxima
            c = T1
            dsts = [c, c + 1, c + 2, c + 3, TT, TT + 1, TT + 2, TT + 3]   # (the 512-wide layer has eight pair maxima)
            for n, (r, b0) in enumerate((r, b0) for r in range(g.NEB) for b0 in (0, 2)):
                V("bmax", (dsts[n], EB + r, b0, b0 + 1), f"v_max_u32_sdwa v{dsts[n]}, v{EB + r}, v{EB + r} dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_{b0} src1_sel:BYTE_{b0 + 1}")
            V("umax3", (c, c, c + 1, c + 2), f"v_max3_u32 v{c}, v{c}, v{c + 1}, v{c + 2}")
            V("umax", (c, c, c + 3), f"v_max_u32 v{c}, v{c}, v{c + 3}")
            if g.NEB > 2:
                V("umax3", (c + 1, TT, TT + 1, TT + 2), f"v_max3_u32 v{c + 1}, v{TT}, v{TT + 1}, v{TT + 2}")
                V("umax3", (c, c, c + 1, TT + 3), f"v_max3_u32 v{c}, v{c}, v{c + 1}, v{TT + 3}")
            for ctrl in ("row_shr:1", "row_shr:2", "row_shr:4", "row_shr:8", "row_bcast:15 row_mask:0xa", "row_bcast:31 row_mask:0xc"):
                group(("nop", (1,), "s_nop 1"),   # VALU write -> DPP read of the same register: two wait states
                      ("dppmax", (c, ctrl), f"v_max_u32_dpp v{c}, v{c}, v{c} {ctrl}" + ("" if "row_mask" in ctrl else " row_mask:0xf") + " bank_mask:0xf"))
            group(("nop", (0,), "s_nop 0"),       # VALU write -> v_readlane of the same register: one wait state (hipcc pads it too)
                  ("readlane", (c,), f"v_readlane_b32 {S_MAX}, v{c}, 63"))
            V("smov", (c + 1,), f"v_mov_b32 v{c + 1}, {S_MAX}")
            # one lane writes the cell; nothing else may issue while EXEC is narrowed (an A-fragment read would load one lane)
            group(("exec1", (), "s_mov_b64 exec, 1"), ("cell", (c + 1, grp), f"ds_write_b32 v{g.VCELL}, v{c + 1} offset:{4 * grp}"), ("execall", (), "s_mov_b64 exec, -1"))

    def emit_epi(self, kind, args):
        g = self.g
        if kind == "raw":
            for part in args:
                self._e(*part)
        elif kind == "waitph":
            if ("ph", args[0]) in self.vm:   # (else a rendezvous' wait has covered it)
                keep = self.vm_wait(("ph", args[0]))
                self._e("waitv", (keep,), f"s_waitcnt vmcnt({keep})")
        elif kind == "scale":   # group l - 1 -> unit kD8Scale + (l - 1) / groups per unit, its slot of the lane's 16 bytes
            unit, off = g.D8_SCALE + args[0] // g.GROUPS_PER_UNIT, g.MT * (args[0] % g.GROUPS_PER_UNIT)
            delta = (unit - self.cur_unit) * 1024
            self.cur_unit = unit
            self._e("soff", (delta,), f"v_add_u32 v{g.SOFF}, 0x{delta & 0xffffffff:x}, v{g.SOFF}")
            self._e("store2", (g.EB, unit, off), f"global_store_dwordx{g.NEB} v{g.SOFF}, v[{g.EB}:{g.EB + g.NEB - 1}], %[db]" + (f" offset:{off}" if g.GROUPS_PER_UNIT > 1 else ""))
        elif "storelate" in self.ablate and self._sync_done_for < len(self.tiles) - 1:
            # experiment (correct results): a tile's dpre store, due now, is held back until the gap behind the NEXT counted vmcnt wait (which
            # cannot tell stores from loads): it is then most of a tile old, not two MFMAs, when the following wait comes.  Its quad (SV, one of
            # two) is not written again before the epilogue after next; flush_acc and tail let none out later than that.
            self.late.append((self._barriers() + 1, args, self.at[0]))
        else:
            super().emit_epi(kind, args)

    def _barriers(self):
        return sum(1 for x in self.ins if x.op == "barrier")

    def fill_cost(self, n):
        return max(n, 1)    # FILL counts instructions here (the forward cores: items)

    def flush_acc(self, acc):
        while self.late and self.late[0][2] <= self.at[0] - 2:   # (storelate) before the store quad is rewritten
            super().emit_epi("store", self.late.pop(0)[1])
        return super().flush_acc(acc)

    def flush_producers(self, regs, m):
        """The last two B fragments of a layer's input are written by the previous layer's LAST epilogue, which is also the long one (scale
        store, wave maximum: ~30 instructions more).  When the new layer's first tile reaches them (k = KS - 2) the trunk empties the
        queue, not only up to the last cvt_pk as CoreBase would: the layer's workspace writes and its maxima cell are then complete, in
        program order, before anything of the next layer is produced, and the next epilogue (due one tile later) starts on an empty
        queue.  The s_nop 1 is the VALU write -> MFMA operand distance in case the producer was the last thing out."""
        ti, k = self.at
        if ti and ti % self.g.MT == 0 and k == self.g.KS - 2:
            n = len(self.epi_q)
            while self.epi_q:
                self._pop_epi()
            self._e("nop", (1,), "s_nop 1")
            return n
        assert not any(it[3] & regs for it in self.epi_q), ("B operand still in the queue", ti, k)
        return 0

    def tail(self):
        # the last tile's epilogue has no MFMAs to hide behind: XDL write -> VALU read of a 16-pass MFMA needs 18 wait states
        self._e("nop", (15,), "s_nop 15")
        self._e("nop", (3,), "s_nop 3")
        while self.epi_q:
            self._pop_epi()
        while self.late:
            super().emit_epi("store", self.late.pop(0)[1])
        self._e("waitall", (), "s_waitcnt vmcnt(0) lgkmcnt(0)")

    def header(self):
        s = self.stats
        return ["// GENERATED by csrc/gen/bwd_core.py -- do not edit (tests/test_bwd_core.py checks it is current).",
                f"// dX trunk, width {self.g.feat}, AUXS = {self.auxs}: {s['mfma']} MFMAs, {s['instructions']} instructions ({s['instructions'] / s['mfma']:.2f} per MFMA), "
                f"{s['barriers']} rendezvous, ring of {self.R} pieces, A fragments {self.PF} ahead, {self.FILL} epilogue instructions per gap"]

    @classmethod
    def clobber_file(cls, save=0):
        return clobber_file(cls.FEAT)


def clobber_file(feat=256):
    g = Geo(feat)
    regs = [r for r in range(g.XREGS if g.Y >= A0 else g.Y, g.N_VGPR) if r not in g.IN_REGS]
    sregs = list(S_SEL) + [S_B4A, S_B4B, S_MAX]
    skip_a = set(range(g.XS - A0, g.XS - A0 + 4)) if g.g1 and g.XS >= A0 else set()
    return (f"// GENERATED by csrc/gen/bwd_core.py: clobber list of the dX trunk statement, width {feat} (the X vector is in/out, the constants and offsets are inputs)\n"
            + ", ".join(f'"v{r}"' for r in regs) + ("".join(f', "a{r}"' for r in range(g.N_AGPR) if r not in skip_a)) + ", " + ", ".join(f'"{s_}"' for s_ in sregs)
            + ', "memory", "scc"\n')


def file_names(feat, auxs):
    return f"{STEM[feat]}_a{auxs}.inc", f"{STEM[feat]}_clobbers.inc"


# =================================================================================================================================
# The trunk on the shared lane model: its own ops, its initial registers, its hazard rules
# =================================================================================================================================
class TrunkMachine(LaneModel):
    """TrunkMachine(trunk, stream [unit, 64, 4], acts {unit: [64, 4]}, x0 [KS][4, 64]): one wave of the workgroup, the others in lock step.
    Besides LaneModel's checks: POFF addresses the unit loaded, no register is read while its (phase) load is in flight, VALU write ->
    DPP read (2 wait states) and -> v_readlane (1), nothing but the cell write issues while EXEC is narrowed."""

    def __init__(self, trunk, stream, acts, x0):
        super().__init__(trunk, stream)
        g = self.g = trunk.g
        self.acts, self.s, self.poff, self.scale_stores, self.cells, self._wrote = acts, {}, 0, {}, {}, {}
        for k in range(g.KS):
            self.v[g.X + 4 * k:g.X + 4 * k + 4] = x0[k]
        self.setf(g.MAGIC, np.full(64, 12583040.0))

    def _valu(self, dst, *srcs):
        self._valu_reads(*srcs)
        self._wrote[dst] = self._clk

    def _states_since_write(self, r):
        return self._clk - self._wrote.get(r, -9) - 1

    def own_op(self, op, a, ins):
        g, v, f = self.g, self.v, self.f
        if op == "sconst":
            self.s[a[0]] = int(ins.text.split(",")[1], 16)
        elif op == "poff":
            self.poff += a[0]
        elif op == "phload":
            assert self.poff == a[1] * 1024, ("POFF does not address the unit loaded", self.poff, a[1])
            self._valu_reads(*range(a[0], a[0] + 4))   # (the previous load of this quad has landed and been used)
            self._vm_issue(("reg", a[0], self.acts[a[1]].T.copy()))
        elif op == "waitv":
            self._vm_wait(a[0])
        elif op == "waitall":
            self._vm_wait(0), self._lgkm_wait(0)
        elif op == "perm_ph":
            dst, ph, k = a
            self._valu(dst, ph)
            v[dst] = 0x43000000 | (((v[ph] >> np.uint32(8 * k)) & 0xFF) << 8)
        elif op == "cos":
            self._valu(a[0], a[0])
            self._trans[a[0]] = self._pc
            self.setf(a[0], np.cos(2 * np.pi * (f(a[0]).astype(np.float64) - 128.0)))
        elif op == "pkmul":
            for j in range(2):
                self._valu(a[0] + j, a[0] + j, a[1] + j)
                self.setf(a[0] + j, f(a[0] + j) * f(a[1] + j))
        elif op in ("max3", "max3r", "max3m", "max2"):
            self._valu(a[0], *a[1:])
            vals = [np.abs(f(r)) if op == "max3" or (op == "max3m" and r == a[3]) else f(r) for r in a[1:]]
            self.setf(a[0], np.maximum.reduce(vals))
        elif op == "pkfma":
            for j in range(2):
                self._valu(a[0] + j, a[1] + j, g.INV, g.MAGIC)
                self.setf(a[0] + j, f(a[1] + j).astype(np.float64) * f(g.INV).astype(np.float64) + f(g.MAGIC).astype(np.float64))
        elif op == "b4a":   # [s1.b0, s0.b0, 0, 0]
            self._valu(a[0], a[1], a[2])
            v[a[0]] = (v[a[2]] & 0xFF) | ((v[a[1]] & 0xFF) << 8)
        elif op == "b4b":   # [s1.b0, s1.b1, s0.b0, s0.b1]
            self._valu(a[0], a[1], a[2])
            v[a[0]] = (v[a[2]] & 0xFFFF) | ((v[a[1]] & 0xFFFF) << 16)
        elif op == "store2":
            assert self.soff == a[1] * 1024, ("SOFF does not address the unit stored", self.soff, a[1])
            self.scale_stores[(a[1], a[2])] = v[a[0]:a[0] + g.NEB].T.copy()
        elif op == "bmax":
            self._valu(a[0], a[1])
            v[a[0]] = np.maximum((v[a[1]] >> np.uint32(8 * a[2])) & 0xFF, (v[a[1]] >> np.uint32(8 * a[3])) & 0xFF)
        elif op in ("umax3", "umax"):
            self._valu(a[0], *a[1:])
            v[a[0]] = np.maximum.reduce([v[r] for r in a[1:]])
        elif op == "dppmax":   # row_shr:n within rows of 16; row_bcast:15 into rows 1, 3; row_bcast:31 into rows 2, 3
            assert self._states_since_write(a[0]) >= 2, ("VALU write -> DPP read needs two wait states", ins.text)
            self._valu(a[0], a[0])
            if a[1].startswith("row_shr:"):
                n = int(a[1].split(":")[1])
                src = np.where((LANE & 15) >= n, LANE - n, LANE)
            elif a[1].startswith("row_bcast:15"):
                src = np.where((LANE >> 4) & 1, (LANE & ~15) - 1, LANE)
            else:
                src = np.where(LANE >= 32, 31, LANE)
            v[a[0]] = np.maximum(v[a[0]], v[a[0]][src])
        elif op == "readlane":
            assert self._states_since_write(a[0]) >= 1, ("VALU write -> v_readlane needs one wait state", ins.text)
            self.s[S_MAX] = int(v[a[0]][63])
        elif op == "smov":
            self._valu(a[0])
            v[a[0]] = self.s[S_MAX]
        elif op == "exec1":
            self._exec1 = True
        elif op == "cell":
            assert self._exec1
            self.cells[a[1]] = int(v[a[0]][0])
            self.pending.append((None, None, None, None))   # an LDS write in the in-order queue of the reads
        elif op == "execall":
            self._exec1 = False
        else:
            super().own_op(op, a, ins)


if __name__ == "__main__":
    sys.exit(max(main(type(f"Trunk{feat}", (Trunk,), {"FEAT": feat}), STEM[feat], __doc__, PF=5) or 0 for feat in STEM))
