"""What the generators of the ring-fed MFMA streams share -- the forward cores (fwd_core.py, fwd_core3.py, fwd_core512.py) and the dX trunk
(bwd_core.py): the instruction record, the unified register naming, the bf16 / fragment helpers, ONE scheduler (``CoreBase``) and ONE
lane-accurate CPU model (``LaneModel``).  A core states only what is different about it (register map, stage list, waves per workgroup,
requests per DMA row, MFMAs per k-step, its epilogue recipe, its other loads, head and tail, file header and clobber list); every core's
stream is held to the same set of checks.

Structure of a core (one wave = 32 points; mlp_layout.h for the stream format):
  * k-step i of the wave consumes unit i of the stream (one 1-KiB A fragment per plane = one k-step of one 32-row output tile).  Units
    reach LDS by LDS-DMA "rows" of NW units (REQS 1-KiB requests per wave and row) into a flat ring of R units; ``sync`` points (counted
    vmcnt + s_barrier) every GROUP tiles make a group's units visible, after which the rows whose ring slots are free are requested.
  * A fragments are fetched PF k-steps ahead (ds_read_b128 into a ring of register quads, counted lgkmcnt before each MFMA).
  * loads retire in order, so every vmcnt is a count of the LOADS (DMA requests, a core's own register loads) issued behind the one
    waited for, read off one tagged queue; stores are left out (they may complete out of order: a wait can only get longer).
  * the epilogue of tile t-1 is spread over the gaps of tile t's MFMAs, starting two MFMAs after the tile's last one (XDL write -> VALU
    read: LaneModel.XDL_NOPS wait states).
  * hazards the assembler does not pad inside inline asm are handled here and checked by the model: trans -> VALU use (1 state), VALU
    write -> MFMA operand (2 states), MFMA D -> VALU read (>= 2 MFMAs later), M0 write -> LDS-DMA (1 state); the trunk's model adds
    VALU write -> DPP read (2) and -> v_readlane (1); nothing but the trunk's cell write issues while EXEC is narrowed.
"""
from __future__ import annotations

import os

import numpy as np

A0 = 256                     # unified register numbering: 0..255 = v, 256..511 = a (one wave per SIMD uses both files)


def rn(r, n=1):
    f, i = ("v", r) if r < A0 else ("a", r - A0)
    return f"{f}{i}" if n == 1 else f"{f}[{i}:{i + n - 1}]"


class Ins:
    __slots__ = ("op", "a", "text")

    def __init__(self, op, a, text):
        self.op, self.a, self.text = op, a, text


def aux_steps(tau):
    return (8 + ((tau + 7) // 8) * 8 + 15) // 16


class Tile:
    """One chunk of the stream = one output tile: units [p0, p0 + n), the MFMA order, the B operand of every k-step (a register quad,
    or a (hi, lo) pair of quads in the parity mode), what happens to the accumulator afterwards."""

    def __init__(self, p0, bregs, n_aux, acc, c0, epi, out, name, save_unit=None, op="MF"):
        self.op = op  # MF = the mode's MFMA (bf16 / f16 operands), MF0 = always bf16 (fc_net.0's split operands), or a spelled-out opcode
        self.save_unit = save_unit  # saving cores: workspace unit (1 KiB per tile of 32 points) of this tile's values, or None
        self.p0, self.n = p0, len(bregs)
        # MFMA order: aux k-steps first (their B operand is always ready: one more gap for the producing epilogue)
        order = list(range(self.n - n_aux, self.n)) + list(range(self.n - n_aux))
        self.pieces = [p0 + k for k in order]
        self.bregs = [bregs[k] for k in order]
        self.acc, self.c0, self.epi, self.out, self.name = acc, c0, epi, out, name


def feats_jump(tiles, nw):
    """SRC_JUMP of a variant that leaves the feats tiles out of the full stage list `tiles`: (first ring row of what follows them, rows
    of feats pieces).  Every trunk layer is whole DMA rows, so the jump is row-aligned."""
    p0 = next(t.p0 for t in tiles if t.name == "feats.0")
    p1 = next(t.p0 for t in tiles if t.name == "sigma.0")
    assert p0 % nw == 0 and p1 % nw == 0, "the feats pieces are not whole DMA rows"
    return p0 // nw, (p1 - p0) // nw


# =================================================================================================================================
# The scheduler
# =================================================================================================================================
class CoreBase:
    """A subclass sets: NW (waves per workgroup = units per DMA row), PRE_ROWS (rows the kernel prologue wrote into the ring), SRC (the
    stream operand of each of a row's requests: one per plane), VOFF_STEP, LABEL, SYNC_AHEAD, PK, MT / MTH (tiles of a trunk / head
    layer), SAVE, AR0 / NA, OUT_HEAD and its register map (VL, VOFF, SIG, TMP, SV, SOFF, KMAGIC, EB, MXT, K128, SCALE_DWORDS), and defines
    stage_list(), header(), clobber_file() (and preamble() / a_frags() / mfmas() / queue_dense() / emit_epi() / gap_loads() / fill_cost() /
    flush_producers() / tail() where it differs)."""

    PRE_ROWS = 0          # rows 0 .. PRE_ROWS - 1: in the ring before the stream starts, never requested
    SYNC_AHEAD = False    # the rendezvous a prefetch needs goes in front of the k-step's first MFMA (True) or into the gap behind it
    PK = "PK"             # the cvt_pk mnemonic (a macro where the kernel chooses bf16 / f16)
    OUT_HEAD = None       # VGPRs the head accumulator is copied to at the end when it lives in AGPRs
    TMP = ()
    WS = "ab"             # the workspace operand of the stores
    KEEP_FIRST = ("m0", "dma", "voff")   # what `nodma` leaves in front of the first rendezvous (the first reads need those requests)
    SRC_JUMP = None       # (row, rows): ring rows >= row are fed from stream rows `rows` further on (a variant that leaves stages out)
    VARIANTS = ()         # (constructor keywords, file suffix) of the further SAVE = 0 streams main() writes
    heads = True          # False (an instance attribute of the cores that offer it): the stream ends with the sigma tile, see tail()

    def __init__(self, auxs, R, PF, GROUP, FILL, ablate, save):
        assert R % self.NW == 0 and R * 1024 * len(self.SRC) <= 65536 * len(self.VL) and PF + 1 <= self.NA and save in (0, self.SAVE)
        if FILL is None:
            FILL = 3 if save else 2  # epilogue instructions per MFMA gap (a saving tile's epilogue has 42 instead of 24)
        self.auxs, self.R, self.PF, self.GROUP, self.FILL, self.save = auxs, R, PF, GROUP, FILL, save
        self.ablate = set(ablate)  # timing experiments only (results are wrong), see text()
        self.tiles, self.n_pieces = self.stage_list(auxs)
        self.ins = []
        self.stats = {}
        self._build()

    # ---- emission helpers ------------------------------------------------------------------------------------------------------
    def _e(self, op, a, text):
        self.ins.append(Ins(op, a, text))

    def mfma(self, acc, areg, breg, c0, op):
        c = "0" if c0 else rn(acc, 16)
        self._e("mfma", (acc, areg, breg, c0), f"{op} {rn(acc, 16)}, {rn(areg, 4)}, {rn(breg, 4)}, {c}")

    def src_row(self, j):
        """the row of the packed stream that ring row j is fed from"""
        return j if self.SRC_JUMP is None or j < self.SRC_JUMP[0] else j + self.SRC_JUMP[1]

    def dsread(self, dst, slot, plane):
        unit = 1024 * len(self.SRC)          # a ring slot holds every plane of its unit; one read base register per 64 KiB of ring
        per_base = 65536 // unit
        self._e("dsread", (dst, slot, plane), f"ds_read_b128 {rn(dst, 4)}, v{self.VL[slot // per_base]} offset:{(slot % per_base) * unit + 1024 * plane}")

    def waitl(self, n):
        self._e("waitl", (n,), f"s_waitcnt lgkmcnt({n})")

    def dma_request(self, j, plane, partial):
        """request `plane` of row j: wave w fetches that plane of unit NW j + w into ring slot (NW j + w) % R from the stream offset VOFF
        holds (w * 1024 + lane * 16 + (src_row(j) - PRE_ROWS) * NW * 1024; advanced behind the row's last request).  A ragged last row (waves >=
        partial skip it: s_cbranch around the requests, SCC from s_cmp) is emitted whole under one branch."""
        planes = len(self.SRC)
        imm = ((self.NW * j) % self.R) * 1024 * planes + 1024 * plane
        label = f".Lskip{self.LABEL}_row{j}_%="
        if partial is not None and plane == 0:
            self._e("dma_pred", (j, partial), f"s_cmp_lt_u32 %[wave], {partial}")
            self._e("dma_br", (j,), f"s_cbranch_scc0 {label}")
        self._e("m0", (j, plane), f"s_add_u32 m0, %[wb], {imm}")
        self._e("nop", (0,), "s_nop 0")
        self._e("dma", (j, plane, partial), f"global_load_lds_dwordx4 v{self.VOFF}, %[{self.SRC[plane]}]")
        self.vm.append(("row", j))
        if plane == planes - 1:
            if partial is not None:
                self._e("label", (j,), f"{label}:")
            rows = self.src_row(j + 1) - self.src_row(j)  # 1, or past the stages a variant leaves out
            self._e("voff", () if rows == 1 else (rows,), f"v_add_u32 v{self.VOFF}, 0x{rows * self.VOFF_STEP:x}, v{self.VOFF}")

    # ---- the loads in flight, oldest first: ("row", j) per DMA request, a core's own tags for its register loads --------------------------
    def vm_wait(self, tag):
        """the vmcnt that lets the newest load tagged `tag` and everything older land: the loads issued behind it.  A wave that skips the
        ragged last row has that row's requests fewer in flight, and the count must hold for it too."""
        if tag in self.vm:
            del self.vm[:len(self.vm) - self.vm[::-1].index(tag)]
        vm = sum(1 for t in self.vm if t != ("row", self.partial_row))
        assert vm <= 63
        return vm

    # ---- ring / DMA-row bookkeeping ------------------------------------------------------------------------------------------------
    def allow_rows(self, free_below):
        # ring slots of units < free_below may be overwritten: row j writes units [NW j, NW j + NW) over units NW j - R ...
        j = self.rows_issued + len(self.pending_rows)
        while j < self.n_rows and self.NW * (j + 1) - self.R <= free_below:
            self.pending_rows.append(j)
            j += 1

    def emit_request(self):
        """the next request of the oldest allowed row"""
        j = self.pending_rows[0]
        part = self.partial_n if j == self.partial_row else None
        self.dma_request(j, self._plane, part)
        while part is not None and self._plane + 1 < len(self.SRC):  # ragged row: every request under the one branch
            self._plane += 1
            self.dma_request(j, self._plane, part)
        self._plane = (self._plane + 1) % len(self.SRC)
        if self._plane == 0:
            self.pending_rows.pop(0)
            self.rows_issued += 1

    def sync_for(self, first_tile):
        T, NW = self.tiles, self.NW
        last = min(first_tile + self.GROUP, len(T)) - 1
        need = (T[last].p0 + T[last].n + NW - 1) // NW  # rows 0 .. need-1 must have landed
        # every row allowed so far is emitted before the wait (program order = count order)
        while self.pending_rows:
            self.emit_request()
        assert self.rows_issued >= need, (first_tile, self.rows_issued, need)
        vm = self.vm_wait(("row", need - 1))
        self._e("sync", (vm, need), f"s_waitcnt vmcnt({vm})")
        self._e("barrier", (), "s_barrier")

    def reads_for(self, i, cur_tile=None):
        """the ds_reads of k-step i as (register quad, ring slot, plane); a rendezvous first when i opens a group of tiles.  The barrier
        proves every wave has issued the MFMAs in front of it: all tiles before the current one are consumed, their slots are free."""
        T, G = self.tiles, self.GROUP
        ti, k = self.ksteps[i]
        if ti > self._sync_done_for and ti % G == 0 and k == 0:
            self._sync_done_for = ti + G - 1
            last = min(ti + G, len(T)) - 1
            if T[last].p0 + T[last].n > self.PRE_ROWS * self.NW:  # (the prologue's rows are in the ring already)
                self.sync_for(ti)
                if cur_tile is not None:
                    self.allow_rows(T[cur_tile].p0)
        slot = T[ti].pieces[k] % self.R
        return [(reg, slot, plane) for reg, plane in self.a_frags(i)]

    # ---- the epilogue queue: entries [earliest MFMA index, kind, args, registers written, accumulator read or None] ---------------------
    def queue_epilogue(self, ti, g0):
        t = self.tiles[ti]
        if t.epi == "sigma":
            self.epi_q.append([g0, "mov", (self.SIG, t.acc), {self.SIG}, t.acc])
        else:
            self.queue_dense(ti, g0)

    def queue_dense(self, ti, g0):
        """plain sin / identity epilogue of a single-plane core, with the PHASE8 / MX8 saves of the training forward"""
        t = self.tiles[ti]
        q_, a, sin = self.epi_q, t.acc, t.epi == "sin"
        to_agpr = t.out[0] >= A0

        def out_pk(q):  # cvt_pk of values 2 q, 2 q + 1 into the output vector (through a temporary when it lives in AGPRs)
            d = self.TMP[q & 3] if to_agpr else t.out[q]
            q_.append([g0, "pk", (d, a + 2 * q, a + 2 * q + 1), set() if to_agpr else {d}, a])
            if to_agpr:
                q_.append([g0, "accw", (t.out[q], d), {t.out[q]}, None])

        def phase(g):
            q_.append([g0, "phase", (sv + (g >> 2), g & 3, a + g), set(), a])

        if self.save and t.save_unit is not None:
            sv = self.SV[self.n_saves & 1]
            self.n_saves += 1
            if sin and "phasefirst" in self.ablate and ti % self.GROUP == self.GROUP - 1:  # (its epilogue runs in a tile that holds no counted wait)
                # experiment (correct results): all 16 PHASE8 bytes first, the store right behind them -- it is then ~8 MFMAs older when
                # the next counted vmcnt wait (which cannot tell stores from LDS-DMA loads) comes -- then the sines and packs
                for g in range(16):
                    phase(g)
                q_.append([g0, "store", (sv, t.save_unit), set(), None])
                for q in range(8):
                    for g in (2 * q, 2 * q + 1):
                        q_.append([g0, "sin", (a + g,), set(), a])
                    if q > 0:
                        out_pk(q - 1)
                out_pk(7)
            elif sin:
                # PHASE8: byte = low mantissa byte of (pre-activation + 1.5 * 2^15), written straight into its place of the store quad
                # by an SDWA add BEFORE the value's sin overwrites the accumulator; cvt_pk one pair behind (trans -> VALU use)
                for q in range(8):
                    for g in (2 * q, 2 * q + 1):
                        phase(g)
                        q_.append([g0, "sin", (a + g,), set(), a])
                    if q > 0:
                        out_pk(q - 1)
                q_.append([g0, "store", (sv, t.save_unit), set(), None])
                out_pk(7)
            else:
                # MX8: E = exponent of 1.0079 max|v| clamped to [6, 254]; u = cvt_pk_u8(v * 2^(133 - E) + 128); byte t of EB = E
                tt = t.save_unit - (self.auxs + 8 * self.MT)
                q_.append([g0, "mx_max", (a, 0, True), set(), a])
                for g in range(2, 16, 2):
                    q_.append([g0, "mx_max", (a, g, False), set(), a])
                q_.append([g0, "mx_exp", (tt,), set(), None])
                for g in range(16):
                    q_.append([g0, "mx_q", (sv + (g >> 2), g & 3, a + g), set(), a])
                q_.append([g0, "store", (sv, t.save_unit), set(), None])
                for q in range(8):
                    out_pk(q)
                if tt == self.MT - 1:
                    q_.append([g0, "store_scale", (self.auxs + 9 * self.MT + 5 * self.MTH,), set(), None])
            return
        # s0 s1 s2 c0 s3 s4 c1 ...: every cvt_pk is separated from its second sin by one instruction (trans -> VALU use)
        if sin:
            q_.append([g0, "sin", (a + 0,), set(), a])
            q_.append([g0, "sin", (a + 1,), set(), a])
        for q in range(8):
            if sin and q < 7:
                q_.append([g0, "sin", (a + 2 * q + 2,), set(), a])
            d = self.TMP[q & 3] if to_agpr else t.out[q]
            q_.append([g0, "pk", (d, a + 2 * q, a + 2 * q + 1), set() if to_agpr else {d}, a])
            if sin and q < 7:
                q_.append([g0, "sin", (a + 2 * q + 3,), set(), a])
            if to_agpr:
                q_.append([g0, "accw", (t.out[q], d), {t.out[q]}, None])

    def _after_trans(self, *srcs):
        for s in srcs:  # trans -> VALU use: one instruction in between
            if s in self.trans_at and len(self.ins) - self.trans_at[s] < 2:
                self._e("nop", (0,), "s_nop 0")

    def emit_epi(self, kind, args):
        n = len(self.ins)
        if kind == "sin":
            self._e("sin", args, f"v_sin_f32 v{args[0]}, v{args[0]}")
            self.trans_at[args[0]] = n
        elif kind == "pk":
            d, s0, s1 = args
            self._after_trans(s0, s1)
            self._e("pk", args, f"{self.PK} v{d}, v{s0}, v{s1}")
        elif kind == "accw":
            self._e("accw", args, f"v_accvgpr_write_b32 {rn(args[0])}, v{args[1]}")
        elif kind == "mov":
            self._e("mov", args, f"v_mov_b32 v{args[0]}, v{args[1]}")
        elif kind == "phase":
            d, byte, src = args
            self._e("phase", args, f"v_add_f32_sdwa v{d}, v{src}, v{self.KMAGIC} dst_sel:BYTE_{byte} dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD")
        elif kind in ("store", "store_scale"):  # a tile's quad (non-temporal), or the feats scale bytes
            reg, unit, ndw = (args[0], args[1], 4) if kind == "store" else (self.EB, args[0], self.SCALE_DWORDS)
            assert reg % 2 == 0  # register tuples are 64-bit aligned on gfx950
            delta = (unit - self.cur_unit) * 1024
            self.cur_unit = unit
            self._e("soff", (delta,), f"v_add_u32 v{self.SOFF}, 0x{delta & 0xffffffff:x}, v{self.SOFF}")
            self._e("store", (reg, unit, ndw), f"global_store_dwordx{ndw} v{self.SOFF}, {rn(reg, ndw)}, %[{self.WS}]" + (" nt" if kind == "store" else ""))
        elif kind == "mx_max":
            a, g, first = args
            m = self.MXT
            if first:
                self._e("mx_max", (m, a + g, a + g + 1, None), f"v_max_f32 v{m}, |v{a + g}|, |v{a + g + 1}|")
            else:
                self._e("mx_max", (m, a + g, a + g + 1, m), f"v_max3_f32 v{m}, |v{a + g}|, |v{a + g + 1}|, v{m}")
        elif kind == "mx_exp":
            (tt,) = args
            m, e, inv, eb = self.MXT, self.MXT + 1, self.MXT + 2, self.EB + (args[0] >> 2)
            self._e("mx_e1", (m,), f"v_fmac_f32 v{m}, 0x3c000000, v{m}")                 # m = 2^-7 m + m (one rounding; VOP2 takes the literal)
            self._e("mx_e2", (e, m), f"v_lshrrev_b32 v{e}, 23, v{m}")
            self._e("mx_e3a", (e,), f"v_max_u32 v{e}, 6, v{e}")                          # clamp to [6, 254]
            self._e("mx_e3", (e,), f"v_min_u32 v{e}, 0xfe, v{e}")
            self._e("mx_e4", (inv, e), f"v_sub_u32 v{inv}, 0x104, v{e}")                 # 260 - E
            self._e("mx_e5", (inv,), f"v_lshlrev_b32 v{inv}, 23, v{inv}")                # 2^(133 - E)
            if tt & 3:
                self._e("mx_e6", (eb, e, 8 * (tt & 3), False), f"v_lshl_or_b32 v{eb}, v{e}, {8 * (tt & 3)}, v{eb}")
            else:
                self._e("mx_e6", (eb, e, 0, True), f"v_mov_b32 v{eb}, v{e}")
        elif kind == "mx_q":
            d, byte, src = args
            tmp, inv = self.MXT + 3, self.MXT + 2
            self._e("mx_q1", (tmp, src, inv), f"v_fma_f32 v{tmp}, v{src}, v{inv}, v{self.K128}")   # v * 2^(133 - E) + 128
            self._e("mx_q2", (d, tmp, byte), f"v_cvt_pk_u8_f32 v{d}, v{tmp}, {byte}, v{d}")
        else:
            raise KeyError(kind)

    def _pop_epi(self):
        _, kind, args, writes, _ = self.epi_q.pop(0)
        n0 = len(self.ins)
        self.emit_epi(kind, args)
        for r in writes:
            self.written_at[r] = len(self.ins) - 1
        return len(self.ins) - n0

    def flush_producers(self, regs, m):
        """MFMA m is about to read `regs`: everything in the queue up to the last instruction that writes one of them must be emitted now"""
        last = max((qi for qi, it in enumerate(self.epi_q) if it[3] & regs), default=-1)
        for _ in range(last + 1):
            assert self.epi_q[0][0] <= m, ("epilogue needed before its accumulator is ready", self.epi_q[0], m)
            self._pop_epi()
        return last + 1

    def flush_acc(self, acc):
        """a tile is about to start on accumulator `acc`: the epilogue that still reads it must be out first"""
        last = max((qi for qi, it in enumerate(self.epi_q) if it[4] == acc), default=-1)
        for _ in range(last + 1):
            self._pop_epi()
        return last + 1

    def operand_ready(self, breg):
        # VALU write -> MFMA read of the B operand: 2 wait states
        dist = len(self.ins) - max(self.written_at.get(r, -10) for r in range(breg, breg + 4))
        if dist < 3:
            self._e("nop", (3 - dist,), f"s_nop {3 - dist}")

    def preamble(self):
        """what stands in front of the first DMA request: moves of operands that arrive in VGPRs and live in AGPRs, constants, first loads"""

    def gap_loads(self, ti, k):
        """a core's own loads in the gap behind k-step k of tile ti, in front of the gap's DMA request"""

    def fill_cost(self, n):
        """what an epilogue item that emitted n instructions counts against FILL"""
        return 1

    def tail(self):
        """behind the last MFMA: the head accumulator is read right behind it (by compiler code or here)"""
        if not self.heads:  # the last tile is sigma's: its move to SIG waits out XDL write -> VALU read (LaneModel.XDL_NOPS)
            self._e("nop", (15,), "s_nop 15")
            self._e("nop", (3,), "s_nop 3")
            while self.epi_q:
                self._pop_epi()
            return
        assert not self.epi_q
        self._e("nop", (15,), "s_nop 15")
        if self.OUT_HEAD is not None:
            self._e("nop", (3,), "s_nop 3")
            for g in range(16):
                self._e("accr", (self.OUT_HEAD + g, self.HEAD + g), f"v_accvgpr_read_b32 v{self.OUT_HEAD + g}, {rn(self.HEAD + g)}")

    def a_frags(self, i):
        """(register quad, plane) of the A fragments of k-step i, in read order"""
        return [(self.AR0 + 4 * (i % self.NA), 0)]

    def mfmas(self, t, k, aregs):
        """(A quad, B quad) of the MFMAs of k-step k of tile t"""
        return [(aregs[0], t.bregs[k])]

    # ---- the schedule ----------------------------------------------------------------------------------------------------------
    def _build(self):
        T, PF, NW = self.tiles, self.PF, self.NW
        self.ksteps = ks = [(ti, k) for ti, t in enumerate(T) for k in range(t.n)]
        N = len(ks)
        assert N == self.n_pieces
        self.n_rows = (N + NW - 1) // NW
        self.partial_row = self.n_rows - 1 if N % NW else None
        self.partial_n = N % NW
        self.rows_issued = self.PRE_ROWS
        self.pending_rows, self._plane = [], 0   # rows allowed but not yet (wholly) requested, plane of the next request
        self.vm = []
        self.epi_q, self.n_saves, self.cur_unit = [], 0, 0
        self.written_at = {}   # register -> index in self.ins of the VALU instruction that last wrote it (B operands only)
        self.trans_at = {}     # VGPR -> index of a v_sin that wrote it
        self._sync_done_for = -1

        # ---- preamble: request the first rows, make the first group visible, start the A-fragment pipeline
        self._e("savem0", (), "s_mov_b32 %[m0save], m0")
        self.preamble()
        self.allow_rows(0)
        for i in range(min(PF, N)):
            for rd in self.reads_for(i):
                self.dsread(*rd)
        m = forced = 0  # MFMA index, epilogue instructions emitted ahead of their gap
        for i in range(N):
            self.at = ti, k = ks[i]
            t = T[ti]
            aregs = [reg for reg, _ in self.a_frags(i)]
            ops = self.mfmas(t, k, aregs)  # (A quad, B quad) of the k-step's MFMAs
            if k == 0 and t.c0:
                forced += self.flush_acc(t.acc)
            forced += self.flush_producers({r for _, b in ops for r in range(b, b + 4)}, m)
            # the reads of k-step i + PF go into this k-step's gaps, behind the rendezvous they may need
            reads = self.reads_for(i + PF, ti) if self.SYNC_AHEAD and i + PF < N else []
            ahead = len(aregs) * min(PF - 1, N - 1 - i)  # reads of later k-steps already issued when this k-step starts
            in_gaps, prev = 0, None
            for p, (areg, breg) in enumerate(ops):
                self.operand_ready(breg)
                if areg != prev:  # everything up to this fragment: the k-step's later fragments and the later k-steps may be in flight
                    self.waitl(len(aregs) - 1 - aregs.index(areg) + ahead + in_gaps)
                    prev = areg
                self.mfma(t.acc, areg, breg, t.c0 and k == 0 and p == 0, t.op)
                m += 1
                if k == t.n - 1 and p == len(ops) - 1 and t.epi is not None:
                    self.queue_epilogue(ti, m + 1)
                # ---- gap
                if p == 0 and not self.SYNC_AHEAD and i + PF < N:
                    reads = self.reads_for(i + PF, ti)
                if p < len(reads):
                    self.dsread(*reads[p])
                    in_gaps += 1
                if p == len(ops) - 1:
                    self.gap_loads(ti, k)
                    if self.pending_rows:
                        self.emit_request()
                n = 0
                while self.epi_q and n < self.FILL and self.epi_q[0][0] <= m - 1:
                    n += self.fill_cost(self._pop_epi())
        assert not self.pending_rows and self.rows_issued == self.n_rows
        self.tail()
        self._e("restm0", (), "s_mov_b32 m0, %[m0save]")
        self.stats = dict(mfma=m, instructions=len(self.ins), forced_epilogue=forced, rows=self.n_rows,
                          barriers=sum(1 for x in self.ins if x.op == "barrier"), nops=sum(1 for x in self.ins if x.op == "nop"))

    # ---- text --------------------------------------------------------------------------------------------------------------------
    ABLATIONS = {  # timing experiments: instruction kinds left out of the text, by family (the op name up to its first underscore)
        "nodma": {"m0", "dma", "voff", "label"},
        "nobarrier": {"barrier"},
        "nosync": {"barrier", "sync"},
        "noepi": {"sin", "pk", "fract", "shl", "and", "sub"},
        "noread": {"dsread", "waitl"},
        "nowaitl": {"waitl"},
        "nonop": {"nop"},
        "nostore": {"store", "soff", "pknorm"},  # (saving cores) the workspace stores and their address steps
        # (saving cores) every store of a wave lands on the wave's FIRST unit: the store instructions and their vmcnt bookkeeping stay,
        # the 196 MB of HBM traffic become 2 MB of L2 traffic
        "storesame": {"soff"},
        # (saving cores) the PHASE8 / MX8 encodes of the saved state
        "noenc": {"phase", "mx"},
    }

    def text(self):
        drop = set().union(*(kinds for name, kinds in self.ABLATIONS.items() if name in self.ablate))
        out = []
        seen_first_sync = False  # the requests in front of the first rendezvous stay: the first reads need them
        for x in self.ins:
            if x.op == "sync":
                seen_first_sync = True
            if x.op.partition("_")[0] in drop and (seen_first_sync or x.op not in self.KEEP_FIRST):
                continue
            out.append(x.text)
        return out

    def inc_file(self):
        lines = self.header()
        lines[-1] += ", %[ab] activation workspace (SGPR pair)." if self.save else "."
        lines += ['"' + t + '\\n"' for t in self.text()]
        return "\n".join(lines) + "\n"


DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "variant_streams.sha256")


def variant_files(cls, stem):
    """the file names of the class's VARIANTS (SAVE = 0, both aux sizes).  Their text is not in git; the committed DIGESTS file pins it:
    one ``<sha256>  <file name>`` line per file, which the build holds what it writes to and tests/test_fwd_core_geometry.py holds the
    generator to, so a change of a stream shows in history as a change of its line."""
    return [f"{stem}_a{auxs}{suffix}.inc" for _, suffix in cls.VARIANTS for auxs in (1, 2)]


def read_digests():
    with open(DIGESTS) as f:
        return {name: digest for digest, name in (line.split() for line in f if line.strip())}


def file_digest(path):
    import hashlib

    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def write_variants(cls, stem, out_dir, record=False, **kw):
    """write the VARIANTS' streams into out_dir, each file in one step (another build may be reading it); ``record``: enter their
    digests into DIGESTS (the generators' command line with the default schedule does).  Returns [(path, core)]."""
    out = []
    for vkw, suffix in cls.VARIANTS:
        for auxs in (1, 2):
            c = cls(auxs, save=0, **kw, **vkw)
            path = os.path.join(out_dir, f"{stem}_a{auxs}{suffix}.inc")
            with open(f"{path}.tmp{os.getpid()}", "w") as f:
                f.write(c.inc_file())
            os.replace(f.name, path)
            out.append((path, c))
    if record:
        pins = read_digests() if os.path.exists(DIGESTS) else {}
        pins.update({os.path.basename(path): file_digest(path) for path, _ in out})
        with open(DIGESTS, "w") as f:
            f.writelines(f"{pins[name]}  {name}\n" for name in sorted(pins))
    return out


def main(cls, stem, doc, **defaults):
    """the generators' command line: writes <stem>_a{1,2}[s<save>].inc, the class's VARIANTS and the two clobber lists; `defaults` names the schedule
    parameters the core's constructor takes (R, PF, GROUP, FILL)"""
    import argparse

    ap = argparse.ArgumentParser(description=doc)
    ap.add_argument("--out", default=None, help="output directory (default: csrc/)")
    ap.add_argument("--ablate", default="", help="comma list of timing ablations: " + ",".join(cls.ABLATIONS))
    for name, value in defaults.items():
        ap.add_argument("--" + name, type=int, default=value)
    a = ap.parse_args()
    out_dir = a.out or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(out_dir, exist_ok=True)
    for auxs in (1, 2):
        for save in sorted({0, cls.SAVE}):
            c = cls(auxs, ablate=[x for x in a.ablate.split(",") if x], save=save, **{name: getattr(a, name) for name in defaults})
            path = os.path.join(out_dir, f"{stem}_a{auxs}{f's{save}' if save else ''}.inc")
            with open(path, "w") as f:
                f.write(c.inc_file())
            print(path, c.stats)
    stock = not a.ablate and all(getattr(a, name) == value for name, value in defaults.items())  # the streams the kernels are built from
    for path, c in write_variants(cls, stem, out_dir, record=stock, ablate=[x for x in a.ablate.split(",") if x],
                                  **{name: getattr(a, name) for name in defaults}):
        print(path, c.stats)
    for save in sorted({0, cls.SAVE}):
        with open(os.path.join(out_dir, f"{stem}_clobbers{f'_s{save}' if save else ''}.inc"), "w") as f:
            f.write(cls.clobber_file(save))


# =================================================================================================================================
# Lane-accurate interpreter (CPU validation)
# =================================================================================================================================
LANE = np.arange(64)
ROW_OF = (np.arange(16)[None, :] & 3) + 8 * (np.arange(16)[None, :] >> 2) + 4 * (LANE[:, None] >> 5)  # [lane, g]


def bf16_bits(x):
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint32)


def bf16_to_f32(b):
    return (np.asarray(b, np.uint32) << 16).view(np.float32)


def frag_to_f32(regs4):
    """4 registers [4, 64] of packed bf16 pairs -> [64 lanes, 8] fp32"""
    lo = bf16_to_f32(regs4 & 0xFFFF)
    hi = bf16_to_f32(regs4 >> 16)
    out = np.empty((64, 8), np.float32)
    out[:, 0::2] = lo.T
    out[:, 1::2] = hi.T
    return out


def f32_to_frag(v):
    """[64, 8] fp32 -> 4 registers [4, 64] uint32 (bf16 RNE, element 0 in the low half)"""
    b = bf16_bits(v)
    return (b[:, 0::2] | (b[:, 1::2] << 16)).T.astype(np.uint32)


class LaneModel:
    """Executes the instruction list of one wave on the unified 512-register file.  The ring is shared by the NW waves of the workgroup:
    a DMA request copies the units all waves fetch.  `planes`: the packed stream(s) as the kernel sees them, each [n_units, 64 lanes, 4]
    uint32 (one, or the parity mode's hi and lo).  Checks, the same for every core:
      * ring protocol: a unit is read only after a rendezvous that covers its row; a ring slot is overwritten only once the MFMAs that
        consume its previous content have been issued ahead of a barrier (by this wave; the barrier extends that to all waves), and
        not while a read of it is in flight;
      * loads retire in order (a real queue, for waves that take and waves that skip the ragged last row): vmcnt lets no needed request
        stay in flight, no register is read while a load into it is; lgkmcnt lets no A fragment an MFMA reads stay in flight; VOFF
        addresses row j when row j is requested; SOFF addresses the unit stored;
      * hazards: XDL write -> VALU read, trans -> VALU use, VALU write -> MFMA operand, M0 write -> LDS-DMA; between a narrowing of
        EXEC and its restoring nothing issues but the one-lane LDS write it is for (the trunk's `cell`).
    A core's model adds the ops that are its own in ``own_op``."""

    XDL_NOPS = 18            # XDL write -> VALU read behind an s_nop chain: wait states after a 16-pass MFMA
    IGNORED = {"savem0", "restm0", "dma_pred", "dma_br", "label"}

    def __init__(self, core, *planes):
        c = self.c = core
        self.stream = planes
        self.uses_per_unit = c.stats["mfma"] // c.n_pieces  # MFMAs of a k-step
        self.v = np.zeros((512, 64), np.uint32)
        self.ring_unit = [[-1] * len(planes) for _ in range(c.R)]
        self.ring = np.zeros((c.R, len(planes), 64, 4), np.uint32)
        self.synced_rows = c.PRE_ROWS
        self.uses = np.zeros(c.n_pieces, np.int32)   # MFMAs issued on the unit
        self.consumed_before_barrier = np.zeros(c.n_pieces, bool)
        self.pending = []        # LDS reads in flight, oldest first: (dst, slot, plane, unit)
        self.ar = {}             # register quad -> (unit, plane) it holds
        # loads in flight, oldest first, of a wave that takes / skips the ragged last row: ("row", j, plane) or ("reg", first register, data [n, 64])
        self.vmq = {"full": [], "skip": []}
        for u in range(c.PRE_ROWS * c.NW):  # in the ring when the stream starts (the prologue wrote them, then a barrier)
            for pl, s in enumerate(planes):
                self.ring_unit[u][pl], self.ring[u, pl] = u, s[u]
        self.voff_rows = 0       # rows VOFF has been advanced by: the source of the next request is stream unit NW * voff_rows + wave
        self.soff = 0            # saving cores: byte offset of SOFF relative to the tile's workspace base
        self.stores = {}         # unit -> [4, 64] uint32 (or [2, 64] for a two-dword scale unit)
        self.last_write = {}     # register -> index of the VALU instruction that wrote it (cvt_pk, moves)
        self._xdl, self._n_mfma, self._nops = {}, 0, 0
        self._trans, self._pc, self._m0_at = {}, 0, -9  # v_sin / v_cos results, instruction index, last M0 write
        self._clk, self._exec1 = 0, False               # wait states issued so far (an instruction is one, s_nop n is n + 1), EXEC narrowed

    def f(self, r):
        return self.v[r].view(np.float32)

    def setf(self, r, x):
        self.v[r] = np.asarray(x, np.float32).view(np.uint32)

    def _set_byte(self, d, byte, b):
        self.v[d] = (self.v[d] & np.uint32(~(0xFF << (8 * byte)) & 0xFFFFFFFF)) | (b << np.uint32(8 * byte))

    # XDL write -> VALU read: the generators start a tile's epilogue two MFMAs after its last one (each later MFMA holds the issue port for
    # 8 wait states; 11 are needed after an 8-pass MFMA) or behind an s_nop chain; checked for every VALU source register
    def _mfma_wrote(self, acc):
        for g in range(16):
            self._xdl[acc + g] = self._n_mfma
        self._n_mfma += 1
        self._nops = 0

    def _valu_reads(self, *regs):
        for r in regs:
            k = self._xdl.get(r)
            assert k is None or self._n_mfma - 1 - k >= 2 or self._nops >= self.XDL_NOPS, ("VALU reads an MFMA result too early", r)
            assert self._pc - self._trans.get(r, -9) >= 2, ("trans result used by the next instruction", r)  # trans -> VALU: 1 wait state
            assert not any(e[0] == "reg" and e[1] <= r < e[1] + len(e[2]) for e in self.vmq["full"]), ("register read while its load is in flight", r)

    def _vm_issue(self, entry, ragged=False):
        self.vmq["full"].append(entry)
        if not ragged:
            self.vmq["skip"].append(entry)

    def _vm_wait(self, keep):
        for q in self.vmq.values():  # loads return in order: all but the `keep` newest have landed
            for e in q[:max(len(q) - keep, 0)]:
                if e[0] == "reg":
                    self.v[e[1]:e[1] + len(e[2])] = e[2]
            del q[:max(len(q) - keep, 0)]

    def _lgkm_wait(self, keep):
        while len(self.pending) > keep:
            dst, slot, plane, unit = self.pending.pop(0)
            if dst is not None:  # (None: an LDS write)
                assert self.ring_unit[slot][plane] == unit, "ring slot overwritten while a read of it was in flight"
                self.v[dst:dst + 4] = self.ring[slot, plane].T
                self.ar[dst] = (unit, plane)

    def own_op(self, op, a, ins):
        assert op in self.IGNORED, "instruction not modelled: " + ins.text

    def run(self):
        c, NW = self.c, self.c.NW
        for n, ins in enumerate(c.ins):
            op, a = ins.op, ins.a
            self._pc = n
            self._clk += 1
            assert not self._exec1 or op in ("cell", "execall"), ("instruction issued with EXEC narrowed to one lane", ins.text)
            if op == "mfma":
                acc, areg, breg, c0 = a
                assert not any(d == areg for d, *_ in self.pending), "MFMA reads an A fragment still in flight"
                for r in range(breg, breg + 4):
                    assert n - self.last_write.get(r, -10) >= 3, ("VALU write -> MFMA operand hazard", ins.text)
                unit, _ = self.ar[areg]
                assert self.uses[unit] < self.uses_per_unit
                self.uses[unit] += 1
                A = frag_to_f32(self.v[areg:areg + 4]).astype(np.float64)  # [lane, j] : row = lane & 31, k = 8 h + j
                B = frag_to_f32(self.v[breg:breg + 4]).astype(np.float64)
                Am, Bm = np.zeros((32, 16)), np.zeros((16, 32))
                for h in range(2):
                    Am[:, 8 * h:8 * h + 8] = A[32 * h:32 * h + 32]
                    Bm[8 * h:8 * h + 8, :] = B[32 * h:32 * h + 32].T
                d = (Am @ Bm)[ROW_OF, (LANE & 31)[:, None]]  # [lane, g]
                for g in range(16):
                    prev = np.zeros(64, np.float32) if c0 else self.f(acc + g).copy()
                    self.setf(acc + g, (prev.astype(np.float64) + d[:, g]).astype(np.float32))
                self._mfma_wrote(acc)
            elif op == "nop":
                self._nops += a[0] + 1
                self._clk += a[0]
            elif op == "dsread":
                dst, slot, plane = a
                unit = self.ring_unit[slot][plane]
                assert unit >= 0 and unit // NW < self.synced_rows, ("unit read before the rendezvous that covers its row", unit, self.synced_rows)
                self.pending.append((dst, slot, plane, unit))
            elif op == "waitl":
                self._lgkm_wait(a[0])
            elif op == "sync":
                vm, need = a
                self._vm_wait(vm)
                for cls, q in self.vmq.items():
                    missing = [e for e in q if e[0] == "row" and e[1] < need]
                    assert not missing, ("vmcnt lets a needed request stay in flight", cls, vm, need, missing[:4])
                self.synced_rows = max(self.synced_rows, need)
            elif op == "barrier":
                self.consumed_before_barrier = self.uses == self.uses_per_unit
            elif op == "m0":
                self._m0_at = n
            elif op == "dma":
                j, plane, partial = a
                assert n - self._m0_at >= 2, "M0 write -> LDS-DMA needs one wait state"
                assert c.PRE_ROWS + self.voff_rows == c.src_row(j), ("VOFF does not address row j of the stream", j, self.voff_rows)
                self._vm_issue(("row", j, plane), ragged=partial is not None)
                for w in range(NW if partial is None else partial):
                    u = NW * j + w
                    slot = u % c.R
                    old = self.ring_unit[slot][plane]
                    assert old < 0 or self.consumed_before_barrier[old], ("DMA overwrites a unit not yet consumed by every wave", old, u)
                    self.ring_unit[slot][plane] = u
                    self.ring[slot, plane] = self.stream[plane][NW * c.src_row(j) + w]
            elif op == "voff":
                self.voff_rows += a[0] if a else 1
            elif op == "fract":
                self._valu_reads(a[0])
                x = self.f(a[0]).astype(np.float64)
                self.setf(a[0], x - np.floor(x))
            elif op == "sin":
                self._valu_reads(a[0])
                self._trans[a[0]] = n
                self.setf(a[0], np.sin(2 * np.pi * self.f(a[0]).astype(np.float64)))
            elif op == "pk":
                d, s0, s1 = a
                self._valu_reads(s0, s1)
                self.v[d] = (bf16_bits(self.f(s0)) | (bf16_bits(self.f(s1)) << 16)).astype(np.uint32)
                self.last_write[d] = n
            elif op in ("accw", "accr", "mov"):
                self._valu_reads(a[1])
                self.v[a[0]] = self.v[a[1]]
                self.last_write[a[0]] = n
            elif op == "shl":
                self.v[a[0]] = (self.v[a[1]] << np.uint32(16)).astype(np.uint32)
            elif op == "and":
                self.v[a[0]] = self.v[a[1]] & np.uint32(0xFFFF0000)
            elif op == "sub":
                d, x, y = a
                self._valu_reads(x, y)
                self.setf(d, self.f(x) - self.f(y))
            elif op == "pknorm":  # v_cvt_pknorm_u16_f32: round(clamp(x, 0, 1) * 65535), RNE
                d, s0, s1 = a
                self._valu_reads(s0, s1)
                u = [np.rint(np.clip(self.f(r).astype(np.float64), 0, 1) * 65535).astype(np.uint32) for r in (s0, s1)]
                self.v[d] = u[0] | (u[1] << np.uint32(16))
            elif op == "phase":  # SDWA add, dst_sel:BYTE_k UNUSED_PRESERVE: the low byte of the fp32 sum goes into byte k
                d, byte, src = a
                self._valu_reads(src)
                self._set_byte(d, byte, (self.f(src) + self.f(c.KMAGIC)).astype(np.float32).view(np.uint32) & np.uint32(0xFF))
            elif op == "soff":
                self.soff += a[0]
            elif op == "store":
                reg, unit, ndw = a
                assert self.soff == unit * 1024 and unit not in self.stores, ("SOFF does not address the unit stored", self.soff, unit)
                self.stores[unit] = self.v[reg:reg + ndw].copy()
            elif op == "mx_max":
                m, x, y, z = a
                self._valu_reads(x, y)
                r = np.maximum(np.abs(self.f(x)), np.abs(self.f(y)))
                self.setf(m, r if z is None else np.maximum(r, self.f(z)))
            elif op == "mx_e1":
                self.setf(a[0], self.f(a[0]).astype(np.float64) * 0.0078125 + self.f(a[0]).astype(np.float64))
            elif op == "mx_e2":
                self.v[a[0]] = self.v[a[1]] >> np.uint32(23)
            elif op == "mx_e3a":  # clamp to [6, 254]
                self.v[a[0]] = np.maximum(self.v[a[0]], np.uint32(6))
            elif op == "mx_e3":
                self.v[a[0]] = np.minimum(self.v[a[0]], np.uint32(254))
            elif op == "mx_e4":
                self.v[a[0]] = (np.uint32(260) - self.v[a[1]]).astype(np.uint32)
            elif op == "mx_e5":
                self.v[a[0]] = (self.v[a[0]] << np.uint32(23)).astype(np.uint32)
            elif op == "mx_e6":
                d, e, sh, first = a
                self.v[d] = self.v[e].copy() if first else ((self.v[e] << np.uint32(sh)) | self.v[d]).astype(np.uint32)
            elif op == "mx_q1":
                t, src, inv = a
                self._valu_reads(src)
                self.setf(t, self.f(src).astype(np.float64) * self.f(inv).astype(np.float64) + self.f(c.K128).astype(np.float64))
            elif op == "mx_q2":  # v_cvt_pk_u8_f32: round to nearest even, saturate to [0, 255]
                d, t, byte = a
                self._set_byte(d, byte, np.clip(np.rint(self.f(t).astype(np.float64)), 0, 255).astype(np.uint32))
            else:
                self.own_op(op, a, ins)
        assert (self.uses == self.uses_per_unit).all()
