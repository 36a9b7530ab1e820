#!/usr/bin/env python3
"""Generator of k_blockw: the bottleneck residual blocks of a C = 256 / C_b = 128 trunk, one wave per SIMD.

    python blockw_gen.py OUT.s            (kernels k_blockw_L1, _L2, _L3 and their _diag twins)

Arithmetic spec: BottleneckResidualConvBlock, /root/reference/python/model.py:372-425 (x + conv1x1(... conv3x3(
... conv1x1(x)))), every conv = conv(mish(bn(.))), model.py:276-292), net shapes model_config.py:98-105.  The HIP
kernel k_block<256,128,btl> (kernels.hip) computes the same thing with eight waves and 256 registers each; DESIGN.md
section 4 (round 4) explains why this form exists: with two waves per SIMD the BN + mish epilogues (VALU) never ran
under MFMA work, 44 % of a block's cycles.

Shape.  One 256-thread workgroup (four waves, one per SIMD, 512 registers each: 256 VGPR + 256 AGPR) owns a position.
Wave w owns the board-row tiles t = w, w + 4, w + 8 (32 padded rows each) and ALL 128 output channels of a layer, as
two accumulator sets in AGPRs: set A = channels 0..63, set B = 64..127 (96 registers each), on
v_mfma_f32_32x32x16_f16: a single wave can issue one instruction per 4 cycles (8 for a transcendental, 8 for an MFMA),
measured with tools/gpu_issue_probe.py, so a 32-cycle MFMA leaves 24 issue cycles for everything else — fragment
reads, waits, the weight ring's DMA, and the epilogues — where the 16-cycle 16x16x32 leaves 8.
The act buffer in LDS (one slot of 128 channels per padded board point, conv_core.h Geo<1,128,3>) is updated IN PLACE:
    3x3 layer l:   phase 1 (A, cin lo)   phase 2 (B, cin lo)   phase 3 (A, cin hi)   phase 4 (B, cin hi)
    under phase 1: epilogue of set B of layer l-1 -> channels hi      (hi is next read by phase 3)
    under phase 4: epilogue of set A of layer l   -> channels lo      (lo was last read by phase 2)
The folded BN of a layer rides in the conv before it: its scale (times log2 e) is multiplied into that conv's fp16
weights on the host, its shift (times log2 e) is the accumulators' initial value (the first MFMA of a chain takes it
as C), so an epilogue is mish alone: exp2, rcp and five plain operations per value.
Weights stream HBM/L2 -> LDS ring by LDS-DMA in 4 KiB granules (64 output channels x 32 k), twelve slots, one barrier
per group of three granules.  A block's input is always x in HBM (fetched in the 16-byte piece layout, activated,
written to LDS), its output x' goes to HBM: the block loop carries no register state, and position / block form one
flat runtime loop.
"""
import sys

from emitter import (A, S, V, Bundle, Emitter, Ins, accread, cvt_pk, ds_read128, ds_write128, gload128, gstore128, mfma32, misc,
                     permswap32, rtxt, salu, trans, valu)

# ---- geometry (conv_core.h Geo<1, 128, 3>) ----------------------------------------------------
SLOTB = 272                     # bytes per act slot: 128 channels fp16 + 16 B pad
SROW = 20                       # padded row stride
PADTOP = 21
PSLOTS = PADTOP + 379 + PADTOP
ACT_BYTES = (PSLOTS * SLOTB + 15) // 16 * 16            # 114,512
GRAN = 4096                     # weight granule: 64 couts x 32 k fp16 = [k16 half j][cout tile c][h][n][8]
NSLOT = 12
RING0 = ACT_BYTES
LDS_BYTES = RING0 + NSLOT * GRAN                        # 163,664
assert LDS_BYTES <= 163840
NLOC = 361
CBLK_BYTES = NLOC * 16          # bytes of one 8-channel block of one position in x
POS_BYTES = 32 * CBLK_BYTES     # C = 256

# ---- register map -----------------------------------------------------------------------------
# AGPR
ACC = {"A": 0, "B": 96}         # acc (c, b) of set s: 16 registers at ACC[s] + (c * 3 + b) * 16
FA = 192                        # weight fragments: fa[buf][j * 2 + c] = a[FA + (buf * 4 + j * 2 + c) * 4 ...]
INIT = 224                      # [2][16] the accumulators' initial value (BN shift) of the set that starts next


def acc(s, c, b):
    return A(ACC[s] + (c * 3 + b) * 16, 16)


def fa(buf, jc):
    return A(FA + (buf * 4 + jc) * 4, 4)


# VGPR
V_TID = 0
V_DMAOFF = 1        # [3] this lane's 16 bytes of granule k of a group: tid * 16 + 4096 k
V_ARING = 4         # RING0 + lane * 16: this lane's piece of weight fragment 0 of ring slot 0
V_BROW = 5          # [3] LDS address of this lane's activation fragment of tile b at tap (0, 0), k16 step 0
V_WROW = 8          # [3] LDS address of this lane's row of tile b, chunk h
V_XOFF = 11         # [3] byte offset of this lane's piece of tile b inside channel block h of the position
V_HOFF = 14         # h * 16: byte offset of this lane's four channels inside an 8-channel group (fp32 parameters)
V_POFF = 15         # h * 32: byte offset of this lane's eight channels inside a 16-channel group (fp32 parameters)
V_C1 = 16           # -2 ln 2
V_C2 = 17           # ln 2
V_ZERO = 20         # [4] zeros
R0 = 24             # [4][3] activation fragments of a k16 step, 4 registers each: buffer ring of four steps


def rfrag(buf, b):
    return V(R0 + (buf * 3 + b) * 4, 4)


P0 = 72             # [32] bn0 parameters of the activation: two banks of 16
XBUF = (104, 152)   # [2][48] x pieces of a quarter
T0 = 200            # [8] temporaries
W0 = 208            # [8]
TMP = 216           # [8]
O0 = 224            # [4] packed results
# (228..255 free)

# SGPR
S_KARG = 0          # [2]
S_WG = 2
S_X = 4             # [2] x
S_WS = 6            # [2] weight stream of the launch's blocks
S_PRM = 8           # [2] parameter table
S_NPOS = 10
S_NBLK = 11
S_NWG = 12
S_STAMP = 14        # [2] diag stamps
S_POS = 16
S_BLK = 17
S_XP = 18           # [2] x of this position
S_XQ = 20           # [2] scratch: a channel block of this position (stores)
S_DMA = 22          # [2] next granule group to fetch
S_PB = 24           # [2] parameters of this block
S_PQ = 26           # [2] scratch: a parameter row
S_RINGW = 28        # RING0 + wave * 1024: LDS address of the wave's piece of slot 0 (M0 = S_RINGW + slot * 4096)
S_OK = 30           # [3][2] lanes whose row of tile b is on the board
S_TMP = 36          # [4]
S_WAVE = 40
S_XL = 42           # [2] scratch: a channel block of this position (loads)
S_T0 = 44           # [2 * 24] diag stamps of one block

LN2 = 0.6931471805599453


def f32hex(x):
    import struct
    return "0x%08x" % struct.unpack("<I", struct.pack("<f", x))[0]


class BlockGen:
    def __init__(self, L, diag=False, dump_at=None):
        self.L = L
        self.diag = diag
        self.dump_at = dump_at            # debugging: at stamp point k dump LDS and registers, then end
        self.stop = None                  # debugging: end after a piece of the entry (tools/gpu_blockw_bisect.py)
        self.opts = {}                    # timing probes (tools/gpu_blockw_phaseprobe.py; wrong results)
        self.e = Emitter()
        self.ngran = 32 + 72 * L          # granules of one block: reduce 16, layers 72 each, expand 16
        self.nstamp = 0
        # parameter table of one block (floats, plan.cpp pack_blockw_runs): bn0 scale[256] shift[256], both times log2(e);
        # then per conv j = 0..L (reduce, inner layers): the NEXT BN's shift[128] times log2(e) (its scale is in the weights)
        self.prm_floats = 512 + 128 * (L + 1)

    # ---- ring ---------------------------------------------------------------------------------
    def dma_issue(self, g, k=0):
        """LDS-DMA of granule g (the k-th of the group S_DMA points at) into slot g % NSLOT"""
        slot = g % NSLOT
        return Bundle([
            salu("s_add_u32", "m0", S(S_RINGW), slot * GRAN),
            misc("s_nop 0"),
            Ins(f"global_load_lds_dwordx4 {rtxt(V(V_DMAOFF + k))}, {rtxt(S(S_DMA, 2))}", "dma", [], [V(V_DMAOFF + k), S(S_DMA, 2)], 16, ("g", g)),
        ])

    def dma_group(self, g0, n):
        """granules g0 .. g0 + n - 1 (n <= 3), then the stream pointer moves on"""
        it = [self.dma_issue(g0 + k, k) for k in range(n)]
        it.append(salu("s_add_u32", S(S_DMA), S(S_DMA), n * GRAN))
        it.append(salu("s_addc_u32", S(S_DMA + 1), S(S_DMA + 1), 0))
        return it

    def ring_sync(self, need):
        """main-stream items: the granules in `need` have landed for every wave, older slots are free: refill them."""
        items = []
        tags = {("g", g) for g in need}
        g0 = min(need)

        def wait_and_barrier(e, tags=tags):
            e.wait_vm_tags(tags)
            if not self.opts.get("nobarrier"):
                e.raw("\ts_barrier")
        items.append(("call", wait_and_barrier))
        lim = min(g0 + NSLOT, self.ngran)
        while self.next_dma < lim:
            n = min(3, lim - self.next_dma)
            if not self.opts.get("nodma"):
                items += self.dma_group(self.next_dma, n)
            self.next_dma += n
        return items

    # ---- K loop --------------------------------------------------------------------------------
    @staticmethod
    def b_off(ky, kx, s16):
        """immediate offset of the activation fragment at tap (ky, kx), k16 step s16 of the 128 resident channels"""
        return (ky * SROW + kx) * SLOTB + s16 * 32

    def kloop(self, g_base, grans, sync_every=3, marks=None):
        """main-stream items of a K loop over a list of granules.  A granule = (set, first, [(ky, kx, s16), (ky, kx, s16)]):
        64 output channels of `set` times 32 input channels as two k16 steps whose activation fragments sit at the given
        tap and channel step; `first`: the accumulators start from the BN shift (INIT registers) or, None, from zero.
        Weights: ring granules g_base ..; activation fragments are fetched two k16 steps ahead (ring of four buffers),
        weight fragments one granule ahead.  marks: {granule index: [items]} inserted before that granule."""
        items = []
        marks = marks or {}
        n = len(grans)
        steps = [(gi, j) for gi in range(n) for j in range(2)]

        def afetch(gi):
            return [ds_read128(fa(gi % 2, jc), V(V_ARING), ((g_base + gi) % NSLOT) * GRAN + jc * 1024) for jc in range(4)]

        def bfetch(si):
            gi, j = steps[si]
            ky, kx, s16 = grans[gi][2][j]
            return [ds_read128(rfrag(si % 4, b), V(V_BROW + b), self.b_off(ky, kx, s16)) for b in range(3)]
        items += self.ring_sync(range(g_base, g_base + min(sync_every, n)))
        items += afetch(0)
        items += bfetch(0)
        if len(steps) > 1:
            items += bfetch(1)
        for si, (gi, j) in enumerate(steps):
            sset, first, _ = grans[gi]
            if j == 0 and gi in marks:
                items += marks[gi]
            need = [rfrag(si % 4, b) for b in range(3)] + ([fa(gi % 2, jc) for jc in range(4)] if j == 0 else [])
            items.append(("call", lambda e, need=need: e.prewait(need)))
            pre_a = afetch(gi + 1) if (j == 0 and gi + 1 < n) else []
            pre_b = bfetch(si + 2) if si + 2 < len(steps) else []
            for b in range(3):
                for c in range(2):
                    if first is True and j == 0:
                        cin = A(INIT + c * 16, 16)
                    elif first is None and j == 0:
                        cin = 0
                    else:
                        cin = acc(sset, c, b)
                    items.append(mfma32(acc(sset, c, b), fa(gi % 2, j * 2 + c), rfrag(si % 4, b), cin))
                if b == 0:
                    # the next granule's weights: a ring sync where they begin a new group, then the fragment reads
                    if j == 0 and gi + 1 < n and (gi + 1) % sync_every == 0:
                        items += self.ring_sync(range(g_base + gi + 1, g_base + min(gi + 1 + sync_every, n)))
                    items += pre_a[:2]
                elif b == 1:
                    items += pre_a[2:]
                    items += pre_b[:1]
                else:
                    items += pre_b[1:]
        return items

    def phase_grans(self, sset, half, first):
        """the 18 granules of a 3x3 phase: set `sset` over input channels half (0 = lo, 1 = hi), order (ky, q, kx)"""
        out = []
        for ky in range(3):
            for q in range(2):
                for kx in range(3):
                    fl = first if (ky, q, kx) == (0, 0, 0) else False
                    out.append((sset, fl, [(ky, kx, 4 * half + 2 * q + j) for j in range(2)]))
        return out

    # ---- fillers ---------------------------------------------------------------------------------
    def prm_row(self, float_off):
        """items that point S_PQ at a row of this block's parameter table"""
        return [salu("s_add_u32", S(S_PQ), S(S_PB), float_off * 4), salu("s_addc_u32", S(S_PQ + 1), S(S_PB + 1), 0)]

    def init_loads(self, sset, row):
        """items: the BN shift (times log2 e) of this lane's channels of set `sset` -> the INIT registers (the first MFMA of
        each accumulator chain of the set takes them as C).  row: float offset of the conv's shift row in the block's table."""
        it = self.prm_row(row + (0 if sset == "A" else 64))
        for c in range(2):
            for g in range(4):
                it.append(gload128(A(INIT + c * 16 + g * 4, 4), V(V_HOFF), S(S_PQ, 2), (32 * c + 8 * g) * 4, "prm"))
        return it

    def mish8(self, t, w):
        """stage by stage over eight values: t[i] = log2(e) * y in, u in w[i] out (mish(y) = t * u, applied by the caller)"""
        it = []
        for i in range(8):
            it.append(trans("v_exp_f32", V(w + i), V(t + i)))
        for i in range(8):
            it.append(valu("v_add_f32", V(TMP + i), 2.0, V(w + i)))
        for i in range(8):
            it.append(valu("v_fma_f32", V(w + i), V(w + i), V(TMP + i), 2.0))
        for i in range(8):
            it.append(trans("v_rcp_f32", V(w + i), V(w + i)))
        for i in range(8):
            it.append(valu("v_fma_f32", V(w + i), V(w + i), V(V_C1), V(V_C2)))
        return it

    def pack8(self, t, w, o):
        """o[0..3] = fp16 of t[i] * w[i]: (o0, o1) = values 0..3, (o2, o3) = values 4..7"""
        it = []
        for i in range(8):
            it.append(valu("v_mul_f32", V(t + i), V(t + i), V(w + i)))
        for k in range(4):
            it.append(cvt_pk(V(o + k), V(t + 2 * k), V(t + 2 * k + 1)))
        return it

    def masked(self, b, ins):
        return Bundle([misc(f"s_mov_b64 exec, {rtxt(S(S_OK + 2 * b, 2))}"), ins, misc("s_mov_b64 exec, -1")])

    def epi_layer(self, sset, dst_half):
        """filler items: mish of accumulator set `sset` (its BN is already inside: scale in the weights, shift in the initial
        value) -> fp16 -> act buffer channels half dst_half.  Lane (n, h) holds, per (cout tile c, tile b), four quads g of
        channels 32 c + 8 g + 4 h ..+3 of its row; quads g, g + 1 pair up with the partner lane (v_permlane32_swap) into the
        16-byte pieces of chunks 4 c + g (h = 0 lanes) and 4 c + g + 1 (h = 1 lanes)."""
        it = []
        for b in range(3):
            for c in range(2):
                for gp in range(2):          # quads 2 gp, 2 gp + 1
                    base = ACC[sset] + (c * 3 + b) * 16 + gp * 8
                    for i in range(8):
                        it.append(accread(V(T0 + i), A(base + i)))
                    it += self.mish8(T0, W0)
                    it += self.pack8(T0, W0, O0)
                    it.append(permswap32(V(O0), V(O0 + 2)))
                    it.append(permswap32(V(O0 + 1), V(O0 + 3)))
                    it.append(self.masked(b, ds_write128(V(V_WROW + b), V(O0, 4), (dst_half * 8 + 4 * c + 2 * gp) * 16)))
        return it

    def xq_point(self, cblk, sreg=S_XQ):
        """items: sreg = channel block cblk of this position"""
        return [salu("s_add_u32", S(sreg), S(S_XP), cblk * CBLK_BYTES), salu("s_addc_u32", S(sreg + 1), S(S_XP + 1), 0)]

    def x_loads(self, quarter, buf, tag):
        """items: this lane's twelve 16-byte pieces of x quarter `quarter` -> X buffer `buf`: piece (j, b) = chunk
        8 quarter + 2 j + h of its row of tile b"""
        it = []
        for j in range(4):
            it += self.xq_point(quarter * 8 + 2 * j, S_XL)
            for b in range(3):
                it.append(gload128(V(XBUF[buf] + (j * 3 + b) * 4, 4), V(V_XOFF + b), S(S_XL, 2), 0, tag))
        return it

    def act_write(self, buf, dst_half):
        """items: the activated pieces in X buffer `buf` -> act buffer half (on-board rows only)"""
        return [self.masked(b, ds_write128(V(V_WROW + b), V(XBUF[buf] + (j * 3 + b) * 4, 4), (dst_half * 8 + 2 * j) * 16))
                for j in range(4) for b in range(3)]

    def act_loads(self, quarter, j):
        """items: bn0 parameters of this lane's eight channels of (quarter, chunk pair j) -> act bank (quarter * 4 + j) % 2"""
        bank = P0 + 16 * ((quarter * 4 + j) % 2)
        it = self.prm_row(quarter * 64 + j * 16)
        for k in range(2):      # scale (k = 0: first four channels), shift
            it.append(gload128(V(bank + 4 * k, 4), V(V_POFF), S(S_PQ, 2), 16 * k, "prm"))
            it.append(gload128(V(bank + 8 + 4 * k, 4), V(V_POFF), S(S_PQ, 2), 1024 + 16 * k, "prm"))
        return it

    def act_quarter(self, quarter, buf, dst_half, write=True, then=None):
        """filler items: the fetched pieces of x quarter `quarter` (X buffer `buf`) -> mish(bn0(.)), in place;
        write: -> act buffer half as each piece is done (otherwise act_write follows later).  The parameters of
        (quarter, 0) were requested by the caller (act_loads); each chunk pair requests the next one's, the last
        one those of (then, 0)."""
        X0 = XBUF[buf]
        it = []
        for j in range(4):
            bank = P0 + 16 * ((quarter * 4 + j) % 2)
            if j + 1 < 4:
                it += self.act_loads(quarter, j + 1)
            elif then is not None:
                it += self.act_loads(then, 0)
            for b in range(3):
                x = X0 + (j * 3 + b) * 4
                for i in range(8):
                    hi = i % 2
                    it.append(valu("v_fma_mix_f32", V(T0 + i), V(x + i // 2), V(bank + i), V(bank + 8 + i),
                                   mods=f" op_sel:[{hi},0,0] op_sel_hi:[1,0,0]"))
                it += self.mish8(T0, W0)
                it += self.pack8(T0, W0, x)
                if write:
                    it.append(self.masked(b, ds_write128(V(V_WROW + b), V(x, 4), (dst_half * 8 + 2 * j) * 16)))
        return it

    def r_loads(self, quarter, buf, tag):
        """items: the residual pieces of output quarter `quarter` -> X buffer `buf`: piece (c, gp, b) = chunk
        8 quarter + 4 c + 2 gp + h of this lane's row of tile b"""
        it = []
        for c in range(2):
            for gp in range(2):
                it += self.xq_point(quarter * 8 + 4 * c + 2 * gp, S_XL)
                for b in range(3):
                    it.append(gload128(V(XBUF[buf] + ((c * 2 + gp) * 3 + b) * 4, 4), V(V_XOFF + b), S(S_XL, 2), 0, tag))
        return it

    def epi_expand(self, quarter, sset, buf):
        """filler items: x' = acc + x (fp16) for output channels quarter * 64 .. -> HBM (the X buffer holds the residual
        pieces, r_loads); conv16.h epilogue_store16's arithmetic"""
        X0 = XBUF[buf]
        it = []
        for c in range(2):
            for gp in range(2):
                it += self.xq_point(quarter * 8 + 4 * c + 2 * gp)
                for b in range(3):
                    x = X0 + ((c * 2 + gp) * 3 + b) * 4
                    base = ACC[sset] + (c * 3 + b) * 16 + gp * 8
                    for i in range(8):
                        it.append(accread(V(T0 + i), A(base + i)))
                    # piece halves -> (my four channels of quad 2 gp, of quad 2 gp + 1)
                    it.append(permswap32(V(x), V(x + 2)))
                    it.append(permswap32(V(x + 1), V(x + 3)))
                    for i in (0, 2, 4, 6, 1, 3, 5, 7):
                        op = "v_fma_mixlo_f16" if i % 2 == 0 else "v_fma_mixhi_f16"
                        ins = valu(op, V(O0 + i // 2), V(T0 + i), 1.0, V(x + i // 2), mods=f" op_sel:[0,0,{i % 2}] op_sel_hi:[0,0,1]",
                                   note="dstsel", cost=8)
                        if i % 2:
                            ins.src |= {("v", O0 + i // 2)}
                        it.append(ins)
                    it.append(permswap32(V(O0), V(O0 + 2)))
                    it.append(permswap32(V(O0 + 1), V(O0 + 3)))
                    it.append(self.masked(b, gstore128(V(V_XOFF + b), V(O0, 4), S(S_XQ, 2), 0, "xst")))
        return it

    # ---- diagnostics ------------------------------------------------------------------------------
    def stamp(self):
        """main-stream item: s_memtime into the block's stamp registers (diag build only)"""
        if self.dump_at is not None:
            k = self.nstamp
            self.nstamp += 1
            return [("call", self.dump_and_end)] if k == self.dump_at else []
        if not self.diag:
            return []
        k = self.nstamp
        self.nstamp += 1
        assert k < 24

        def f(e, k=k):
            e.wait_lgkm_all()
            e.raw(f"\ts_memtime {rtxt(S(S_T0 + 2 * k, 2))}")
            if k == 0:
                e.raw(f"\ts_memrealtime {rtxt(S(S_T0 + 42, 2))}")      # slot 21: 100 MHz clock at the block's first stamp
            e.raw("\ts_waitcnt lgkmcnt(0)")
        return [("call", f)]

    def dump_and_end(self, e, parts=("vgpr", "sgpr", "agpr", "lds")):
        """debugging (tools/gpu_blockw_simcmp.py): the workgroup's LDS and every wave's registers -> the stamps buffer,
        [LDS 163,840 B][wave w: v0..v255, a0..a255 as 512 x 64 dwords], then the program ends.  v248..v255 are scratch."""
        e.wait_vm_all()
        e.wait_lgkm_all()
        e.raw("\ts_barrier")
        # registers first (v248.. are clobbered afterwards): wave w at 163840 + w * 131072, register r at r * 256 + lane * 4
        # (the dump goes behind position 0 of the x buffer, which the harness allocates large enough: the stamps pointer
        # is not trusted here — it is one of the things being debugged; the SGPRs go out too, as "register" v248..)
        e.raw(f"\ts_add_u32 s{S_STAMP}, s{S_X}, {POS_BYTES}")
        e.raw(f"\ts_addc_u32 s{S_STAMP + 1}, s{S_X + 1}, 0")
        e.raw(f"\ts_mul_i32 s{S_TMP}, s{S_WAVE}, 131072")
        e.raw(f"\ts_add_u32 s{S_TMP}, s{S_TMP}, 163840")
        e.raw(f"\ts_add_u32 s{S_TMP + 2}, s{S_STAMP}, s{S_TMP}")
        e.raw(f"\ts_addc_u32 s{S_TMP + 3}, s{S_STAMP + 1}, 0")
        e.raw("\tv_mov_b32 v250, v0")
        e.raw("\tv_and_b32 v251, 63, v0")
        e.raw("\tv_lshlrev_b32 v251, 2, v251")            # lane * 4
        for r in range(248):
            if "vgpr" in parts:
                e.raw(f"\tglobal_store_dword v251, v{r}, s[{S_TMP + 2}:{S_TMP + 3}] offset:{(r * 256) % 4096}")
            if (r * 256) % 4096 == 3840:
                e.raw(f"\ts_add_u32 s{S_TMP + 2}, s{S_TMP + 2}, 4096")
                e.raw(f"\ts_addc_u32 s{S_TMP + 3}, s{S_TMP + 3}, 0")
        # SGPRs 0..63 in the slot of "register" 248, 64..95 in that of 249 (lane i = SGPR i)
        for base, reg in (((0, 248), (64, 249)) if "sgpr" in parts else ()):
            e.raw("\tv_mov_b32 v252, 0")
            e.raw("\ts_nop 3")
            for i in range(64 if base == 0 else 32):
                if base + i in (S_STAMP, S_STAMP + 1):
                    continue
                e.raw(f"\tv_writelane_b32 v252, s{base + i}, {i}")
            e.raw("\ts_nop 1")
            e.raw(f"\tglobal_store_dword v251, v252, s[{S_TMP + 2}:{S_TMP + 3}] offset:{(reg * 256) % 4096}")
            e.raw("\ts_nop 1")
        # (248 = 15.5 pages: the pointer stands at register 240's page; registers 250..255 are skipped)
        e.raw(f"\ts_add_u32 s{S_TMP + 2}, s{S_TMP + 2}, 4096")
        e.raw(f"\ts_addc_u32 s{S_TMP + 3}, s{S_TMP + 3}, 0")
        for r in range(256):
            if "agpr" in parts:
                e.raw(f"\tv_accvgpr_read_b32 v252, a{r}")
                e.raw("\ts_nop 1")
                e.raw(f"\tglobal_store_dword v251, v252, s[{S_TMP + 2}:{S_TMP + 3}] offset:{(r * 256) % 4096}")
                e.raw("\ts_nop 1")
            if (r * 256) % 4096 == 3840:
                e.raw(f"\ts_add_u32 s{S_TMP + 2}, s{S_TMP + 2}, 4096")
                e.raw(f"\ts_addc_u32 s{S_TMP + 3}, s{S_TMP + 3}, 0")
        # LDS: thread t copies bytes [t * 16 + 4096 * i, +16), i = 0 .. 39
        e.raw("\tv_lshlrev_b32 v253, 4, v250")
        e.raw(f"\ts_mov_b64 s[{S_TMP + 2}:{S_TMP + 3}], s[{S_STAMP}:{S_STAMP + 1}]")
        for i in range(40 if "lds" in parts else 0):
            e.raw("\tds_read_b128 v[244:247], v253")
            e.raw("\ts_waitcnt lgkmcnt(0)")
            e.raw(f"\tglobal_store_dwordx4 v253, v[244:247], s[{S_TMP + 2}:{S_TMP + 3}]")
            e.raw("\ts_waitcnt vmcnt(0)")
            e.raw("\tv_add_u32 v253, 4096, v253")
        e.raw("\ts_waitcnt vmcnt(0)")
        e.raw("\ts_endpgm")

    # ---- the block ------------------------------------------------------------------------------
    def block_body(self):
        L = self.L
        main = []
        self.next_dma = NSLOT          # granules 0..11 were issued at the block's entry
        self.nstamp = 0
        g = 0
        bar = ("call", lambda e: e.raw("\ts_barrier"))
        wlw = Ins("", "wait_lds_writes")
        main += self.stamp()
        # -- the block's input: x quarters 0, 1 (requested at the block's entry, with the first parameters) -> act buffer
        # lo, hi; quarters 2, 3 are requested as the buffers come free ---------------------------------------------
        main += self.act_quarter(0, 0, 0, then=1)
        main += self.x_loads(2, 0, "x2")
        main += self.act_quarter(1, 1, 1, then=2)
        main += self.x_loads(3, 1, "x3")
        main += self.init_loads("A", 512)             # the reduce conv's accumulators start from bn1's shift
        main.append(wlw)
        main += self.stamp()
        # -- reduce, first half: x quarters 0, 1 (act lo, hi: k16 steps 0..7), set A then set B; quarter 2's activation
        # rides along, its LDS stores wait for the barrier behind the K loop -------------------------------------
        def red(sset, first):
            return [(sset, first if s == 0 else False, [(1, 1, 2 * s + j) for j in range(2)]) for s in range(4)]
        main.append(("start", "act2", self.act_quarter(2, 0, 0, write=False, then=3)))
        main += self.kloop(g, red("A", True) + red("B", True), 4, marks={1: self.init_loads("B", 512)})
        g += 8
        main.append(("flush", "act2"))
        main += self.stamp()
        main.append(bar)                               # lo and hi are free: every wave has left the K loop
        main += self.act_write(0, 0)
        main += self.act_quarter(3, 1, 1)
        main.append(wlw)
        main += self.stamp()
        main += self.kloop(g, red("A", False) + red("B", False), 4, marks={5: self.init_loads("A", 512 + 128)})
        g += 8
        main += self.stamp()
        # -- reduce epilogue: set A exposed (lo is read by the first phase), set B under phase 1 -----------------
        main.append(bar)                               # every wave is done reading the act buffer
        main += self.epi_layer("A", 0)
        main.append(wlw)
        main += self.stamp()
        pendingB = self.epi_layer("B", 1)
        for l in range(1, L + 1):
            row = 512 + 128 * l                        # shift row of this layer's conv (= the next BN's)
            nxt = 512 + 128 * (l + 1)
            # phases 1, 2 read lo: one K loop.  Phase 1 carries the previous conv's set-B epilogue, which must have read
            # set B out before phase 2 starts it afresh; set B's initial value is fetched once set A's first step is out
            lo = self.phase_grans("A", 0, True) + self.phase_grans("B", 0, True)
            main.append(("start", "epiB", pendingB))
            marks = {1: self.init_loads("B", row), 18: [("flush", "epiB")] + (self.stamp() if l == 1 else [])}
            if l < L:
                marks[19] = self.init_loads("A", nxt)
            main += self.kloop(g, lo, 3, marks)
            g += 36
            if l == 1:
                main += self.stamp()
            # phases 3, 4 read hi: every wave's set-B epilogue must be in LDS
            main.append(wlw)
            hi = self.phase_grans("A", 1, False) + self.phase_grans("B", 1, False)
            marks = {18: (self.stamp() if l == 1 else []) + [("start", "epiA", self.epi_layer("A", 0))]}
            main += self.kloop(g, hi, 3, marks)
            g += 36
            main.append(("flush", "epiA"))
            main.append(wlw)
            main += self.stamp()
            pendingB = self.epi_layer("B", 1)
        # -- last layer's set B epilogue: exposed (the expand reads lo and hi from its first step) ----------------
        main.append(bar)                               # every wave is done reading hi
        main += pendingB
        main.append(wlw)
        main += self.stamp()
        # -- expand: four quarters of 64 output channels, sets A, B, A, B; a quarter's epilogue (residual add, x' -> HBM)
        # rides under the next quarter's K loop; the residual pieces alternate between the two X buffers -------------
        main += self.r_loads(0, 0, "r0")
        main += self.r_loads(1, 1, "r1")
        for qo in range(4):
            sset = "AB"[qo % 2]
            gr = [(sset, None if s == 0 else False, [(1, 1, 2 * s + j) for j in range(2)]) for s in range(4)]
            main += self.kloop(g, gr, 4)
            g += 4
            if qo > 0:
                main.append(("flush", f"xe{qo - 1}"))
                if qo + 1 < 4:
                    main += self.r_loads(qo + 1, (qo + 1) % 2, f"r{qo + 1}")
            main.append(("start", f"xe{qo}", self.epi_expand(qo, sset, qo % 2)))
        main.append(("flush", "xe3"))
        main += self.stamp()
        assert g == self.ngran, (g, self.ngran)
        # every wave is past the last K loop before the ring and the act buffer are reused
        main.append(bar)
        return main

    # ---- whole kernel ---------------------------------------------------------------------------
    def kernel(self, name):
        e = self.e
        self.kname = name
        e.raw(f"\t.globl\t{name}\n\t.p2align\t8\n\t.type\t{name},@function")
        e.label(name)
        # ---- prologue --------------------------------------------------------------------------
        e.raw("\ts_load_dwordx8 s[4:11], s[0:1], 0x0")       # x, wstream, prm, npos, nblk
        e.raw("\ts_load_dwordx4 s[12:15], s[0:1], 0x20")     # nwg, pad, stamps
        e.raw("\tv_and_b32 v101, 63, v0")                       # lane
        e.raw("\tv_lshrrev_b32 v102, 6, v0")                    # wave
        e.raw("\ts_nop 3")                                       # a VGPR write -> v_readfirstlane of it needs a wait state
        e.raw(f"\tv_readfirstlane_b32 s{S_WAVE}, v102")
        e.raw("\tv_and_b32 v103, 31, v101")                     # n
        e.raw("\tv_lshrrev_b32 v104, 5, v101")                  # h
        e.raw("\ts_nop 4")
        for k in range(3):
            e.raw(f"\tv_lshlrev_b32 v{V_DMAOFF + k}, 4, v0")
            if k:
                e.raw(f"\tv_add_u32 v{V_DMAOFF + k}, {4096 * k}, v{V_DMAOFF + k}")
        e.raw(f"\tv_lshlrev_b32 v{V_ARING}, 4, v101")
        e.raw(f"\tv_add_u32 v{V_ARING}, {RING0}, v{V_ARING}")
        for b in range(3):
            e.raw(f"\ts_lshl_b32 s{S_TMP}, s{S_WAVE}, 5")
            e.raw(f"\ts_add_u32 s{S_TMP}, s{S_TMP}, {128 * b}")
            e.raw(f"\tv_add_u32 v105, s{S_TMP}, v103")               # r = 32 t + n
            # fragment base: r * SLOTB + h * 16   (rowshift of tap (0, 0) is -PADTOP: cancels PADTOP)
            e.raw(f"\tv_mul_u32_u24 v106, {SLOTB}, v105")
            e.raw(f"\tv_lshl_add_u32 v{V_BROW + b}, v104, 4, v106")
            e.raw(f"\tv_add_u32 v109, {PADTOP}, v105")
            e.raw(f"\tv_mul_u32_u24 v109, {SLOTB}, v109")
            e.raw(f"\tv_lshl_add_u32 v{V_WROW + b}, v104, 4, v109")
            # board point: y = r / 20, x = r % 20; on the board iff x < 19 and y < 19
            e.raw("\tv_mul_u32_u24 v110, 3277, v105")
            e.raw("\tv_lshrrev_b32 v110, 16, v110")                   # y = r * 3277 >> 16 (r < 1024)
            e.raw("\tv_mul_u32_u24 v111, 20, v110")
            e.raw("\tv_sub_u32 v111, v105, v111")                     # x
            e.raw("\tv_cmp_gt_u32 vcc, 19, v111")
            e.raw(f"\tv_cmp_gt_u32 s[{S_OK + 2 * b}:{S_OK + 2 * b + 1}], 19, v110")
            e.raw(f"\ts_and_b64 s[{S_OK + 2 * b}:{S_OK + 2 * b + 1}], s[{S_OK + 2 * b}:{S_OK + 2 * b + 1}], vcc")
            e.raw("\tv_mul_u32_u24 v112, 19, v110")
            e.raw("\tv_add_u32 v112, v112, v111")                     # loc
            e.raw(f"\tv_cndmask_b32 v112, 0, v112, s[{S_OK + 2 * b}:{S_OK + 2 * b + 1}]")
            e.raw("\tv_lshlrev_b32 v112, 4, v112")                    # loc * 16
            e.raw(f"\tv_mul_u32_u24 v113, {CBLK_BYTES}, v104")
            e.raw(f"\tv_add_u32 v{V_XOFF + b}, v112, v113")
        e.raw(f"\tv_lshlrev_b32 v{V_HOFF}, 4, v104")
        e.raw(f"\tv_lshlrev_b32 v{V_POFF}, 5, v104")
        e.raw(f"\tv_mov_b32 v{V_C1}, {f32hex(-2.0 * LN2)}")
        e.raw(f"\tv_mov_b32 v{V_C2}, {f32hex(LN2)}")
        for i in range(4):
            e.raw(f"\tv_mov_b32 v{V_ZERO + i}, 0")
        e.raw(f"\ts_lshl_b32 s{S_RINGW}, s{S_WAVE}, 10")
        e.raw(f"\ts_add_u32 s{S_RINGW}, s{S_RINGW}, {RING0}")       # M0 base: the wave's 1 KiB piece of ring slot 0
        # zero the act buffer (the halo slots stay zero for the whole launch: epilogues write on-board rows only)
        e.raw("\tv_lshlrev_b32 v100, 4, v0")
        e.raw("\tv_mov_b32 v101, v100")
        nz = (ACT_BYTES + 4095) // 4096
        for i in range(nz):
            last = ACT_BYTES - i * 4096
            if last < 4096:
                e.raw(f"\tv_cmp_gt_u32 vcc, {last}, v101")
                e.raw("\ts_and_saveexec_b64 s[36:37], vcc")
            e.raw(f"\tds_write_b128 v100, v[{V_ZERO}:{V_ZERO + 3}]")
            if last < 4096:
                e.raw("\ts_mov_b64 exec, s[36:37]")
            else:
                e.raw("\tv_add_u32 v100, 4096, v100")
        e.raw("\ts_waitcnt lgkmcnt(0)")
        # flat loop state
        e.raw(f"\ts_mov_b32 s{S_POS}, s{S_WG}")
        e.raw(f"\ts_mov_b32 s{S_BLK}, 0")
        e.raw(f"\ts_cmp_ge_u32 s{S_POS}, s{S_NPOS}")
        e.raw(f"\ts_cbranch_scc0 .L{name}_go")
        self.long_jump(e, f".L{name}_end", False)
        e.label(f".L{name}_go")
        self.set_position(e)
        e.raw(f"\ts_mov_b64 s[{S_DMA}:{S_DMA + 1}], s[{S_WS}:{S_WS + 1}]")
        e.raw(f"\ts_mov_b64 s[{S_PB}:{S_PB + 1}], s[{S_PRM}:{S_PRM + 1}]")
        e.raw("\ts_barrier")
        if self.stop:
            if self.stop.startswith("dump"):
                self.dump_and_end(e, tuple(self.stop.split("_")[1:]))
                e.label(f".L{name}_end")
                return
            pieces = {"prologue": [], "store": [], "xloads": self.x_loads(0, 0, "x0") + self.x_loads(1, 1, "x1"),
                      "prm": self.act_loads(0, 0), "dma": [it for g in range(0, NSLOT, 3) for it in self.dma_group(g, 3)]}
            for it in pieces[self.stop]:
                e.emit(it)
            e.raw("\ts_waitcnt vmcnt(0) lgkmcnt(0)")
            if self.stop != "prologue":
                e.raw(f"\tv_mov_b32 v{TMP}, 0x3c003c00")
                e.raw(f"\tv_lshlrev_b32 v{TMP + 1}, 2, v0")
                e.raw(f"\tglobal_store_dword v{TMP + 1}, v{TMP}, s[{S_X}:{S_X + 1}]")
                e.raw("\ts_waitcnt vmcnt(0)")
            e.raw("\ts_endpgm")
            e.label(f".L{name}_end")
            return
        self.block_entry(e)
        e.label(f".L{name}_block")
        # loop-head state: the entry's operations (x quarters 0, 1; the first parameters; the block's first twelve granules)
        # are the youngest vector-memory operations; whatever is older (the previous block's stores) is never waited for by name
        want = ["x0"] * 12 + ["x1"] * 12 + ["prm"] * 4 + [("g", g) for g in range(NSLOT)]
        head = [t for (_, t) in e.vm[-40:]]
        assert head == want, head
        e.vm = list(e.vm[-40:])
        e.lgkm = []
        main = self.block_body()
        if self.opts.get("nofiller"):
            main = [it for it in main if not (isinstance(it, tuple) and it[0] in ("start", "flush"))]
        if self.opts.get("synthfill"):     # every filler stream replaced by that many independent plain VALU instructions
            n = self.opts["synthfill"]
            main = [(it[0], it[1], [valu("v_fma_f32", V(T0 + i % 8), V(V_C1), V(V_C2), V(T0 + i % 8)) for i in range(n)])
                    if (isinstance(it, tuple) and it[0] == "start") else it for it in main]
        if self.opts.get("noread"):        # K loops without their fragment reads
            main = [it for it in main if not (isinstance(it, Ins) and it.kind == "ds_r")]
        if self.opts.get("noprewait"):
            main = [it for it in main if not (isinstance(it, tuple) and it[0] == "call" and getattr(it[1], "__name__", "") == "<lambda>"
                                              and "need" in it[1].__code__.co_varnames)]
        e.weave(main, budget=self.opts.get("budget", 24))
        # ---- advance (position, block) -------------------------------------------------------------
        if self.diag:
            self.write_stamps(e)
        e.raw(f"\ts_add_u32 s{S_BLK}, s{S_BLK}, 1")
        e.raw(f"\ts_cmp_lt_u32 s{S_BLK}, s{S_NBLK}")
        e.raw(f"\ts_cbranch_scc1 .L{name}_next")
        e.raw(f"\ts_mov_b32 s{S_BLK}, 0")
        e.raw(f"\ts_add_u32 s{S_POS}, s{S_POS}, s{S_NWG}")
        e.raw(f"\ts_cmp_ge_u32 s{S_POS}, s{S_NPOS}")
        e.raw(f"\ts_cbranch_scc1 .L{name}_end")
        self.set_position(e)
        e.label(f".L{name}_next")
        # weights and parameters of the block about to run
        e.raw(f"\ts_mul_i32 s{S_TMP}, s{S_BLK}, {self.ngran * GRAN}")
        e.raw(f"\ts_add_u32 s{S_DMA}, s{S_WS}, s{S_TMP}")
        e.raw(f"\ts_addc_u32 s{S_DMA + 1}, s{S_WS + 1}, 0")
        e.raw(f"\ts_mul_i32 s{S_TMP}, s{S_BLK}, {self.prm_floats * 4}")
        e.raw(f"\ts_add_u32 s{S_PB}, s{S_PRM}, s{S_TMP}")
        e.raw(f"\ts_addc_u32 s{S_PB + 1}, s{S_PRM + 1}, 0")
        self.block_entry(e)
        head = [t for (_, t) in e.vm[-40:]]
        assert head == want, head
        self.long_jump(e, f".L{name}_block", True)
        e.label(f".L{name}_end")
        e.raw("\ts_waitcnt vmcnt(0) lgkmcnt(0)")
        e.raw("\ts_endpgm")
        e.label(f".L{name}_fend")
        e.raw(f"\t.size\t{name}, .L{name}_fend-{name}")

    def block_entry(self, e):
        """x quarters 0, 1 of the block about to run and its first bn0 parameters are requested first, then its first
        twelve granules: the DMA issue covers part of the loads' latency, the rest of it is the one exposed wait per block"""
        e.raw("\ts_waitcnt lgkmcnt(0)")
        e.lgkm = []
        for it in self.x_loads(0, 0, "x0") + self.x_loads(1, 1, "x1") + self.act_loads(0, 0):
            e.emit(it)
        for g in range(0, NSLOT, 3):
            for it in self.dma_group(g, 3):
                e.emit(it)

    def long_jump(self, e, target, backward):
        """s_branch reaches +-128 KiB; a block body is larger"""
        self.njump = getattr(self, "njump", 0) + 1
        here = f".Lpc{self.njump}_{self.kname}"
        e.raw(f"\ts_getpc_b64 s[{S_TMP}:{S_TMP + 1}]")
        e.label(here)
        e.raw(f"\ts_add_u32 s{S_TMP}, s{S_TMP}, {target}-{here}")
        e.raw(f"\ts_addc_u32 s{S_TMP + 1}, s{S_TMP + 1}, {-1 if backward else 0}")
        e.raw(f"\ts_setpc_b64 s[{S_TMP}:{S_TMP + 1}]")

    def set_position(self, e):
        # S_XP = x + pos * POS_BYTES
        e.raw(f"\ts_mul_i32 s{S_TMP}, s{S_POS}, {POS_BYTES}")
        e.raw(f"\ts_mul_hi_u32 s{S_TMP + 1}, s{S_POS}, {POS_BYTES}")
        e.raw(f"\ts_add_u32 s{S_XP}, s{S_X}, s{S_TMP}")
        e.raw(f"\ts_addc_u32 s{S_XP + 1}, s{S_X + 1}, s{S_TMP + 1}")

    def write_stamps(self, e):
        # stamps of (first position of workgroups 0..7, every block): [wg][blk][wave][24] u64
        n = self.nstamp
        e.raw(f"\ts_cmp_lg_u64 s[{S_STAMP}:{S_STAMP + 1}], 0")
        e.raw(f"\ts_cbranch_scc0 .Lnostamp_{self.kname}")
        e.raw(f"\ts_cmp_lt_u32 s{S_WG}, 8")
        e.raw(f"\ts_cbranch_scc0 .Lnostamp_{self.kname}")
        e.raw(f"\ts_cmp_eq_u32 s{S_POS}, s{S_WG}")
        e.raw(f"\ts_cbranch_scc0 .Lnostamp_{self.kname}")
        # offset = ((wg * 16 + blk) * 4 + wave) * 24 * 8
        e.raw(f"\ts_lshl_b32 s{S_TMP}, s{S_WG}, 4")
        e.raw(f"\ts_add_u32 s{S_TMP}, s{S_TMP}, s{S_BLK}")
        e.raw(f"\ts_lshl_b32 s{S_TMP}, s{S_TMP}, 2")
        e.raw(f"\ts_add_u32 s{S_TMP}, s{S_TMP}, s{S_WAVE}")
        e.raw(f"\ts_mul_i32 s{S_TMP}, s{S_TMP}, 192")
        e.raw(f"\ts_add_u32 s{S_TMP + 2}, s{S_STAMP}, s{S_TMP}")
        e.raw(f"\ts_addc_u32 s{S_TMP + 3}, s{S_STAMP + 1}, 0")
        e.raw(f"\ts_memrealtime {rtxt(S(S_T0 + 44, 2))}")              # slot 22: ... and behind its last
        e.raw(f"\ts_memtime {rtxt(S(S_T0 + 46, 2))}")                  # slot 23: shader clock at the same instant
        e.raw("\ts_waitcnt lgkmcnt(0)")
        e.raw(f"\tv_mov_b32 v{TMP}, 0")
        for k in list(range(n)) + [21, 22, 23]:
            e.raw(f"\tv_mov_b32 v{TMP + 2}, s{S_T0 + 2 * k}")
            e.raw(f"\tv_mov_b32 v{TMP + 3}, s{S_T0 + 2 * k + 1}")
            e.raw(f"\tglobal_store_dwordx2 v{TMP}, v[{TMP + 2}:{TMP + 3}], s[{S_TMP + 2}:{S_TMP + 3}] offset:{8 * k}")
        e.raw("\ts_waitcnt vmcnt(0)")
        e.label(f".Lnostamp_{self.kname}")




def descriptor(name, lds):
    return f"""
	.section	.rodata,"a",@progbits
	.p2align	6, 0x0
	.amdhsa_kernel {name}
		.amdhsa_group_segment_fixed_size {lds}
		.amdhsa_private_segment_fixed_size 0
		.amdhsa_kernarg_size 64
		.amdhsa_user_sgpr_count 2
		.amdhsa_user_sgpr_kernarg_segment_ptr 1
		.amdhsa_system_sgpr_workgroup_id_x 1
		.amdhsa_system_vgpr_workitem_id 0
		.amdhsa_next_free_vgpr 512
		.amdhsa_next_free_sgpr 96
		.amdhsa_accum_offset 256
		.amdhsa_reserve_vcc 1
		.amdhsa_float_round_mode_32 0
		.amdhsa_float_round_mode_16_64 0
		.amdhsa_float_denorm_mode_32 3
		.amdhsa_float_denorm_mode_16_64 3
		.amdhsa_dx10_clamp 1
		.amdhsa_ieee_mode 1
	.end_amdhsa_kernel
	.text
"""


def metadata(names, lds):
    ks = ""
    for n in names:
        ks += f"""  - .agpr_count:     256
    .args:
      - .offset:         0
        .size:           64
        .value_kind:     by_value
    .group_segment_fixed_size: {lds}
    .kernarg_segment_align: 8
    .kernarg_segment_size: 64
    .max_flat_workgroup_size: 256
    .name:           {n}
    .private_segment_fixed_size: 0
    .sgpr_count:     96
    .sgpr_spill_count: 0
    .symbol:         {n}.kd
    .uniform_work_group_size: 1
    .vgpr_count:     512
    .vgpr_spill_count: 0
    .wavefront_size: 64
"""
    return f"""	.amdgpu_metadata
---
amdhsa.kernels:
{ks}amdhsa.target:   amdgcn-amd-amdhsa--gfx950
amdhsa.version:
  - 1
  - 2
...
	.end_amdgpu_metadata
"""


def main():
    out = sys.argv[1]
    variants = [(L, d, None) for L in (1, 2, 3) for d in (False, True)]
    if len(sys.argv) > 2:
        variants = [(int(sys.argv[2]), False, int(sys.argv[3]) if len(sys.argv) > 3 else None)]
    text = '\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"\n\t.text\n'
    names = []
    for L, diag, dump in variants:
        name = f"k_blockw_L{L}" + ("_diag" if diag else "")
        g = BlockGen(L, diag, dump)
        g.kernel(name)
        text += g.e.text() + descriptor(name, LDS_BYTES)
        names.append(name)
        print(name, g.e.stats, "lines", len(g.e.lines), file=sys.stderr)
    text += metadata(names, LDS_BYTES)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
