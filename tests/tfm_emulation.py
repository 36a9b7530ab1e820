"""CPU emulation of the transformer trunk one kernel at a time, at the engine's fp16 points, and the kernel checker.

TEST INFRASTRUCTURE ONLY: used by tests/test_transformer_emulation_cpu.py and tests/test_transformer_blocks_gpu.py.
The block is the one of tests/tfm_restatement_dh.py, in its three stages qkv_stage / attn_stage / ffn_stage (the three
launches of csrc/transformer.hip); what is written here is the entry points on the engine's own tensors, the attention
kernel's own softmax, the twin, the mutants and the checker.  Every entry point starts from the tensor the engine
itself read (teacher forcing: HipEngine.debug_x and debug_tfm on engines stopped by P3HIP_DEBUG_STOP_BLOCK), so errors
do not cascade and every kernel of every block is judged on its own.

Layouts: x and o are token-major [N][361][d] (d the model width; the stream's padding channels d..Cs-1 are not part of
the emulation, the GPU test holds them to exact zero); q, k, v are the engine's [N][head][361][D] without the 23
padding rows.  Tokens are s = 19 row + col.

Modes (`Tfm(cfg, W, fp16=..., twin=...)`):
  * fp16=False: the float64 restatement stage by stage (bit for bit tfm_restatement_dh.forward).
  * fp16=True: round-to-nearest-even to fp16 at the points below, everything else in float64.
  * twin=True (implies fp16): the same fp16 points with fp32 arithmetic done another way than the kernels do it:
    float32 torch matmuls (another summation order than the MFMA k loops), exp2 of log2(e)-scaled scores, RMSNorm with
    torch.rsqrt and SiLU as x / (1 + exp(-x)) in fp32.  It is the benign stand-in for the GPU that sets BOUNDS.

fp16 points, kernel by kernel (every accumulation is fp32 on the MFMAs; weights of the six GEMMs are fp16 A fragments,
plan.cpp pack_afrag; the RMSNorm scales and the RoPE tables are fp32):
  k_tfm_qkv   * the source rows are the stored fp16 x, widened to fp32; RMSNorm_in in fp32 (sum of squares, rsqrtf of
                mean + 1e-6, times scale) and its result the fp16 LDS tile xs (rms_rows, `dst[..] = (_Float16)(..)`).
              * q, k, v = xs . [Wq | Wk | Wv] in fp32; RoPE on q and k in fp32 on the accumulators; one rounding at the
                store (`h4{(_Float16)y[0], ..}`).
  k_tfm_attn  * operands q, k, v as stored.  Scores are fp32, scaled by log2(e) / sqrt(D) after the MFMA.
              * D = 32: numerators exp2(s - m), m the row's maximum over the 361 keys; their fp32 values are summed,
                their fp16 roundings are the P operand of O^T = V^T . P^T.
              * D = 64: the same per block of 64 keys with the running maximum m_b up to and including the block;
                o and the sum are multiplied by alpha = exp2(m_(b-1) - m_b) in fp32 before the block is added.  A
                numerator is therefore rounded to fp16 relative to the running maximum of its block, not the row's,
                and rescaled afterwards in fp32: a numerator that the row-maximum form flushes or rounds on the
                subnormal grid keeps 11 bits when its block's running maximum was lower.  Measured on the emulation
                (test_online_softmax_form_is_not_the_row_maximum_form): the two forms are never more than one rounding
                of o apart (0.85 checker units on the fixtures, 0.81 hot) but differ in 6.6 - 8.4 % of the elements
                of o on the fixtures (Wq, Wk x 1.5) and in 2.7 - 2.9 % hot (x 4.0: a peaked row is carried by one
                key).  tfm_restatement_dh's argument that they are equal holds to that one rounding; it is enough to
                miss attn_d64's fraction bit-identical, so the emulation does what the kernel does.
              * o = acc * (1 / sum) in fp32, one rounding at the store.
  k_tfm_ffn   * operand o as stored; x1 = o . Wo + x in fp32, never rounded (LDS fp32 rows at C <= 96, registers at
                C >= 128: the same values); RMSNorm_out of x1 in fp32, its result the fp16 tile xs.
              * gate and up in fp32; silu(gate) * up rounded into the fp16 tile hs.
              * x_next = fp16(hs . Wdown + x1), one rounding at the store.
`flush_subnormals=True` is the named switch for MFMAs that would read fp16-subnormal operands as zero: every operand
of the attention kernel (q, k, v, P) below 2^-14 in magnitude becomes 0.  The two settings are far apart in the
checker's measure (o of block 0: 81 - 90 % bit-identical, err up to 6.1 on the fixtures and 1.6 hot;
test_subnormal_switch_is_visible_to_the_checker), and the MI355X matched the default, False: its MFMAs honour
fp16-subnormal operands (TWIN's MI355X column, 99.8 % of o bit-identical, was measured with False).

The checker is trunk_emulation.check_block on [n][channels][361] views: err = |engine - emulation| / (ulp16(emulation)
+ FLOOR_REL * scale) and the fraction bit-identical; scale is the RMS of the emulated tensor for q, k, v and o, and
trunk_emulation.block_scale (the larger RMS of input and branch) for x.  Its message names the kernel and tensor, the
block, the slot, the channel, its group of 8 and its head, and the token (row, col; corner / edge / interior).
"""
from __future__ import annotations

import os
import sys
from typing import Dict, Optional

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tfm_restatement as tfm  # noqa: E402
import tfm_restatement_dh as dh  # noqa: E402
import trunk_emulation as te  # noqa: E402

F64 = torch.float64
L, LPAD = 361, 384
LOG2E = 1.4426950408889634
MASKED = -3.0e38
KEY_BLOCK = 64          # keys per block of the D = 64 online softmax
HOT_SCALE = 4.0         # hot_weights: Wq and Wk of the seeded init times this (the fixtures: 1.5)

# family: the twin's worst (largest err, lowest fraction bit-identical) over the eight fixture nets, plain and hot
# (test_twin_passes_the_checker), and over every job of tests/test_transformer_blocks_gpu.py
# (test_twin_on_the_gpu_test_batches); both tests hold the twin to these figures.  Then what one MI355X measured on
# the jobs of tests/test_transformer_blocks_gpu.py (its stem: 0.91 / 1.000).
TWIN = {                                  # MI355X: err / identical
    "qkv": (0.884, 0.9937),               # 0.85 / 0.996
    "attn_d32": (0.846, 0.9971),          # 0.84 / 0.998
    "attn_d64": (0.850, 0.9960),          # 0.85 / 0.998
    "ffn_small": (1.398, 0.9899),         # 1.05 / 0.993
    "ffn_wide": (1.273, 0.9443),          # 1.14 / 0.972
    "qkv hot": (0.884, 0.9931),           # 0.86 / 0.996
    "attn_d32 hot": (1.133, 0.9973),      # 1.04 / 0.998
    "attn_d64 hot": (1.661, 0.9960),      # 1.10 / 0.998
    "ffn_small hot": (1.239, 0.9907),     # 1.17 / 0.996
    "ffn_wide hot": (1.293, 0.9573),      # 0.95 / 0.979
}


def _rule(err, ident):
    """trunk_emulation.BOUNDS' rule: twice the twin's worst err rounded up to the next 0.5 (the margin of 1.6x - 2.2x
    that table keeps; it covers the MFMA's summation order, which the twin only approximates), and the twin's lowest
    fraction bit-identical minus 0.05."""
    return float(np.ceil(2.0 * err / 0.5) * 0.5), float(np.floor((ident - 0.05) * 1000) / 1000)


# family: (max err, lowest fraction bit-identical): qkv 2.0 / 0.943, attn_d32 2.0 / 0.947, attn_d64 2.0 / 0.946,
# ffn_small 3.0 / 0.939, ffn_wide 3.0 / 0.894; hot: qkv 2.0 / 0.943, attn_d32 2.5 / 0.947, attn_d64 3.5 / 0.946,
# ffn_small 2.5 / 0.940, ffn_wide 3.0 / 0.907.  The stem is held to trunk_emulation.BOUNDS["stem"] (the same k_init).
BOUNDS = {f: _rule(*v) for f, v in TWIN.items()}


def hot_weights(name, scale=HOT_SCALE):
    """(cfg, W): the fixture weights of `name` with Wq and Wk scaled by `scale` instead of 1.5: peaked attention."""
    return dh.fixture_weights(name, scale)


def family(cfg, kernel, hot=False):
    """The BOUNDS key of a kernel ("qkv", "attn", "ffn") of cfg."""
    D = cfg.channels // cfg.bottleneck_channels
    f = {"qkv": "qkv", "attn": f"attn_d{D}", "ffn": "ffn_small" if cfg.channels <= 96 else "ffn_wide"}[kernel]
    return f + (" hot" if hot else "")


def tokens(x_debug, d):
    """HipEngine.debug_x's [n][Cs][361] -> the model's channels token-major [n][361][d], float64."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x_debug, np.float64)[:, :d].transpose(0, 2, 1)))


def _t(a, dt=F64):
    return a.to(dt) if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, np.float64)).to(dt)


class Tfm:
    """The transformer trunk of one network, kernel by kernel.  `mutate` injects the slips of
    tests/test_transformer_emulation_cpu.py into the twin (a dict with "kind" and where)."""

    def __init__(self, cfg, W: Dict[str, np.ndarray], fp16: bool = True, twin: bool = False,
                 mutate: Optional[dict] = None, flush_subnormals: bool = False):
        self.cfg = cfg
        self.fp16 = fp16 or twin
        self.twin = twin
        self.mut = mutate or {}
        self.flush = flush_subnormals
        self.d, self.nh = cfg.channels, cfg.bottleneck_channels
        self.D = self.d // self.nh
        self.W = W
        self.W16 = {k: (v.astype(np.float16).astype(np.float32) if k.startswith("blocks.") and k.endswith(".w") else v)
                    for k, v in W.items()} if self.fp16 else W
        self.dt = torch.float32 if twin else F64
        self._stem = te.Trunk(cfg, W, fp16=self.fp16, twin=twin)
        cos, sin = tfm.rope_tables(head_dim=self.D)
        # the engine's tables are fp32 (plan.cpp: spiral_rope_table in double, stored as float)
        self.cos, self.sin = (torch.from_numpy(a.astype(np.float32) if twin else a).to(self.dt) for a in (cos, sin))

    # ---- helpers --------------------------------------------------------------------------------------------------
    def r16(self, x):
        return x.half().to(x.dtype) if self.fp16 else x

    def w(self, i, n):
        """weight `n` of block i as the GEMM reads it; the WTILE mutant: one 16-channel output tile from its neighbour"""
        t = torch.from_numpy(np.asarray(self.W16[f"blocks.{i}.{n}"], np.float64)).to(self.dt)
        m = self.mut
        if m.get("kind") == "WTILE" and m["block"] == i and m["weight"] + ".w" == n:
            t = t.clone()
            c = 16 * m["tile"]
            t[:, c:c + 16] = t[:, c + 16:c + 32]
        return t

    def _m(self, kind, i=None):
        return self.mut.get("kind") == kind and (i is None or self.mut.get("block", i) == i)

    def rms32(self, x, scale, eps=1e-6):
        inv = torch.rsqrt((x * x).sum(-1, keepdim=True) * np.float32(1.0 / x.shape[-1]) + np.float32(eps))
        return (x * inv * scale).half().float()

    # ---- entry points ---------------------------------------------------------------------------------------------
    def stem(self, features=None, planes=None, scalars=None):
        """x0 [N][361][d]: fp16(init_conv(planes) + init_game(scalars)), k_init as trunk_emulation states it."""
        x = self._stem.stem(features, planes, scalars)
        return x.reshape(x.shape[0], self.d, L).permute(0, 2, 1).contiguous()

    def qkv(self, i, x):
        """k_tfm_qkv of block i on x [N][361][d] -> q, k, v [N][head][361][D]."""
        x = _t(x)
        if not self.twin:
            return tuple(a.permute(0, 2, 1, 3).contiguous() for a in dh.qkv_stage(x, self.W16, i, self.nh, self.fp16))
        N = x.shape[0]
        x = x.float()
        scale = _t(self.W[f"blocks.{i}.rms_in.scale"], torch.float32)
        h = self.rms32(x, scale, 1e-5 if self._m("EPS", i) and self.mut["norm"] == "in" else 1e-6)
        row = torch.arange(L).repeat(N)
        if self._m("ROPEROW", i):
            # a 64-token tile that spans two positions: the tokens of the second one take the table row of their index
            # counted from the tile's first position (361 + s), clamped to the table's last row
            g = torch.arange(N * L)
            first = (g // 64 * 64) // L
            row = torch.clamp(g - first * L, max=L - 1)
        cos, sin = self.cos[row].reshape(N, L, 1, self.D), self.sin[row].reshape(N, L, 1, self.D)
        out = []
        for n in ("q", "k", "v"):
            a = (h @ self.w(i, n + ".w")).reshape(N, L, self.nh, self.D)
            if n != "v":
                if self._m("ROPESWAP", i):   # one head's pairs taken in the other order: (x[2j+1], x[2j])
                    hd = self.mut["head"]
                    a = a.clone()
                    a[:, :, hd] = a[:, :, hd].reshape(N, L, -1, 2).flip(-1).reshape(N, L, self.D)
                a = tfm._rope(a, cos, sin)
            out.append(a.half().double().permute(0, 2, 1, 3).contiguous())
        return tuple(out)

    def attn(self, q, k, v):
        """k_tfm_attn on q, k, v [N][head][361][D] -> o [N][361][d]."""
        q, k, v = _t(q), _t(k), _t(v)
        if not self.fp16 or (self.D == 32 and not self.twin and not self.flush):
            return dh.attn_stage(*(a.permute(0, 2, 1, 3) for a in (q, k, v)), self.fp16)
        return self.attn_kernel(q, k, v)[0]

    def attn_kernel(self, q, k, v, online=None):
        """The kernel's own softmax on 384 keys (23 masked), scores in log2 units: the whole row at D = 32, online over
        blocks of 64 keys at D = 64 (`online` overrides).  Returns (o [N][361][d], the running maxima [6 or 1][N][head][361])."""
        dt = self.dt
        N, H, _, D = q.shape
        online = (D == 64) if online is None else online
        if self.flush:
            q, k, v = (torch.where(a.abs() < 2.0 ** -14, torch.zeros_like(a), a) for a in (q, k, v))
        q, k, v = q.to(dt), k.to(dt), v.to(dt)
        pad = torch.zeros(N, H, LPAD - L, D, dtype=dt)
        k, v = torch.cat([k, pad], 2), torch.cat([v, pad], 2)
        m_ = self.mut
        if m_.get("kind") == "KSHIFT":       # the K rows of the last 16-key tile with keys (352..367) one row late
            k = k.clone()
            k[:, :, 352:367] = k[:, :, 353:368].clone()
        kscale = np.float32(LOG2E) / np.float32(np.sqrt(D)) if self.twin else LOG2E / np.sqrt(D)
        s = (q @ k.transpose(-1, -2)) * kscale                 # [N][H][361 queries][384 keys]
        s[..., L:] = MASKED
        if m_.get("kind") == "PADKEY":       # one padding key left unmasked: its k is zero, so its score is 0
            s[..., m_["key"]] = 0.0
        if m_.get("kind") == "K360":         # the last, partial 16-query step of one head loses key 360
            s[:, m_["head"], 352:L, 360] = MASKED
        step = KEY_BLOCK if online else LPAD
        o = torch.zeros(N, H, L, D, dtype=dt)
        tot = torch.zeros(N, H, L, dtype=dt)
        m = torch.full((N, H, L), MASKED, dtype=dt)
        maxima = []
        for b in range(0, LPAD, step):
            sb = s[..., b:b + step]
            mb = torch.maximum(m, sb.amax(-1))
            alpha = torch.exp2(m - mb)
            if m_.get("kind") == "ALPHA0":   # a rescale by less than 2^-8 taken for "nothing earlier matters"
                alpha = torch.where(alpha < 2.0 ** -8, torch.zeros_like(alpha), alpha)
            m = mb
            maxima.append(m)
            tot = tot * alpha
            if not m_.get("kind") == "NORESCALE":
                o = o * alpha[..., None]
            e = torch.exp2(sb - m[..., None])
            tot = tot + e.sum(-1)
            p = self.r16(e)
            if self.flush:
                p = torch.where(p < 2.0 ** -14, torch.zeros_like(p), p)
            o = o + p @ v[:, :, b:b + step]
        o = o * (1.0 / tot)[..., None]
        o = self.r16(o).double().permute(0, 2, 1, 3).reshape(N, L, H * D)
        return o, torch.stack(maxima).double()

    def ffn(self, i, o, x):
        """k_tfm_ffn of block i on o and x [N][361][d] -> the next x [N][361][d]."""
        o, x = _t(o), _t(x)
        if not self.twin:
            return dh.ffn_stage(o, x, self.W16, i, self.fp16)
        o, x = o.float(), x.float()
        x1 = o @ self.w(i, "o.w") + x
        scale = _t(self.W[f"blocks.{i}.rms_out.scale"], torch.float32)
        h = self.rms32(x1, scale, 1e-5 if self._m("EPS", i) and self.mut["norm"] == "out" else 1e-6)
        g, u = h @ self.w(i, "ffn_gate.w"), h @ self.w(i, "ffn_up.w")
        if self._m("SILUSWAP", i):           # one 16-channel tile of the SwiGLU tile: silu(up) * gate
            c = 16 * self.mut["tile"]
            g, u = g.clone(), u.clone()
            g[..., c:c + 16], u[..., c:c + 16] = u[..., c:c + 16].clone(), g[..., c:c + 16].clone()
        hs = (g / (1.0 + torch.exp(-g)) * u).half().float()
        return (hs @ self.w(i, "ffn_down.w") + x1).half().double()

    def block(self, i, x):
        """{"q", "k", "v", "o", "x"}: what the three kernels of block i leave, chained from x."""
        q, k, v = self.qkv(i, x)
        o = self.attn(q, k, v)
        return {"q": q, "k": k, "v": v, "o": o, "x": self.ffn(i, o, x)}

    def trunk(self, features=None, planes=None, scalars=None):
        """{"x": [x0 .. x_B], "q" / "k" / "v" / "o": one per block}: the whole trunk, chained."""
        rec = {"x": [self.stem(features, planes, scalars)], "q": [], "k": [], "v": [], "o": []}
        for i in range(self.cfg.blocks):
            b = self.block(i, rec["x"][-1])
            for key in ("q", "k", "v", "o"):
                rec[key].append(b[key])
            rec["x"].append(b["x"])
        return rec

    def heads(self, x):
        """raw [N][1889] of the trunk output x [N][361][d] (trunk_emulation.Trunk.heads)."""
        x = _t(x)
        return self._stem.heads(x.permute(0, 2, 1).reshape(x.shape[0], self.d, 19, 19))

    def forward(self, features=None, planes=None, scalars=None):
        return self.heads(self.trunk(features, planes, scalars)["x"][-1])


# ---- the hot regime ------------------------------------------------------------------------------------------------

def attention_regime(emu: Tfm, q, k):
    """What the softmax of one block meets, from emulated (or engine) q, k [N][head][361][D], scores in log2 units:
    peak: the mean largest attention probability; tiny: the share of numerators below 2^-24 of their row's maximum;
    subnormal: the share in [2^-24, 2^-14); late: the share of rows whose maximum is among keys 320..360;
    step8: the share of rows whose running maximum over blocks of 64 keys rises by 8 or more in one step after the
    first block (alpha <= 2^-8: o and the sum really are rescaled)."""
    q, k = _t(q), _t(k)
    s = (q @ k.transpose(-1, -2)) * (LOG2E / np.sqrt(q.shape[-1]))
    m = s.amax(-1, keepdim=True)
    e = torch.exp2(s - m)
    run = torch.stack([s[..., :b + KEY_BLOCK].amax(-1) for b in range(0, L, KEY_BLOCK)])
    return {
        "peak": float((e.amax(-1) / e.sum(-1)).mean()),
        "tiny": float((s - m < -24).double().mean()),
        "subnormal": float(((s - m >= -24) & (s - m < -14)).double().mean()),
        "late": float((s.argmax(-1) >= 320).double().mean()),
        "step8": float(((run[1:] - run[:-1]).amax(0) >= 8).double().mean()),
    }


# ---- the checker ---------------------------------------------------------------------------------------------------

def _cm(a):
    """[n][head][361][D] or [n][361][d] -> [n][channels][361] (channel = head * D + lane of the head)."""
    a = np.asarray(a, np.float64)
    if a.ndim == 4:
        return a.transpose(0, 1, 3, 2).reshape(a.shape[0], -1, a.shape[2])
    return a.transpose(0, 2, 1)


def check_kernel(kernel, tensor, block, engine, emu, scale, head_width, slots=None, label="", bound=(16.0, 0.0)):
    """trunk_emulation.check_block on one tensor a kernel wrote; the message starts `block <label><block> <kernel>
    <tensor>` and names slot, channel, group of 8, head and token of the worst element."""
    return te.check_block(_cm(engine), _cm(emu), scale, f"{label}{block} {kernel} {tensor}", slots, *bound,
                          head_width=head_width)


def check_qkv(emu: Tfm, i, x, q, k, v, slots=None, label="", hot=False):
    b = BOUNDS[family(emu.cfg, "qkv", hot)]
    out = {}
    for name, got, want in zip("qkv", (q, k, v), emu.qkv(i, x)):
        out[name] = check_kernel("k_tfm_qkv", name, i, got, want, te.rms(want), emu.D, slots, label, b)
    return out


def check_attn(emu: Tfm, i, q, k, v, o, slots=None, label="", hot=False):
    want = emu.attn(q, k, v)
    return check_kernel("k_tfm_attn", "o", i, o, want, te.rms(want), emu.D, slots, label,
                        BOUNDS[family(emu.cfg, "attn", hot)])


def check_ffn(emu: Tfm, i, o, x, x_next, slots=None, label="", hot=False):
    want = emu.ffn(i, o, x)
    return check_kernel("k_tfm_ffn", "x", i, x_next, want, te.block_scale(_cm(x), _cm(want)), emu.D, slots, label,
                        BOUNDS[family(emu.cfg, "ffn", hot)])


def teacher_forced(emu: Tfm, rec, features=None, planes=None, scalars=None, slots=None, label="", hot=False):
    """Check the stem and the three kernels of every block from the engine's own tensors: rec = {"x": [x0 .. x_B],
    "q", "k", "v", "o": one per block} in this module's layouts.  Returns {"stem" or (kernel, block): stats}; the
    statistics of qkv are the worst of its three tensors."""
    x0 = emu.stem(features, planes, scalars)
    out = {"stem": te.check_block(_cm(rec["x"][0]), _cm(x0), te.rms(x0), f"{label}stem", slots, *te.bounds(emu.cfg, "stem"))}
    for i in range(len(rec["x"]) - 1):
        st = check_qkv(emu, i, rec["x"][i], rec["q"][i], rec["k"][i], rec["v"][i], slots, label, hot)
        out[("qkv", i)] = {"max_err": max(s["max_err"] for s in st.values()),
                           "identical": min(s["identical"] for s in st.values())}
        out[("attn", i)] = check_attn(emu, i, rec["q"][i], rec["k"][i], rec["v"][i], rec["o"][i], slots, label, hot)
        out[("ffn", i)] = check_ffn(emu, i, rec["o"][i], rec["x"][i], rec["x"][i + 1], slots, label, hot)
    return out


def collect(fam: dict, cfg, stats, hot=False):
    """Fold teacher_forced's statistics into {family: [lowest fraction identical, largest err]}."""
    for key, s in stats.items():
        f = "stem" if key == "stem" else family(cfg, key[0], hot)
        a = fam.setdefault(f, [1.0, 0.0])
        a[0], a[1] = min(a[0], s["identical"]), max(a[1], s["max_err"])
    return fam
