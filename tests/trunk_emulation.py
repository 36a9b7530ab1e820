"""CPU emulation of the convolutional trunks at the engine's fp16 storage points, and the block checker.

TEST INFRASTRUCTURE ONLY: used by tests/test_trunk_emulation_cpu.py and tests/test_trunk_blocks_gpu.py.  The layer
helpers come from oracle/torch_restatement.py (the float64 restatement of the reference's model.py); what is written
here is where the engine rounds.  Every entry point can be called on its own, so a GPU test can start block k from the
engine's own x after block k - 1 (teacher forcing) and judge one block at a time.

Modes (`Trunk(cfg, W, fp16=..., twin=...)`):
  * fp16=False: the float64 restatement, re-staged block by block (equal to oracle/torch_restatement.forward to 1e-9).
  * fp16=True: round-to-nearest-even to fp16 at the storage points below, every other value in float64 (accumulation,
    the folded BN scale and shift, mish).  This is the scheme the engine computes, without its fp32 arithmetic.
  * twin=True (implies fp16): the same storage points with the engine's fp32 arithmetic done another way: float32
    torch convolutions (another summation order than the MFMA K loops), the BN fold in fp32 as plan.cpp fold_bn does,
    and mish in fp32 by the engine's formulas (conv_core.h mish_t2 in the fused block kernel, mish_f elsewhere).  It is
    a benign stand-in for the GPU: the checker's thresholds are set so that it passes on every fixture and block.

Storage points (where the engine writes fp16; every accumulation is fp32 on the MFMAs):
  * weights of every trunk conv and of the broadcast dense (plan.cpp build_plan packs them as _Float16 streams); the
    head convs conv_p, conv_g and value.conv likewise (k_headsx stages them as fp16 A fragments).  The dense biases,
    the game-state dense of the stem and the BN parameters stay fp32.
  * the folded BN: scale = gamma / sqrt(var + eps), shift = beta - mean * scale in fp32 (plan.cpp fold_bn, about
    line 413); the fused block kernel multiplies both by log2(e) once more (conv_core.h scale_log2e).
  * x after the stem: fp16(conv5x5(planes) + game dense) (kernels.hip k_init epilogue, `o[i] = (_Float16)(acc + bias)`).
  * x after every residual block: fp16(x16 + branch) with the branch and the sum in fp32 (conv_core.h epilogue_store,
    residual_add; the C = 128 / 256 form in conv16.h epilogue_store16_act).
  * every activated conv input mish(bn(.)): fp16 in the act buffer (LDS) or, layer-wise, in HBM (conv_core.h
    bn_mish4_l2 / epilogue_layer, stage_math / stage_store; kernels.hip k_lconv `activate` + epilogue_store).
  * the nbt block's raw inner stream t after the reduce conv and after the first pair: fp16 in HBM scratch, while the
    next conv's activation is taken from the fp32 accumulator (kernels.hip k_block, "nbt: the raw inner residual stream
    t is parked in HBM scratch"; k_lconv DUAL without RES).
  * broadcast blocks: t = fp16(mish(conv_first(mish(bn0(x16))))) (k_conv1x1 EPI 0 or the fused tail of k_block) and
    u = fp16(mish(bn1(dense(t) + b))) (k_bdense / bdense_passes).
Which value the next block activates:
  * fused trunks (C = 128, 256: k_block): the stored fp16 x (kernels.hip top comment: "bn0 + mish is applied to the
    fp16 value that is stored"), so block k depends on x16 alone.
  * layer-wise trunks (C = 384 / C_b = 192, C = 192 classic: k_lconv): the last conv of a block followed by another
    residual block is DUAL: it stores fp16(x + y) AND activates the unrounded fp32 sum for the next block's first conv
    (k_lconv: epilogue_store of the raw sum, then `activate()` on the same accumulators).  The emulation carries that
    fp32 sum (`xs`) to the next block in forward(); a block started from a stored x16 alone (teacher forcing) differs
    from the engine there by a rounding of the activated input, which the checker's thresholds absorb (the twin is
    measured the same way, tests/test_trunk_emulation_cpu.py).  After the stem or a broadcast block the first conv
    stages mish(bn0(.)) from the stored x16.

A known property of the engine's mish (conv_core.h mish_t2: t = log2(e) y, e = 2^t, t (ln2 - 2 ln2 / (e (e + 2) + 2))):
below about y = -4 the factor ln2 - 2 ln2 r cancels and loses relative accuracy (1e-5 at y = -4, 3e-4 at y = -8,
measured on the formulas in fp32 on the CPU), and below about y = -16.6 (e < 6e-8,
so e (e + 2) + 2 rounds to 2) it returns exactly 0 where mish(y) is about y e^y, -1e-6 at y = -16.6.  The absolute error
stays below 2e-6 (1.6e-6 measured; MISH_TAIL_ABS, checked by tests/test_trunk_emulation_cpu.py on the twin's formula); it is not a
defect.  The checker's absolute floor covers it.
"""
from __future__ import annotations

import os
import sys
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import torch_restatement as tr  # noqa: E402
import tfm_restatement  # noqa: E402

F64 = torch.float64
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
HEAD_CONVS = ("policy.conv_p.w", "policy.conv_g.w", "value.conv.w")
MISH_TAIL_ABS = 2e-6
HOT_MISH_IN = 40.0   # hot_weights: the largest mish input of every BN
HOT_X = 300.0        # hot_weights: the largest stem output
HEADS_TOL = 2e-4   # |raw| of the engine's heads against heads() on the engine's own x; the twin's worst is 1.5e-5


def is_layerwise(cfg) -> bool:
    """plan.cpp choose_plan: the trunks whose blocks run conv by conv through k_lconv."""
    return cfg.channels in (192, 384)


def inputs(pos):
    """(planes [N,19,19,15] float32, scalars [N,8] float32) of feature records, as k_init reads them."""
    n = len(pos)
    planes = np.zeros((n, 19, 19, 15), np.float32)
    sc = np.zeros((n, 8), np.float32)
    for k in range(n):
        f = pos[k]
        col = int(f["color"])
        for ch, key in ((0, "board"), (7, "stones_atari"), (9, "stones_two_liberties"),
                        (11, "stones_three_liberties"), (13, "stones_laddered")):
            g = np.asarray(f[key]).reshape(19, 19)
            planes[k, :, :, ch] = g == col
            planes[k, :, :, ch + 1] = g == -col
        for t in range(5):
            i, j = int(f["last_moves"][t]["i"]), int(f["last_moves"][t]["j"])
            if (i, j) == (19, 0):
                sc[k, 2 + t] = 1
            elif 0 <= i < 19 and 0 <= j < 19:
                planes[k, i, j, 2 + t] = 1
        sc[k, 0 if col == 1 else 1] = 1
        sc[k, 7] = np.float32(-1.0 if col == 1 else 1.0) * np.float32(f["komi"]) / np.float32(15.0)
    return planes, sc


def mish_engine(y, log2e_form=True):
    """The engine's fp32 mish of a float32 tensor y: mish_t2 (fused block kernel, on t = log2(e) y) or mish_f."""
    y = y.float()
    if log2e_form:
        t = y * np.float32(LOG2E)
        e = torch.exp2(t)
        r = 1.0 / (e * (e + 2.0) + 2.0)
        return t * (r * np.float32(-2.0 * LN2) + np.float32(LN2))
    s = torch.exp2(y * np.float32(LOG2E)) + 1.0
    r = 1.0 / (s * s + 1.0)
    return y - 2.0 * y * r


class Trunk:
    """The conv trunk of one network, block by block.  Tensors are float64 NCHW [N, C, 19, 19]; `mutate` injects the
    slips of tests/test_trunk_emulation_cpu.py (a dict with "kind" M1 .. M6 and where)."""

    def __init__(self, cfg, W: Dict[str, np.ndarray], fp16: bool = True, twin: bool = False,
                 mutate: Optional[dict] = None):
        self.cfg, self.W = cfg, W
        self.fp16 = fp16 or twin
        self.twin = twin
        self.mut = mutate or {}
        self.dt = torch.float32 if twin else F64
        self.layerwise = is_layerwise(cfg)
        self._w: Dict[str, torch.Tensor] = {}
        self._bn: Dict[str, tuple] = {}
        self.observe: Optional[Dict[str, float]] = None   # set to a dict: max |mish input| per BN, by act()

    # ---- storage and arithmetic -----------------------------------------------------------------------------------
    def r16(self, x):
        return x.half().to(x.dtype) if self.fp16 else x

    def weight(self, name):
        """OIHW conv weight (or [in, out] dense), fp16-rounded in the fp16 modes."""
        if name not in self._w:
            w = np.asarray(self.W[name], np.float32)
            if self.fp16:
                w = w.astype(np.float16).astype(np.float32)
            t = torch.from_numpy(w.astype(np.float64)).to(self.dt)
            if t.dim() == 4:
                t = t.permute(3, 2, 0, 1).contiguous()
            self._w[name] = t
        return self._w[name]

    def bn(self, prefix):
        if prefix not in self._bn:
            g, b, m, v = (np.asarray(self.W[f"{prefix}.{f}"]) for f in ("gamma", "beta", "mean", "var"))
            if self.twin:   # plan.cpp fold_bn, in fp32
                g, b, m, v = (a.astype(np.float32) for a in (g, b, m, v))
                sc = (g / np.sqrt(v + np.float32(tr.BN_EPS))).astype(np.float32)
                sh = (b - m * sc).astype(np.float32)
            else:
                g, b, m, v = (a.astype(np.float64) for a in (g, b, m, v))
                sc = g / np.sqrt(v + tr.BN_EPS)
                sh = b - m * sc
            self._bn[prefix] = (torch.from_numpy(sc).to(self.dt)[None, :, None, None],
                                torch.from_numpy(sh).to(self.dt)[None, :, None, None])
        return self._bn[prefix]

    def mish(self, y):
        if self.twin:
            return mish_engine(y, not self.layerwise)
        return tr._mish(y)

    def act(self, y, blk, idx):
        """mish(bn(y)) of conv idx's input in block blk, stored in fp16."""
        sc, sh = self.bn(f"blocks.{blk}.bn{idx}")
        z = y * sc + sh
        if self.observe is not None:
            p = f"blocks.{blk}.bn{idx}"
            self.observe[p] = max(self.observe.get(p, 0.0), float(z.abs().max()))
        if self.mut.get("kind") == "M3" and self.mut["block"] == blk:
            z = z.half().to(z.dtype)               # M3: the BN output rounded to fp16 before mish
        return self.r16(self.mish(z))

    def conv(self, a, blk, idx):
        name = f"blocks.{blk}.conv{idx}.w"
        w = self.weight(name)
        k = w.shape[-1]
        m = self.mut
        if m.get("kind") == "M1" and m["block"] == blk and m["conv"] == idx:
            w = w.clone()
            w[m["channel"]] = w[m["channel"]].flip(-1)   # M1: one output channel's kernel mirrored left-right
        if m.get("kind") == "M2" and m["block"] == blk and m["conv"] == idx and k == 3:
            # M2: the act buffer is a column-padded grid with row stride 20; a non-zero pad slot makes column 0's
            # left tap read the previous row's last point and column 18's right tap the next row's first point
            p = F.pad(a, (1, 1, 1, 1))
            p[:, :, 2:20, 0] = a[:, :, 0:18, 18]
            p[:, :, 1:19, 20] = a[:, :, 1:19, 0]
            return F.conv2d(p, w)
        return F.conv2d(a, w, padding=k // 2)

    # ---- entry points ---------------------------------------------------------------------------------------------
    def stem(self, features=None, planes=None, scalars=None):
        """x0 = fp16(init_conv(planes) + init_game(scalars)): k_init.  Give feature records or (planes, scalars)."""
        if features is not None:
            planes, scalars = inputs(features)
        if self.mut.get("kind") == "M6":   # M6: one slot of the batch evaluated with its neighbour's features
            s = self.mut["slot"]
            planes, scalars = planes.copy(), scalars.copy()
            planes[s], scalars[s] = planes[s + 1], scalars[s + 1]
        x = torch.from_numpy(np.asarray(planes, np.float64)).to(self.dt).permute(0, 3, 1, 2)
        gw = torch.from_numpy(np.asarray(self.W["init_game.w"], np.float64)).to(self.dt)
        gb = torch.from_numpy(np.asarray(self.W["init_game.b"], np.float64)).to(self.dt)
        gs = torch.from_numpy(np.asarray(scalars, np.float64)).to(self.dt) @ gw + gb
        x = F.conv2d(x, self.weight("init_conv.w"), padding=2) + gs[:, :, None, None]
        return self.r16(x).to(F64)

    def block(self, k, x_in, xa=None):
        """x after block k from x (float64, the stored value); xa: the unrounded sum the engine activates instead
        (layer-wise DUAL), None = x.  Returns x_out."""
        return self.block_xs(k, x_in, xa)[0]

    def block_xs(self, k, x_in, xa=None):
        """(x_out, xs): xs is the unrounded block output the next layer-wise block activates."""
        cfg = self.cfg
        x = x_in.to(self.dt)
        xa = x if xa is None else xa.to(self.dt)
        kind = cfg.block_kind(k)
        N, C = x.shape[0], cfg.channels
        if kind == "broadcast":
            t = self.r16(self.mish(self.conv(self.act(x, k, 0), k, 0))).reshape(N, C, 361)
            d = t @ self.weight(f"blocks.{k}.dense.w")
            if self.mut.get("kind") == "M5" and self.mut["block"] == k:
                # M5: the dense normalised over the 384 padded rows of the act buffer instead of the 361 board points.
                # The broadcast block has no global pool (BroadcastResidualBlock: conv_first, Dense over the 361
                # points, conv_last), so this "mean over padded rows" slip is applied to the dense, the one reduction
                # over the board the block has.
                d = d * (361.0 / 384.0)
            d = d + torch.from_numpy(np.asarray(self.W[f"blocks.{k}.dense.b"], np.float64)).to(self.dt)
            u = self.act(d.reshape(N, C, 19, 19), k, 1)
            xs = x + self.branch(self.conv(u, k, 1), k)
        elif kind == "btl":
            a = self.act(xa, k, 0)
            for j in range(cfg.inner_layers + 1):
                a = self.act(self.conv(a, k, j), k, j + 1)
            xs = x + self.branch(self.conv(a, k, cfg.inner_layers + 1), k)
        elif kind == "nbt":
            ts = self.conv(self.act(xa, k, 0), k, 0)   # raw t stored in fp16, activated from the fp32 accumulator
            t = self.r16(ts)
            for r in range(2):
                u = self.conv(self.act(ts, k, 1 + 2 * r), k, 1 + 2 * r)
                ts = t + self.conv(self.act(u, k, 2 + 2 * r), k, 2 + 2 * r)
                t = self.r16(ts)
            xs = x + self.branch(self.conv(self.act(ts, k, 5), k, 5), k)
        else:   # classic
            xs = x + self.branch(self.conv(self.act(self.conv(self.act(xa, k, 0), k, 0), k, 1), k, 1), k)
        return self.r16(xs).to(F64), xs.to(F64)

    def branch(self, y, k):
        if self.mut.get("kind") == "M4" and self.mut["block"] == k:
            return y.half().to(y.dtype)            # M4: the residual branch rounded to fp16 before the add
        return y

    def heads(self, x):
        """raw [N, 1889] (float64; the twin in float32) of the stored trunk output x (float64 NCHW)."""
        W = self.W
        if self.fp16:
            W = {k: (v.astype(np.float16).astype(np.float32) if k in HEAD_CONVS else v) for k, v in W.items()}
        dt = torch.float32 if self.twin else F64
        return tfm_restatement._heads(x.to(dt), W, x, dt)["raw"]

    def next_xa(self, k, x, xs):
        """What block k + 1 activates after block k: the unrounded sum where a layer-wise block feeds another one."""
        cfg = self.cfg
        if self.layerwise and cfg.block_kind(k) != "broadcast" and k + 1 < cfg.blocks and \
                cfg.block_kind(k + 1) != "broadcast":
            return xs
        return x

    def trunk(self, features=None, planes=None, scalars=None):
        """[x0, x1, ..., x_blocks]: the stored x after the stem and after every block, chained."""
        xs_list = [self.stem(features, planes, scalars)]
        x = xa = xs_list[0]
        for k in range(self.cfg.blocks):
            x_new, xs = self.block_xs(k, x, xa)
            xa = self.next_xa(k, x_new, xs)
            x = x_new
            xs_list.append(x)
        return xs_list

    def forward(self, features=None, planes=None, scalars=None):
        return self.heads(self.trunk(features, planes, scalars)[-1])


def hot_weights(cfg, W, pos, target=HOT_MISH_IN):
    """W with the BN gammas and betas of the blocks scaled, one BN at a time in trunk order, so that the largest mish
    input of that BN over the positions `pos` is `target` in the float64 emulation, and the stem scaled so that its
    largest output is HOT_X: activations of every layer span about +-target (mish's asymptotic branches) and the
    residual stream is in the hundreds (fp16 ulps of 0.125 - 0.5).  A uniform gain compounds from layer to layer and
    overflows fp16 within a block."""
    W = dict(W)
    planes, sc = inputs(pos)
    x0 = Trunk(cfg, W, fp16=False).stem(planes=planes, scalars=sc)
    s0 = np.float32(HOT_X / float(x0.abs().max()))
    for n in ("init_conv.w", "init_game.w", "init_game.b"):
        W[n] = (np.asarray(W[n], np.float32) * s0).astype(np.float32)
    probe = Trunk(cfg, W, fp16=False)
    probe.observe = {}
    probe.trunk(planes=planes, scalars=sc)
    order = list(probe.observe)        # insertion order = the order the trunk applies them
    for p in order:
        probe = Trunk(cfg, W, fp16=False)
        probe.observe = {}
        probe.trunk(planes=planes, scalars=sc)
        s = np.float32(target / probe.observe[p])
        for f in ("gamma", "beta"):
            W[f"{p}.{f}"] = (np.asarray(W[f"{p}.{f}"], np.float32) * s).astype(np.float32)
    return W


# ---- the checker -------------------------------------------------------------------------------------------------

def fp16_ulp(v):
    """ulp of the fp16 value nearest |v| (2^-24 in the subnormal range)."""
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def _regions():
    """board point -> 0 corner, 1 edge row or column, 2 interior (row-major 19 x 19)."""
    r, c = np.divmod(np.arange(361), 19)
    edge_r, edge_c = (r == 0) | (r == 18), (c == 0) | (c == 18)
    return np.where(edge_r & edge_c, 0, np.where(edge_r | edge_c, 1, 2))


REGION = _regions()
REGION_NAMES = ("corner", "edge", "interior")

# Thresholds of check_block.  err = |engine - emulation| / (ulp16(emulation) + FLOOR_REL * scale), scale = the larger
# RMS of the block's input x and of its branch (output - input): the absolute floor for residual sums that cancel (an
# emulated value near 0 has a tiny ulp while both sides carry rounding noise at the scale of the terms summed) and for
# mish's tail.  Set so that the twin passes every conv fixture and block by a margin; noted at each: the twin's worst
# over the 17 fixtures (test_twin_passes_the_block_checker) and over the batches of test_trunk_blocks_gpu.py
# (test_twin_on_the_gpu_test_batches), then what one MI355X measured.
FLOOR_REL = 2 ** -11           # half an fp16 ulp of the scale
# kind: (max err, lowest fraction bit-identical).  A layer-wise block started from the stored x16 activates a value
# the engine took from the fp32 sum (module docstring), which alone leaves up to half its outputs an ulp apart; the
# fused kernels see the same x16 as the emulation.
BOUNDS = {                         # twin worst err / identical, then MI355X (C = 128 .. 384, batches 1 - 300)
    "stem": (2.0, 0.99),           # twin 0.89 / 0.9997; GPU 0.80 / 1.000
    "btl": (2.5, 0.78),            # fused; twin 1.14 / 0.828; GPU 1.10 / 0.841
    "nbt": (6.0, 0.62),            # fused; twin 3.84 (test_b3c256nbt, GPU batch) / 0.710; GPU 2.92 / 0.752
    "broadcast": (4.5, 0.82),      # twin 2.32 / 0.879; GPU 1.55 / 0.894
    "lw_btl": (3.0, 0.62),         # layer-wise; twin 1.61 / 0.687; GPU 1.32 / 0.702
    "lw_nbt": (15.0, 0.45),        # layer-wise; twin 7.53 (test_b3c384nbt, GPU batch) / 0.510; GPU 6.14 / 0.509
    "classic": (6.5, 0.55),        # layer-wise; twin 3.22 / 0.624; GPU 3.12 / 0.626
    "hot": (2.0, 0.80),            # hot_weights nets, every block; twin 0.90 / 0.868; GPU 0.90 / 0.868
}


def kind_of(cfg, k):
    """The BOUNDS key of block k of cfg."""
    kind = cfg.block_kind(k)
    if kind in ("btl", "nbt") and is_layerwise(cfg):
        return "lw_" + kind
    return kind


def bounds(cfg, k, hot=False):
    """(max_err, min_identical) of block k of cfg ("stem" for the stem); hot: a net of hot_weights."""
    if k == "stem":
        return BOUNDS["stem"]
    return BOUNDS["hot"] if hot else BOUNDS[kind_of(cfg, k)]


def check_block(engine_x, emu_x, scale, block="?", slots=None, max_err=16.0, min_identical=0.0, head_width=None):
    """Compare the engine's x after one block ([n, C, 361] or [n, C, 19, 19]) with the emulation's from the same input.
    Returns the statistics; on failure raises AssertionError naming the worst (block, slot, channel group, point).
    head_width (tests/tfm_emulation.py): the channels are attention heads of that width, and the head is named too."""
    e = np.asarray(engine_x, np.float64).reshape(len(engine_x), -1, 361)
    m = np.asarray(emu_x, np.float64).reshape(e.shape)
    slots = list(range(len(e))) if slots is None else [int(s) for s in slots]
    d = np.abs(e - m)
    err = d / (fp16_ulp(m) + FLOOR_REL * float(scale))
    err = np.where(np.isfinite(e), err, np.inf)
    st = {
        "identical": float((e == m).mean()),
        "max_err": float(err.max()),
        "region": {REGION_NAMES[r]: float(err[:, :, REGION == r].max()) for r in range(3)},
        "group": err.reshape(len(e), -1, 8, 361).max(axis=(0, 2, 3)),
        "slot": err.max(axis=(1, 2)),
        "max_abs": float(d.max()),
    }
    if st["max_err"] > max_err or st["identical"] < min_identical:
        n, c, p = np.unravel_index(int(np.argmax(err)), err.shape)
        bad_g = [int(g) for g in np.nonzero(st["group"] > max_err)[0]]
        bad_s = [slots[int(s)] for s in np.nonzero(st["slot"] > max_err)[0]]
        bad_r = [k for k, v in st["region"].items() if v > max_err]
        heads = "" if head_width is None else (
            f"head {c // head_width} lane {c % head_width}, heads over the bound "
            f"{[int(h) for h in np.nonzero(err.reshape(len(e), -1, head_width, 361).max(axis=(0, 2, 3)) > max_err)[0]]}, "
            + (lambda t: f"tokens over the bound {t.min()}..{t.max()}, " if len(t) else "")(np.nonzero(err.max(axis=(0, 1)) > max_err)[0]))
        raise AssertionError(
            f"block {block}: max err {st['max_err']:.3g} (bound {max_err}) identical {st['identical']:.4f} "
            f"(bound {min_identical}); worst at slot {slots[n]} channel {c} (group {c // 8}) {heads}point {p} "
            f"(row {p // 19} col {p % 19}, {REGION_NAMES[REGION[p]]}): engine {e[n, c, p]!r} emulation {m[n, c, p]!r}; "
            f"over the bound: regions {bad_r} groups {bad_g[:12]}{'...' if len(bad_g) > 12 else ''} "
            f"slots {bad_s[:12]}{'...' if len(bad_s) > 12 else ''}")
    return st


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)))))


def block_scale(x_in, emu_out):
    """The floor's scale of one block: the larger RMS of its input and of its branch."""
    x_in, emu_out = np.asarray(x_in, np.float64), np.asarray(emu_out, np.float64)
    return max(rms(x_in), rms(emu_out - x_in.reshape(emu_out.shape)))


def teacher_forced(trunk: Trunk, xs_engine, features=None, planes=None, scalars=None, slots=None, label="", hot=False):
    """Check the stem and every block of `trunk` from the engine's own x before it: xs_engine = [x0, ..., x_B] (each
    n x C x 361 or n x C x 19 x 19; slots: the batch slots they are).  Returns {"stem" or block: stats}."""
    C = trunk.cfg.channels
    xs = [torch.from_numpy(np.asarray(x, np.float64).reshape(len(x), C, 19, 19)) for x in xs_engine]
    x0 = trunk.stem(features, planes, scalars)
    out = {"stem": check_block(xs[0], x0, rms(x0), f"{label}stem", slots, *bounds(trunk.cfg, "stem"))}
    for k in range(len(xs) - 1):
        m = trunk.block(k, xs[k])
        out[k] = check_block(xs[k + 1], m, block_scale(xs[k], m), f"{label}{k} ({trunk.cfg.block_kind(k)})", slots,
                             *bounds(trunk.cfg, k, hot))
    return out
