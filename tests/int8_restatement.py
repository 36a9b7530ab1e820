"""CPU emulation of the engine's calibrated INT8 forward pass (P3HIP_FLAG_INT8).

TEST INFRASTRUCTURE ONLY: used by tests/test_int8_cpu.py and tests/test_int8_gpu.py.  The layer helpers come from
oracle/torch_restatement.py; the quantization points are written here.

The convs of the layer-wise blocks (btl / nbt / classic at the widths the fused block kernel lacks) take int8 inputs:
the activated tensor mish(bn(.)) quantized per tensor with s_a, the weights per output channel with s_w[c], exact
integer accumulation, y = acc * float32(s_a * s_w[c]) in fp32.  Everything else is the fp16 engine: the raw residual
streams (x, and the nbt block's t) are stored in fp16, as are the init conv, broadcast blocks and head inputs.

`forward(..., scales)` runs the INT8 scheme with the given activation scales (the engine's order: block by block, conv
by conv); `forward(..., scales=None, observe=list)` runs the fp16 scheme the engine calibrates on and appends every
quantized tensor's max |v| to `observe`, so `minmax_scales` can give the MinMax scales of a set of positions.
"""
from __future__ import annotations

import os
import sys
from typing import Dict, List, Optional

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import torch_restatement as tr  # noqa: E402
import tfm_restatement  # noqa: E402

DT = torch.float64
FP16_WEIGHTS = ("init_conv.w", "policy.conv_p.w", "policy.conv_g.w", "value.conv.w")

# the layer-wise trunks (plan.cpp choose_plan: C = 384 / C_b = 192 btl or nbt, C = 192 classic)
LAYERWISE = ("test_b3c384btl3", "test_b3c384nbt", "test_b3c192classic", "b14c384btl3", "b10c384nbt", "b15c192_classic")


def is_layerwise(cfg) -> bool:
    return (cfg.channels == 384 and cfg.bottleneck_channels == 192 and cfg.block_type in ("btl", "nbt")) or \
        (cfg.channels == 192 and cfg.block_type == "classic")


def quantize(y, s):
    """q = clamp(rint(y / s), -127, 127) (round half to even, -128 unused); a zero scale gives 0."""
    y = np.asarray(y, np.float32)
    s = np.float32(s)
    if not s > 0:
        return np.zeros_like(y)
    return np.clip(np.rint(y / s), -127, 127).astype(np.float32)


def weight_scales(w_hwio):
    """Per output channel: s_w[c] = max_k |W[k, c]| / 127 (float32)."""
    w = np.asarray(w_hwio, np.float32).reshape(-1, w_hwio.shape[-1])
    return (np.abs(w).max(0) / np.float32(127)).astype(np.float32)


def quantize_weights(w_hwio):
    """(q, s_w): q = clamp(rint(W / s_w[c]), -127, 127), 0 where s_w = 0."""
    w = np.asarray(w_hwio, np.float32)
    sw = weight_scales(w)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(sw > 0, np.clip(np.rint(w / np.where(sw > 0, sw, 1)), -127, 127), 0).astype(np.float32)
    return q, sw


def quantized_tensors(cfg) -> List[str]:
    """Names of the quantized tensors in the engine's order: block by block, conv by conv (the input of conv j)."""
    if not is_layerwise(cfg):
        return []
    out = []
    for i in range(cfg.blocks):
        kind = cfg.block_kind(i)
        if kind == "broadcast":
            continue
        n = {"btl": cfg.inner_layers + 2, "nbt": 6, "classic": 2}[kind]
        out += [f"blocks.{i}.conv{j}.in" for j in range(n)]
    return out


def _r16(x):
    return x.half().to(DT)


class _Q:
    """The conv of one layer-wise layer, int8 (scales given) or fp16 (calibration: observe max |input|)."""

    def __init__(self, W, scales, observe):
        self.W, self.scales, self.observe, self.k = W, scales, observe, 0

    def act(self, y, blk, idx):
        return tr._mish(tr._bn(y, self.W, f"blocks.{blk}.bn{idx}", DT))

    def conv(self, a, blk, idx):
        """conv idx of block blk on its activated input a (float64 NCHW); returns the fp32 output y as float64."""
        w = self.W[f"blocks.{blk}.conv{idx}.w"]
        k = self.k
        self.k += 1
        if self.scales is None:
            a = _r16(a)   # the fp16 plan stores the activated tensor in fp16
            if self.observe is not None:
                self.observe.append(float(a.abs().max()))
            return tr._conv(a, tr._t(np.asarray(w, np.float16).astype(np.float32), DT))
        s = np.float32(self.scales[k])
        q = torch.from_numpy(quantize(a.numpy(), s)).to(DT)
        wq, sw = quantize_weights(w)
        acc = tr._conv(q, torch.from_numpy(wq).to(DT))                    # exact: integers below 2^53
        mult = (s * sw).astype(np.float32)                                 # s_a * s_w[c] in fp32
        y = acc.numpy().astype(np.float32) * mult[None, :, None, None]    # (float) acc * mult in fp32
        return torch.from_numpy(y.astype(np.float64))


def forward(cfg, W: Dict[str, np.ndarray], planes_nhwc, feats, scales=None, observe: Optional[list] = None):
    """The engine's forward pass: INT8 convs in the layer-wise blocks with `scales`, or (scales None) the fp16 plan
    with `observe` collecting the calibration maxima.  Outputs as oracle/torch_restatement.forward."""
    assert is_layerwise(cfg), cfg.name
    W = {k: (v.astype(np.float16).astype(np.float32) if (k in FP16_WEIGHTS or
             (k.startswith("blocks.") and k.endswith(".w") and (".dense." in k or "conv" in k and
              cfg.block_kind(int(k.split(".")[1])) == "broadcast"))) else v) for k, v in W.items()}
    if scales is not None:
        assert len(scales) == len(quantized_tensors(cfg))
    Q = _Q(W, scales, observe)
    x = tr._t(planes_nhwc, DT).permute(0, 3, 1, 2)
    gs = tr._dense(tr._t(feats, DT), W, "init_game", DT)
    x = _r16(tr._conv(x, tr._t(W["init_conv.w"], DT)) + gs[:, :, None, None])
    N = x.shape[0]
    # xa: what the next layer-wise block's first conv activates.  The last conv of a layer-wise block that feeds
    # another one activates its fp32 sum x + y before x is stored in fp16 (dual); after the init conv or a broadcast
    # block the first conv stages mish(bn0(.)) from the stored fp16 x (pre).
    xa = x
    for i in range(cfg.blocks):
        kind = cfg.block_kind(i)
        if kind == "broadcast":   # the fp16 engine: t and u stored in fp16
            t = _r16(tr._mish(tr._preact(x, W, i, 0, DT))).reshape(N, cfg.channels, 361)
            t = t @ tr._t(W[f"blocks.{i}.dense.w"], DT) + tr._t(W[f"blocks.{i}.dense.b"], DT)
            u = _r16(tr._mish(tr._bn(t.reshape(N, cfg.channels, 19, 19), W, f"blocks.{i}.bn1", DT)))
            x = xa = _r16(x + tr._conv(u, tr._t(W[f"blocks.{i}.conv1.w"], DT)))
            continue
        if kind == "btl":
            a = Q.act(xa, i, 0)
            for j in range(cfg.inner_layers + 1):
                a = Q.act(Q.conv(a, i, j), i, j + 1)
            xs = x + Q.conv(a, i, cfg.inner_layers + 1)
        elif kind == "nbt":
            ts = Q.conv(Q.act(xa, i, 0), i, 0)       # the raw t is stored in fp16, its activation taken from fp32
            t = _r16(ts)
            for r in range(2):
                u = Q.conv(Q.act(ts, i, 1 + 2 * r), i, 1 + 2 * r)
                ts = t + Q.conv(Q.act(u, i, 2 + 2 * r), i, 2 + 2 * r)
                t = _r16(ts)
            xs = x + Q.conv(Q.act(ts, i, 5), i, 5)
        else:   # classic
            xs = x + Q.conv(Q.act(Q.conv(Q.act(xa, i, 0), i, 0), i, 1), i, 1)
        x = _r16(xs)
        xa = xs if i + 1 < cfg.blocks and cfg.block_kind(i + 1) != "broadcast" else x
    return tfm_restatement._heads(x, W, x.permute(0, 2, 3, 1), DT)


# The calibration set of the tests: seeded random positions, separate from every evaluated set
CALIB_SEED, CALIB_BATCHES, CALIB_BATCH = 9001, 2, 16


# Bounds of the GPU tests on the INT8 engine against the float64 goldens (max |d| of move logits, move probabilities,
# value probabilities).  Each is three times the emulation's own error on the same fixture with its MinMax scales from
# calibration_batches(), rounded up (the larger of two measurements: where the quantizer rounds changes with
# differences as small as fp16 storage, and the flips cascade through the layers);
# tests/test_int8_cpu.py checks that the emulation stays within half of each.
BOUNDS = {
    "test_b3c384btl3": {"logit": 0.05, "prob": 1.8e-4, "value_prob": 4e-3},
    "test_b3c384nbt": {"logit": 0.13, "prob": 3.5e-4, "value_prob": 1.25e-2},
    "test_b3c192classic": {"logit": 0.075, "prob": 2.7e-4, "value_prob": 1.4e-3},
    "b14c384btl3": {"logit": 0.16, "prob": 6.5e-4, "value_prob": 2.2e-2},
    "b10c384nbt": {"logit": 0.5, "prob": 4e-3, "value_prob": 1e-2},
}


def calibration_batches():
    """[features records] of the calibration batches (features.random_positions, seeds CALIB_SEED + b)."""
    from p3achygo_amd import features
    return [features.random_positions(CALIB_BATCH, seed=CALIB_SEED + b) for b in range(CALIB_BATCHES)]


def errors(out, ref):
    """The three error measures the INT8 bounds are stated in: max |d| of the move logits, move probabilities and
    value probabilities, against reference outputs (the golden npz fields or oracle_torch's dict)."""
    return {"logit": float(np.abs(out["raw"][:, :362] - ref["raw"][:, :362]).max()),
            "prob": float(np.abs(out["move_probs"] - ref["move_probs"]).max()),
            "value_prob": float(np.abs(out["value_probs"] - ref["value_probs"]).max())}


def minmax_scales(cfg, W, batches) -> np.ndarray:
    """MinMax calibration over `batches` of (planes, scalars): s_a = max over all batches / 127, engine order."""
    amax = None
    for planes, sc in batches:
        obs: list = []
        forward(cfg, W, planes, sc, scales=None, observe=obs)
        a = np.asarray(obs, np.float32)
        amax = a if amax is None else np.maximum(amax, a)
    return (amax / np.float32(127)).astype(np.float32)
