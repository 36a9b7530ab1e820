"""CPU emulation of the fused INT8 blocks (P3HIP_FLAG_INT8_FUSED and P3HIP_FLAG_INT8_C128, DESIGN.md section 9 "Fused
INT8 blocks").

TEST INFRASTRUCTURE ONLY: used by tests/test_int8_block_cpu.py and tests/test_int8_block_gpu.py, and at C = 128 through
tests/int8_block_c128.py.  The quantizer, the conv of one quantized layer (`_Q`), the error measures and the calibration
set come from tests/int8_restatement.py.

The emulation takes the width from `cfg`; the served set is a parameter, `widths`: a (C, C_b) pair.  This module's own
is that of P3HIP_FLAG_INT8_FUSED, with its fixtures (SERVED) and bounds (BOUNDS); tests/int8_block_c128.py holds those of
P3HIP_FLAG_INT8_C128.

The scheme of section 9 on the C = 256 / C_b = 128 and C = 128 / C_b = 64 btl trunks, where a block depends on the
stored fp16 x alone:
  a0 = q(mish(bn0(x16)));  conv j: exact integer accumulation, y = (float) acc * float32(s_a * s_w[c]);
  reduce and inner convs hand q(mish(bn_{j+1}(y))) on;  the expand conv gives x <- fp16((float) x16 + y).
The init conv, the broadcast blocks (t and u stored in fp16), the heads and x are the fp16 engine's.  Calibration
(scales None) is the fp16 plan: every activated tensor stored in fp16, its max |v| observed.
"""
from __future__ import annotations

import os
import sys
from typing import Dict, List, Optional

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import int8_restatement as ir  # noqa: E402
from int8_restatement import _Q, calibration_batches, errors, quantize  # noqa: E402,F401
from oracle import torch_restatement as tr  # noqa: E402
import tfm_restatement  # noqa: E402

DT = torch.float64

WIDTHS = (256, 128)   # (C, C_b) of the trunks P3HIP_FLAG_INT8_FUSED serves

# the trunks P3HIP_FLAG_INT8_FUSED serves among the fixtures
SERVED = ("test_b3c256btl1", "test_b5c256btl2_i2", "test_b10c256btl1_i2", "b12c256btl3")

# Bounds of the GPU tests against the float64 goldens (max |d| of move logits, move probabilities, value
# probabilities): three times the emulation's own error on the same fixture with its MinMax scales from
# calibration_batches(), rounded up (section 9's rule: where the quantizer rounds is fragile and the flips cascade).
# The emulation's errors these come from: test_b3c256btl1 0.022 / 5.5e-5 / 1.2e-3, test_b5c256btl2_i2
# 0.016 / 3.6e-5 / 8.1e-4, test_b10c256btl1_i2 0.047 / 2.3e-4 / 1.9e-3, b12c256btl3 0.047 / 2.3e-4 / 4.0e-3;
# tests/test_int8_block_cpu.py checks that the emulation stays within half of each.
BOUNDS = {
    "test_b3c256btl1": {"logit": 0.07, "prob": 1.7e-4, "value_prob": 3.6e-3},
    "test_b5c256btl2_i2": {"logit": 0.05, "prob": 1.1e-4, "value_prob": 2.5e-3},
    "test_b10c256btl1_i2": {"logit": 0.15, "prob": 7e-4, "value_prob": 6e-3},
    "b12c256btl3": {"logit": 0.15, "prob": 7e-4, "value_prob": 1.2e-2},
}


def is_served(cfg, widths=WIDTHS) -> bool:
    return (cfg.channels, cfg.bottleneck_channels) == widths and cfg.block_type == "btl" and 1 <= cfg.inner_layers <= 3


def quantized_tensors(cfg, widths=WIDTHS) -> List[str]:
    """Names of the quantized tensors in the engine's order: block by block, conv by conv (the input of conv j)."""
    if not is_served(cfg, widths):
        return []
    return [f"blocks.{i}.conv{j}.in" for i in range(cfg.blocks) if cfg.block_kind(i) != "broadcast"
            for j in range(cfg.inner_layers + 2)]


def block_scales(cfg, scales, k):
    """The (inner layers + 2) scales of btl block k out of the engine's array."""
    n = cfg.inner_layers + 2
    at = n * sum(cfg.block_kind(i) != "broadcast" for i in range(k))
    return np.asarray(scales, np.float32)[at:at + n]


def fp16_weights(cfg, W):
    """W with the tensors the fp16 engine rounds to fp16: init conv, head convs, the broadcast blocks' convs and dense."""
    return {k: (v.astype(np.float16).astype(np.float32) if (k in ir.FP16_WEIGHTS or
            (k.startswith("blocks.") and k.endswith(".w") and (".dense." in k or "conv" in k and
             cfg.block_kind(int(k.split(".")[1])) == "broadcast"))) else v) for k, v in W.items()}


def btl_block(cfg, k, x, Q):
    """x after btl block k from the stored x (float64 NCHW) with the convs of Q (int8 with its scales, or fp16)."""
    a = Q.act(x, k, 0)
    for j in range(cfg.inner_layers + 1):
        a = Q.act(Q.conv(a, k, j), k, j + 1)
    return ir._r16(x + Q.conv(a, k, cfg.inner_layers + 1))


def block(cfg, W, k, x_in, scales_k=None):
    """Teacher-forced: btl block k alone from x_in ([n, C, 361] or [n, C, 19, 19]); scales_k: its
    (inner layers + 2) activation scales, or None for the unquantized fp16 block (activated tensors stored in fp16,
    fp16 weights).  Returns [n, C, 19, 19] float64."""
    x = torch.from_numpy(np.asarray(x_in, np.float64).reshape(len(x_in), cfg.channels, 19, 19))
    return btl_block(cfg, k, x, _Q(W, scales_k, None)).numpy()


def forward(cfg, W: Dict[str, np.ndarray], planes_nhwc, feats, scales=None, observe: Optional[list] = None,
            widths=WIDTHS):
    """The fused INT8 engine's forward pass with `scales`, or (scales None) the fp16 plan it calibrates on with
    `observe` collecting the calibration maxima.  Outputs as oracle/torch_restatement.forward."""
    assert is_served(cfg, widths), cfg.name
    W = fp16_weights(cfg, W)
    if scales is not None:
        assert len(scales) == len(quantized_tensors(cfg, widths))
    Q = _Q(W, scales, observe)
    x = tr._t(planes_nhwc, DT).permute(0, 3, 1, 2)
    gs = tr._dense(tr._t(feats, DT), W, "init_game", DT)
    x = ir._r16(tr._conv(x, tr._t(W["init_conv.w"], DT)) + gs[:, :, None, None])
    N = x.shape[0]
    for i in range(cfg.blocks):
        if cfg.block_kind(i) == "broadcast":   # the fp16 engine: t and u stored in fp16
            t = ir._r16(tr._mish(tr._preact(x, W, i, 0, DT))).reshape(N, cfg.channels, 361)
            t = t @ tr._t(W[f"blocks.{i}.dense.w"], DT) + tr._t(W[f"blocks.{i}.dense.b"], DT)
            u = ir._r16(tr._mish(tr._bn(t.reshape(N, cfg.channels, 19, 19), W, f"blocks.{i}.bn1", DT)))
            x = ir._r16(x + tr._conv(u, tr._t(W[f"blocks.{i}.conv1.w"], DT)))
        else:
            x = btl_block(cfg, i, x, Q)
    return tfm_restatement._heads(x, W, x.permute(0, 2, 3, 1), DT)


def minmax_scales(cfg, W, batches, widths=WIDTHS) -> np.ndarray:
    """MinMax calibration over `batches` of (planes, scalars): s_a = max over all batches / 127, engine order."""
    amax = None
    for planes, sc in batches:
        obs: list = []
        forward(cfg, W, planes, sc, scales=None, observe=obs, widths=widths)
        a = np.asarray(obs, np.float32)
        amax = a if amax is None else np.maximum(amax, a)
    return (amax / np.float32(127)).astype(np.float32)
