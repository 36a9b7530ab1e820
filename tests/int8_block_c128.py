"""CPU emulation of the fused INT8 blocks at C = 128 / C_b = 64 (P3HIP_FLAG_INT8_C128, DESIGN.md section 9 "Fused INT8
blocks at C = 128").

TEST INFRASTRUCTURE ONLY: used by tests/test_int8_c128_cpu.py and tests/test_int8_c128_gpu.py.  The scheme is that of
tests/int8_block_restatement.py unchanged (a block depends on the stored fp16 x alone); `btl_block`, `_Q`,
`fp16_weights`, `block_scales`, `errors` and `calibration_batches` come from there.  What differs is the served set, and
with it `is_served`, `quantized_tensors`, `forward`, `minmax_scales` and the bounds.
"""
from __future__ import annotations

import os
import sys
from typing import Dict, List, Optional

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import int8_restatement as ir  # noqa: E402
from int8_block_restatement import _Q, block_scales, btl_block, calibration_batches, errors, fp16_weights  # noqa: E402,F401
from oracle import torch_restatement as tr  # noqa: E402
import tfm_restatement  # noqa: E402

DT = torch.float64

# the trunks P3HIP_FLAG_INT8_C128 serves among the fixtures with a float64 golden
SERVED = ("test_b3c128btl2", "test_b5c128btl1_i2", "b12c128btl3")

# Bounds of the GPU tests against the float64 goldens (max |d| of move logits, move probabilities, value
# probabilities): three times the emulation's own error on the same fixture with its MinMax scales from
# calibration_batches(), rounded up, the larger of two measurements (the rule of int8_restatement.BOUNDS: where the
# quantizer rounds is fragile and the flips cascade).  The two measurements: the scales as calibrated, and the same
# scales times 1 + 1e-6, which moves the rounding boundaries as a difference of fp16 storage would.  The emulation's
# errors these come from (calibrated | times 1 + 1e-6):
#   test_b3c128btl2     0.0122 / 3.5e-5 / 1.36e-3  |  0.0120 / 3.5e-5 / 1.36e-3
#   test_b5c128btl1_i2  0.0272 / 1.1e-4 / 2.94e-3  |  0.0278 / 8.7e-5 / 2.52e-3
#   b12c128btl3         0.0373 / 1.6e-4 / 8.6e-4   |  0.0351 / 2.2e-4 / 1.88e-3
# (fp16 storage alone: 5.0e-4, 1.0e-3 and 2.7e-3 in the logits.)  tests/test_int8_c128_cpu.py checks that the emulation
# stays within half of each.
BOUNDS = {
    "test_b3c128btl2": {"logit": 0.04, "prob": 1.1e-4, "value_prob": 4.1e-3},
    "test_b5c128btl1_i2": {"logit": 0.085, "prob": 3.4e-4, "value_prob": 9e-3},
    "b12c128btl3": {"logit": 0.12, "prob": 6.7e-4, "value_prob": 5.7e-3},
}


def is_served(cfg) -> bool:
    return cfg.channels == 128 and cfg.bottleneck_channels == 64 and cfg.block_type == "btl" and \
        1 <= cfg.inner_layers <= 3


def quantized_tensors(cfg) -> List[str]:
    """Names of the quantized tensors in the engine's order: block by block, conv by conv (the input of conv j)."""
    if not is_served(cfg):
        return []
    return [f"blocks.{i}.conv{j}.in" for i in range(cfg.blocks) if cfg.block_kind(i) != "broadcast"
            for j in range(cfg.inner_layers + 2)]


def block(cfg, W, k, x_in, scales_k=None):
    """Teacher-forced: btl block k alone from x_in ([n, 128, 361] or [n, 128, 19, 19]); scales_k: its
    (inner layers + 2) activation scales, or None for the unquantized fp16 block (activated tensors stored in fp16,
    fp16 weights).  Returns [n, 128, 19, 19] float64."""
    x = torch.from_numpy(np.asarray(x_in, np.float64).reshape(len(x_in), cfg.channels, 19, 19))
    return btl_block(cfg, k, x, _Q(W, scales_k, None)).numpy()


def forward(cfg, W: Dict[str, np.ndarray], planes_nhwc, feats, scales=None, observe: Optional[list] = None):
    """The INT8_C128 engine's forward pass with `scales`, or (scales None) the fp16 plan it calibrates on with
    `observe` collecting the calibration maxima.  Outputs as oracle/torch_restatement.forward."""
    assert is_served(cfg), cfg.name
    W = fp16_weights(cfg, W)
    if scales is not None:
        assert len(scales) == len(quantized_tensors(cfg))
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


def minmax_scales(cfg, W, batches) -> np.ndarray:
    """MinMax calibration over `batches` of (planes, scalars): s_a = max over all batches / 127, engine order."""
    amax = None
    for planes, sc in batches:
        obs: list = []
        forward(cfg, W, planes, sc, scales=None, observe=obs)
        a = np.asarray(obs, np.float32)
        amax = a if amax is None else np.maximum(amax, a)
    return (amax / np.float32(127)).astype(np.float32)
