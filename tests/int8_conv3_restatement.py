"""CPU emulation of calibrated INT8 for the 3x3 convs only (P3HIP_FLAG_INT8_CONV3, DESIGN.md section 9 "INT8 for the 3x3
convs only").

TEST INFRASTRUCTURE ONLY: used by tests/test_int8_conv3_cpu.py and tests/test_int8_conv3_gpu.py.  The forward pass and the
blocks are those of tests/int8_any_restatement.py with another conv: `_Q3` runs a 3x3 conv on int8 (int8_restatement._Q:
the activated input quantized from its unrounded value, per-channel weight scales, exact integer sums) and a 1x1 conv as
the fp16 plan does (the activated input stored in fp16, fp16 weights).  So the rounding points are the fp16 plan's own
everywhere, and int8 codes stand exactly where a 3x3 conv reads:

  * the fp16 1x1 reduce hands q(mish(bn(y))) to the first 3x3, quantized from its fp32 y (no fp16 value in between);
  * a 3x3 conv hands q(mish(bn(y))) to the next 3x3, as the INT8 plans do;
  * the last 3x3 hands (fp16) mish(bn(y)) to the fp16 1x1 expand; the raw streams (x, the nbt block's t) are fp16.

A classic trunk has only 3x3 convs: the flag's plan is P3HIP_FLAG_INT8's / _INT8_ANY's, and this emulation is theirs, bit
for bit (every conv is quantized).
"""
from __future__ import annotations

import os
import sys
from typing import Dict, List, Optional

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import int8_any_restatement as ar  # noqa: E402
from int8_any_restatement import config, feeds_layerwise, handed_on, weights  # noqa: E402,F401
from int8_restatement import _Q, _r16, calibration_batches, errors, quantize  # noqa: E402,F401
from int8_block_restatement import fp16_weights  # noqa: E402
from oracle import torch_restatement as tr  # noqa: E402
import tfm_restatement  # noqa: E402
import trunk_emulation as te  # noqa: E402

DT = torch.float64

# the nets of tests/test_int8_conv3_gpu.py, and what each exercises
NETS = ("test_b3c384btl3",      # templated, three passes of reduce
        "test_b3c384nbt",       # dual + res at both ends of the pairs
        "test_b3c192btl3",      # runtime width, C_b 96 padded to 128
        "test_b3c96nbt",        # both widths padded
        "test_b3c64btl2")       # one K slice, one output pass: no prefetch
CLASSIC = ("test_b3c192classic", "test_b3c128classic")   # equality with the existing INT8 plans

# The emulation's own error against the float64 outputs (conv_widths_common.outputs(..., fp16=False) on
# conv_widths_common.positions()) with its MinMax scales from calibration_batches(): max |d| of move logits, move
# probabilities, value probabilities.  Measured on the CPU (python tests/int8_conv3_restatement.py): first with the MinMax
# scales, second with every scale raised by one fp16 ulp (x (1 + 2^-10)), as int8_any_restatement.MEASURED.
MEASURED = {
    "test_b3c384btl3": ((1.24e-2, 3.34e-5, 7.79e-4), (1.30e-2, 4.41e-5, 9.65e-4)),
    "test_b3c384nbt": ((1.97e-2, 7.66e-5, 2.71e-3), (2.43e-2, 7.08e-5, 3.06e-3)),
    "test_b3c192btl3": ((9.76e-3, 2.78e-5, 1.81e-3), (1.15e-2, 3.11e-5, 1.52e-3)),
    "test_b3c96nbt": ((2.14e-2, 8.12e-5, 1.98e-3), (2.17e-2, 7.32e-5, 2.61e-3)),
    "test_b3c64btl2": ((5.13e-3, 1.59e-5, 6.73e-4), (5.16e-3, 1.40e-5, 9.54e-4)),
}
# The INT8 / INT8_ANY emulation (every conv of the block quantized) on the same nets, positions and calibration, MinMax
# scales: the move-logit error of this scheme is below it on every net
INT8_ALL_CONVS = {
    "test_b3c384btl3": (1.47e-2, 4.48e-5, 1.88e-3),
    "test_b3c384nbt": (4.03e-2, 1.33e-4, 7.41e-3),
    "test_b3c192btl3": (1.50e-2, 4.04e-5, 1.67e-3),
    "test_b3c96nbt": (3.87e-2, 1.30e-4, 4.60e-3),
    "test_b3c64btl2": (9.32e-3, 2.36e-5, 1.39e-3),
}
# The project's rule for INT8 GPU tests (int8_restatement.BOUNDS): three times the larger measurement, rounded up;
# tests/test_int8_conv3_cpu.py checks the rule and that the emulation stays within half of each
BOUNDS = {
    "test_b3c384btl3": {"logit": 0.04, "prob": 1.4e-4, "value_prob": 3e-3},
    "test_b3c384nbt": {"logit": 0.075, "prob": 2.4e-4, "value_prob": 9.5e-3},
    "test_b3c192btl3": {"logit": 0.035, "prob": 1e-4, "value_prob": 5.5e-3},
    "test_b3c96nbt": {"logit": 0.07, "prob": 2.5e-4, "value_prob": 8e-3},
    "test_b3c64btl2": {"logit": 0.016, "prob": 5e-5, "value_prob": 3e-3},
}


def conv3_indices(cfg, kind) -> List[int]:
    """the 3x3 convs of a block, by conv index"""
    return {"btl": list(range(1, cfg.inner_layers + 1)), "nbt": [1, 2, 3, 4], "classic": [0, 1]}[kind]


def quantized_tensors(cfg) -> List[str]:
    """Names of the quantized tensors in the engine's order: the inputs of the 3x3 convs only."""
    return [f"blocks.{i}.conv{j}.in" for i in range(cfg.blocks) if cfg.block_kind(i) != "broadcast"
            for j in conv3_indices(cfg, cfg.block_kind(i))]


def block_scales(cfg, scales, k):
    """The scales of layer-wise block k out of the engine's array."""
    at = sum(len(conv3_indices(cfg, cfg.block_kind(i))) for i in range(k) if cfg.block_kind(i) != "broadcast")
    return np.asarray(scales, np.float32)[at:at + len(conv3_indices(cfg, cfg.block_kind(k)))]


class _Q3(_Q):
    """int8_restatement._Q with the 1x1 convs left to the fp16 plan; the scales (and the calibration's maxima) count the
    3x3 convs alone.  scales None and observe None: the unquantized fp16 block."""

    def conv(self, a, blk, idx):
        w = self.W[f"blocks.{blk}.conv{idx}.w"]
        if w.shape[0] == 3:
            return super().conv(a, blk, idx)
        a = _r16(a)   # the 1x1 conv reads the activated tensor from fp16 storage
        return tr._conv(a, tr._t(np.asarray(w, np.float16).astype(np.float32), DT))


def block(cfg, W, k, x_in, scales_k=None, xa=None):
    """Teacher-forced: layer-wise block k alone from the stored x_in ([n, C, 361] or [n, C, 19, 19]); xa: the unrounded
    sum of the block before it where that is layer-wise too (None: x_in; either way the block's first conv, a 1x1, reads it
    activated and rounded to fp16); scales_k: the block's 3x3 activation scales, or None for the unquantized fp16 block.
    Returns (x_out, xs) as [n, C, 19, 19] float64."""
    x = torch.from_numpy(np.asarray(x_in, np.float64).reshape(len(x_in), cfg.channels, 19, 19))
    a = x if xa is None else torch.from_numpy(np.asarray(xa, np.float64).reshape(x.shape))
    out, xs = ar.layerwise_block(cfg, k, x, a, _Q3(W, scales_k, None))
    return out.numpy(), xs.numpy()


def forward(cfg, W: Dict[str, np.ndarray], planes_nhwc, feats, scales=None, observe: Optional[list] = None):
    """The INT8_CONV3 engine's forward pass with `scales`, or (scales None) the fp16 plan it calibrates on with `observe`
    collecting the maxima of the 3x3 inputs.  Outputs as oracle/torch_restatement.forward."""
    assert cfg.block_type in ("btl", "nbt", "classic"), cfg.name
    W = fp16_weights(cfg, W)
    if scales is not None:
        assert len(scales) == len(quantized_tensors(cfg))
    Q = _Q3(W, scales, observe)
    x = tr._t(planes_nhwc, DT).permute(0, 3, 1, 2)
    gs = tr._dense(tr._t(feats, DT), W, "init_game", DT)
    x = _r16(tr._conv(x, tr._t(W["init_conv.w"], DT)) + gs[:, :, None, None])
    N = x.shape[0]
    xa = x
    for i in range(cfg.blocks):
        if cfg.block_kind(i) == "broadcast":   # the fp16 engine: t and u stored in fp16
            t = _r16(tr._mish(tr._preact(x, W, i, 0, DT))).reshape(N, cfg.channels, 361)
            t = t @ tr._t(W[f"blocks.{i}.dense.w"], DT) + tr._t(W[f"blocks.{i}.dense.b"], DT)
            u = _r16(tr._mish(tr._bn(t.reshape(N, cfg.channels, 19, 19), W, f"blocks.{i}.bn1", DT)))
            x = xa = _r16(x + tr._conv(u, tr._t(W[f"blocks.{i}.conv1.w"], DT)))
            continue
        x, xs = ar.layerwise_block(cfg, i, x, xa, Q)
        xa = xs if feeds_layerwise(cfg, i) else x
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


def emulation_errors(name, scales=None):
    """(errors, scales) of the emulation of `name` with its MinMax scales from calibration_batches() against the float64
    outputs of conv_widths_common.positions(): what BOUNDS is made from."""
    import conv_widths_common as cw
    cfg, W = config(name), weights(name)
    if scales is None:
        scales = minmax_scales(cfg, W, [te.inputs(c) for c in calibration_batches()])
    pos = cw.positions()
    ref = cw.outputs(cfg, W, pos, fp16=False)
    planes, sc = te.inputs(pos)
    return errors(forward(cfg, W, planes, sc, scales=scales), ref), scales


if __name__ == "__main__":   # the two measurements behind BOUNDS, and the INT8 / INT8_ANY emulation's beside them
    for n in (sys.argv[1:] or NETS):
        e1, s = emulation_errors(n)
        e2, _ = emulation_errors(n, (s * np.float32(1 + 2.0 ** -10)).astype(np.float32))
        e0, _ = ar.emulation_errors(n)
        print(n, *(tuple(float(f"{e[k]:.3g}") for k in ("logit", "prob", "value_prob")) for e in (e1, e2, e0)), flush=True)
