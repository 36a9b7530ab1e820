"""CPU emulation of calibrated INT8 inference at any width (P3HIP_FLAG_INT8_ANY, DESIGN.md section 9 "INT8 at any width").

TEST INFRASTRUCTURE ONLY: used by tests/test_int8_any_cpu.py and tests/test_int8_any_gpu.py.  This is the forward pass of
tests/int8_restatement.py with its `is_layerwise` restriction lifted: any btl / nbt / classic config, the same
quantization points.  The quantizer, the conv of one quantized layer (`_Q`), the error measures and the calibration set
come from there, so there is one scheme.

The engine pads C and C_b to multiples of 64.  Padding needs no modelling: a padded channel is an exact 0 in every
tensor, fp16 or int8 (its BN folds to scale = shift = 0, its weights and their scale are 0), so it adds exact zeros to
every sum and cannot raise a maximum.

`block(...)` is one layer-wise block alone, teacher-forced from a stored x; `xa` is the unrounded fp32 sum the block before
it handed on (the engine's `dual` output is activated from it, not from the fp16 x).
"""
from __future__ import annotations

import os
import sys
from typing import Dict, List, Optional

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import int8_restatement as ir  # noqa: E402
from int8_restatement import _Q, _r16, calibration_batches, errors, quantize  # noqa: E402,F401
from int8_block_restatement import fp16_weights  # noqa: E402
from oracle import torch_restatement as tr  # noqa: E402
import tfm_restatement  # noqa: E402

DT = torch.float64

# the nets of tests/test_int8_any_gpu.py, and why each is there
NETS = ("test_b3c64btl2",       # one slice per conv (no prefetch), one output pass, C_b padded 32 -> 64
        "test_b3c96nbt",        # both widths padded; nbt dual / res flows
        "test_b3c128nbt",       # the reference's nbt shapes that had no INT8
        "test_b3c256nbt",
        "test_b3c192btl3",      # odd slice count 3 at the 1x1 reduce, C_b padded 96 -> 128
        "test_b3c128classic",   # 3x3 C -> C from the raw stream (pre)
        "test_b3c320nbt",       # five slices, C_b padded 160 -> 192
        "test_b4c512btl3_i2")   # the wide end, broadcast blocks between layer-wise blocks

# Bounds of the GPU tests on the INT8_ANY engine against the float64 outputs (conv_widths_common.outputs(..., fp16=False)
# on conv_widths_common.positions()): max |d| of move logits, move probabilities, value probabilities.  By the rule of
# int8_restatement.BOUNDS: three times the emulation's own error on the same positions with its MinMax scales from
# calibration_batches(), rounded up; the larger of two measurements (quantizer rounding flips cascade through the
# layers).  Measured on the CPU, (logit, prob, value_prob): first with the MinMax scales, second with every scale
# raised by one fp16 ulp (x (1 + 2^-10)), the difference the engine's fp16 calibration plan may show against the
# emulation's (the GPU test allows rtol 4e-3 there), which moves where the quantizer rounds:
MEASURED = {
    "test_b3c64btl2": ((9.32e-3, 2.36e-5, 1.39e-3), (7.72e-3, 2.52e-5, 1.42e-3)),
    "test_b3c96nbt": ((3.87e-2, 1.30e-4, 4.60e-3), (4.41e-2, 1.15e-4, 4.76e-3)),
    "test_b3c128nbt": ((5.63e-2, 1.66e-4, 3.94e-3), (5.02e-2, 1.54e-4, 3.89e-3)),
    "test_b3c256nbt": ((5.33e-2, 2.27e-4, 5.11e-3), (5.71e-2, 2.04e-4, 5.05e-3)),
    "test_b3c192btl3": ((1.50e-2, 4.04e-5, 1.67e-3), (1.49e-2, 5.27e-5, 1.88e-3)),
    "test_b3c128classic": ((2.61e-2, 7.25e-5, 4.38e-3), (3.61e-2, 7.50e-5, 2.86e-3)),
    "test_b3c320nbt": ((4.19e-2, 1.62e-4, 2.28e-3), (4.41e-2, 1.37e-4, 3.86e-3)),
    "test_b4c512btl3_i2": ((1.48e-2, 5.13e-5, 8.66e-4), (1.42e-2, 4.40e-5, 1.08e-3)),
}
# three times the larger, rounded up; tests/test_int8_any_cpu.py checks that the emulation stays within half of each
BOUNDS = {
    "test_b3c64btl2": {"logit": 0.03, "prob": 8e-5, "value_prob": 4.5e-3},
    "test_b3c96nbt": {"logit": 0.14, "prob": 4e-4, "value_prob": 1.5e-2},
    "test_b3c128nbt": {"logit": 0.17, "prob": 5e-4, "value_prob": 1.2e-2},
    "test_b3c256nbt": {"logit": 0.18, "prob": 7e-4, "value_prob": 1.6e-2},
    "test_b3c192btl3": {"logit": 0.045, "prob": 1.6e-4, "value_prob": 6e-3},
    "test_b3c128classic": {"logit": 0.11, "prob": 2.3e-4, "value_prob": 1.4e-2},
    "test_b3c320nbt": {"logit": 0.14, "prob": 5e-4, "value_prob": 1.2e-2},
    "test_b4c512btl3_i2": {"logit": 0.045, "prob": 1.6e-4, "value_prob": 3.5e-3},
}


def config(name):
    from p3achygo_amd import netspec
    return netspec.get_config(name)


def weights(name):
    from p3achygo_amd import netspec
    return netspec.generate_weights(config(name), randomize=True)


def n_convs(cfg, kind) -> int:
    return {"btl": cfg.inner_layers + 2, "nbt": 6, "classic": 2}[kind]


def quantized_tensors(cfg) -> List[str]:
    """Names of the quantized tensors in the engine's order: block by block, conv by conv (the input of conv j)."""
    out = []
    for i in range(cfg.blocks):
        kind = cfg.block_kind(i)
        if kind != "broadcast":
            out += [f"blocks.{i}.conv{j}.in" for j in range(n_convs(cfg, kind))]
    return out


def block_scales(cfg, scales, k):
    """The scales of layer-wise block k out of the engine's array."""
    at = sum(n_convs(cfg, cfg.block_kind(i)) for i in range(k) if cfg.block_kind(i) != "broadcast")
    return np.asarray(scales, np.float32)[at:at + n_convs(cfg, cfg.block_kind(k))]


def layerwise_block(cfg, i, x, xa, Q, a0=None):
    """(x_out, xs) of btl / nbt / classic block i from the stored x and what its first conv activates, xa; xs is the
    unrounded sum.  The quantization points of int8_restatement.forward.  a0: the first conv's activated input itself,
    in place of mish(bn0(xa)) (teacher-forced from the engine's own int8 tensor)."""
    kind = cfg.block_kind(i)
    a0 = Q.act(xa, i, 0) if a0 is None else a0
    if kind == "btl":
        a = a0
        for j in range(cfg.inner_layers + 1):
            a = Q.act(Q.conv(a, i, j), i, j + 1)
        xs = x + Q.conv(a, i, cfg.inner_layers + 1)
    elif kind == "nbt":
        ts = Q.conv(a0, i, 0)                    # the raw t is stored in fp16, its activation taken from fp32
        t = _r16(ts)
        for r in range(2):
            u = Q.conv(Q.act(ts, i, 1 + 2 * r), i, 1 + 2 * r)
            ts = t + Q.conv(Q.act(u, i, 2 + 2 * r), i, 2 + 2 * r)
            t = _r16(ts)
        xs = x + Q.conv(Q.act(ts, i, 5), i, 5)
    else:   # classic
        xs = x + Q.conv(Q.act(Q.conv(a0, i, 0), i, 1), i, 1)
    return _r16(xs), xs


def feeds_layerwise(cfg, i) -> bool:
    """block i hands its unrounded sum to block i + 1 (both layer-wise: the engine's dual output)"""
    return cfg.block_kind(i) != "broadcast" and i + 1 < cfg.blocks and cfg.block_kind(i + 1) != "broadcast"


def handed_on(xs_emulated, x_stored):
    """Teacher-forced estimate of the unrounded sum a layer-wise block of the ENGINE handed to the next one, from the
    emulation's sum of that block and the engine's stored x after it.  The engine's sum lies within half an fp16 ulp of
    its stored x; where the emulation's sum rounds to that x it is the better estimate (it carries the bits below fp16),
    elsewhere the emulation has left the engine's path (a quantizer flip upstream) and the stored x is what is known."""
    xs = np.asarray(xs_emulated, np.float64)
    x = np.asarray(x_stored, np.float64).reshape(xs.shape)
    return np.where(xs.astype(np.float16).astype(np.float64) == x, xs, x)


def block(cfg, W, k, x_in, scales_k=None, xa=None, codes=None):
    """Teacher-forced: layer-wise block k alone from the stored x_in ([n, C, 361] or [n, C, 19, 19]); xa: the unrounded
    sum of the block before it where that is layer-wise too (None: x_in); scales_k: the block's activation scales, or
    None for the unquantized fp16 block (activated tensors stored in fp16, fp16 weights).  codes (with scales_k): the
    engine's own int8 input of the block's first conv ([n, C, 361] integers, p3hip_debug_act_i8), taken in place of
    q(mish(bn0(xa))): codes * s quantizes back to the codes exactly.  Returns (x_out, xs) as [n, C, 19, 19] float64."""
    x = torch.from_numpy(np.asarray(x_in, np.float64).reshape(len(x_in), cfg.channels, 19, 19))
    a = x if xa is None else torch.from_numpy(np.asarray(xa, np.float64).reshape(x.shape))
    a0 = None
    if codes is not None:
        a0 = np.asarray(codes, np.float32).reshape(x.shape) * np.float32(scales_k[0])
        assert np.array_equal(quantize(a0, scales_k[0]), np.asarray(codes, np.float32).reshape(x.shape))
        a0 = torch.from_numpy(a0.astype(np.float64))
    out, xs = layerwise_block(cfg, k, x, a, _Q(W, scales_k, None), a0)
    return out.numpy(), xs.numpy()


def forward(cfg, W: Dict[str, np.ndarray], planes_nhwc, feats, scales=None, observe: Optional[list] = None):
    """The INT8_ANY engine's forward pass with `scales`, or (scales None) the fp16 plan it calibrates on with `observe`
    collecting the calibration maxima.  Outputs as oracle/torch_restatement.forward."""
    assert cfg.block_type in ("btl", "nbt", "classic"), cfg.name
    W = fp16_weights(cfg, W)
    if scales is not None:
        assert len(scales) == len(quantized_tensors(cfg))
    Q = _Q(W, scales, observe)
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
        x, xs = layerwise_block(cfg, i, x, xa, Q)
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
    import trunk_emulation as te
    cfg, W = config(name), weights(name)
    if scales is None:
        scales = minmax_scales(cfg, W, [te.inputs(c) for c in calibration_batches()])
    pos = cw.positions()
    ref = cw.outputs(cfg, W, pos, fp16=False)
    planes, sc = te.inputs(pos)
    return errors(forward(cfg, W, planes, sc, scales=scales), ref), scales


if __name__ == "__main__":   # the two measurements behind BOUNDS
    for n in (sys.argv[1:] or NETS):
        e1, s = emulation_errors(n)
        e2, _ = emulation_errors(n, (s * np.float32(1 + 2.0 ** -10)).astype(np.float32))
        print(n, *(tuple(float(f"{e[k]:.3g}") for k in ("logit", "prob", "value_prob")) for e in (e1, e2)), flush=True)
