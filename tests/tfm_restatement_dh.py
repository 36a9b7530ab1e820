"""Float64 restatement of transformer trunks of any model width d and head count h (python/model_transformer.py
TransformerBlock with embed_dim d, num_heads h, head_dim d / h), with the reference's stem and heads.

TEST INFRASTRUCTURE ONLY: used by tests/golden/make_transformer_golden_dh.py and the tests of the nets of
netspec.WIDE_TRANSFORMER_CONFIGS.  RMSNorm, RoPE, the stem, the heads and the fp16 rounding points are those of
tests/tfm_restatement.py, which fixes h = 3; here the head count comes from the config (its bottleneck_channels, the
.p3w header's Cb) and the RoPE table has the config's head width.  At d = 96, h = 3 every operation is the one
tfm_restatement performs, in the same order, so the outputs are bit for bit the same.

fp16=True rounds where transformer.hip stores fp16, as tfm_restatement does.  At head width 64 k_tfm_attn's softmax is
online over blocks of 64 keys: a numerator is rounded to fp16 relative to the running maximum rather than the row's
maximum; both make it at most 1, so exp(s - max) rounded once stands for it here (the same relative step, no storage
point the emulation lacks).  That holds to one rounding of o, which is enough for the output-level bounds this module
serves; tests/tfm_emulation.py, which judges k_tfm_attn in fp16 ulps, emulates the online form itself and measures the
difference.  The block is written as its three stages (qkv_stage, attn_stage, ffn_stage: the three kernels), which
tfm_emulation.py calls one at a time.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

import tfm_restatement as tfm
from oracle import torch_restatement as tr

# Wq and Wk of the fixtures: the seeded random init times this (tests/golden/make_transformer_golden_dh.py chose the
# smallest of 1.5, 2.0, 2.5, 3.0 that peaks every head of block 0: mean largest attention probability >= 0.05)
QK_SCALES = {
    "test_b2d96h3_tfm": 1.5, "b14d96h3_transformer": 1.5,
    "test_b2d64h2_tfm": 1.5, "test_b2d128h2_tfm": 1.5, "test_b2d192h6_tfm": 1.5, "test_b2d256h4_tfm": 1.5,
    "test_b2d384h12_tfm": 1.5, "test_b2d384h6_tfm": 1.5,
}


def fixture_weights(name, qk_scale=None):
    """netspec's seeded random init (randomize=True) of config `name` with Wq and Wk scaled by QK_SCALES[name]."""
    from p3achygo_amd import netspec
    cfg = netspec.get_config(name)
    W = netspec.generate_weights(cfg, randomize=True)
    s = np.float32(QK_SCALES[name] if qk_scale is None else qk_scale)
    for i in range(cfg.blocks):
        for n in ("q", "k"):
            W[f"blocks.{i}.{n}.w"] = (W[f"blocks.{i}.{n}.w"] * s).astype(np.float32)
    return cfg, W


def _wt(W, i, n):
    return torch.from_numpy(np.asarray(W[f"blocks.{i}.{n}"], np.float64))


def qkv_stage(x, W, i, heads, fp16=False):
    """RMSNorm_in, the three projections and RoPE on q and k of block i: x [N][361][C] -> q, k, v [N][361][heads][D]."""
    N, L, C = x.shape
    D = C // heads
    cos, sin = (torch.from_numpy(a)[None, :, None, :] for a in tfm.rope_tables(head_dim=D))
    h = tfm._rms(x, _wt(W, i, "rms_in.scale"), fp16)
    q, k, v = (h @ _wt(W, i, n + ".w") for n in ("q", "k", "v"))
    q, k, v = (a.reshape(N, L, heads, D) for a in (q, k, v))
    q = tfm._r16(tfm._rope(q, cos, sin), fp16)
    k = tfm._r16(tfm._rope(k, cos, sin), fp16)
    v = tfm._r16(v, fp16)
    return q, k, v


def attn_stage(q, k, v, fp16=False, attn_probe=None):
    """dot_product_attention (no mask, scale 1 / sqrt(D)) on q, k, v [N][361][heads][D] -> o [N][361][C]; fp16: the
    numerators rounded once, relative to the row's maximum."""
    N, L, heads, D = q.shape
    s = torch.einsum("nqhd,nkhd->nhqk", q, k) / np.sqrt(D)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    pr = e / e.sum(-1, keepdim=True)
    if attn_probe is not None:
        attn_probe.append(pr)
    o = torch.einsum("nhqk,nkhd->nqhd", tfm._r16(e, fp16), v) / e.sum(-1).permute(0, 2, 1)[..., None]
    return tfm._r16(o.reshape(N, L, heads * D), fp16)


def ffn_stage(o, x, W, i, fp16=False):
    """o . Wo + x, RMSNorm_out, SwiGLU, . Wdown + residual of block i: o, x [N][361][C] -> the next x."""
    x = x + o @ _wt(W, i, "o.w")
    res = x
    h = tfm._rms(x, _wt(W, i, "rms_out.scale"), fp16)
    g = h @ _wt(W, i, "ffn_gate.w")
    u = tfm._r16(F.silu(g) * (h @ _wt(W, i, "ffn_up.w")), fp16)
    return tfm._r16(res + u @ _wt(W, i, "ffn_down.w"), fp16)


def block(x, W, i, heads, fp16=False, attn_probe=None):
    """TransformerBlock.call on token-major x [N][361][C] with `heads` heads (tfm_restatement.block, h free), in its
    three stages: the three kernels of transformer.hip, which tests/tfm_emulation.py judges one at a time."""
    q, k, v = qkv_stage(x, W, i, heads, fp16)
    o = attn_stage(q, k, v, fp16, attn_probe)
    return ffn_stage(o, x, W, i, fp16)


def forward(cfg, W: Dict[str, np.ndarray], planes_nhwc, feats, fp16=False, attn_probe=None) -> Dict[str, np.ndarray]:
    """P3achyGoModel.call with a transformer trunk of cfg.channels and cfg.bottleneck_channels heads; outputs as
    tfm_restatement.forward."""
    dtype = torch.float64
    if fp16:
        W = {k: (v.astype(np.float16).astype(np.float32) if k in tfm.FP16_WEIGHTS or k.startswith("blocks.") and k.endswith(".w")
                 else v) for k, v in W.items()}
    T = lambda n: tr._t(W[n], dtype)
    x = tr._t(planes_nhwc, dtype).permute(0, 3, 1, 2)
    gs = tr._dense(tr._t(feats, dtype), W, "init_game", dtype)
    x = tr._conv(x, T("init_conv.w")) + gs[:, :, None, None]
    N, C = x.shape[0], x.shape[1]
    x = tfm._r16(x.permute(0, 2, 3, 1).reshape(N, 361, C), fp16)      # NHWC reshape: token s = 19 row + col
    for i in range(cfg.blocks):
        x = block(x, W, i, cfg.bottleneck_channels, fp16, attn_probe if i == 0 else None)
    trunk = x
    x = x.reshape(N, 19, 19, C).permute(0, 3, 1, 2)
    return tfm._heads(x, W, trunk, dtype)


def attention_peak(probe):
    """per head of block 0: the mean over positions and queries of the largest attention probability"""
    return probe[0].amax(-1).mean(dim=(0, 2)).numpy()
