"""Float64 PyTorch restatement of the transformer trunk (python/model_transformer.py TransformerBlock, config
b14d96h3_transformer) with the reference's stem and heads (model.py:1230-1295).

TEST INFRASTRUCTURE ONLY: used by tests/golden/make_transformer_golden.py and tests/test_transformer_cpu.py.  The
stem and the heads come from the helpers of oracle/torch_restatement.py; the block is written here, from the
reference's TransformerBlock.call and RoPE.call.

`fp16=True` rounds to fp16 where the engine stores fp16: the weights of every convolution and of every trunk GEMM
(the head denses stay fp32), the stem output, RMSNorm outputs, q / k / v after RoPE, the unnormalised softmax
numerators, the attention output, silu(gate) * up and the residual stream after every block (transformer.hip).  It
measures the error the engine's storage precision alone must produce.
"""
from __future__ import annotations

import os
import sys
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import torch_restatement as tr  # noqa: E402

RMS_EPS = 1e-6   # keras.layers.RMSNormalization default (the reference passes none; not verified against Keras here)
HEADS = 3
FP16_WEIGHTS = ("init_conv.w", "policy.conv_p.w", "policy.conv_g.w", "value.conv.w")   # besides blocks.*.w


QK_SCALE = 1.5   # the fixtures' Wq and Wk: random-init scale x1.5 (tests/golden/make_transformer_golden.py)


def fixture_weights(name):
    """Weights of the transformer fixtures: netspec's seeded random init (randomize=True) with Wq and Wk scaled by
    QK_SCALE, so that attention is clearly non-uniform."""
    from p3achygo_amd import netspec
    cfg = netspec.TRANSFORMER_CONFIGS[name]
    W = netspec.generate_weights(cfg, randomize=True)
    for i in range(cfg.blocks):
        for n in ("q", "k"):
            W[f"blocks.{i}.{n}.w"] = (W[f"blocks.{i}.{n}.w"] * np.float32(QK_SCALE)).astype(np.float32)
    return cfg, W


def rope_tables(num_rotations=4, head_dim=32, grid_len=19, theta=100.0):
    """spiral_rope_cos_sin_table (model_transformer.py), restated: [361][head_dim] cos and sin, float64."""
    per = head_dim // num_rotations
    nth = head_dim // 4
    thetas = theta ** (-np.arange(nth) / nth)
    th = np.zeros(head_dim)
    for i in range(head_dim):
        k, r = i // per, (i % per) // 2
        th[i] = thetas[min(nth - 1, 2 * (k % (num_rotations // 2)) + (r // 2) * num_rotations + r % 2)]
    s = np.arange(grid_len * grid_len)
    row, col = s // grid_len, s % grid_len          # meshgrid(indexing="ij"): the first coordinate is the row
    ang = (np.arange(head_dim) // per) * (np.pi / num_rotations)
    proj = row[:, None] * np.cos(ang)[None, :] + col[:, None] * np.sin(ang)[None, :]
    return np.cos(th[None, :] * proj), np.sin(th[None, :] * proj)


def _r16(x, on):
    return x.half().double() if on else x


def _rms(x, scale, on):
    return _r16(x * torch.rsqrt((x * x).mean(-1, keepdim=True) + RMS_EPS) * scale, on)


def _rope(x, cos, sin):
    """RoPE.call: x'[2j] = x[2j] cos + x[2j+1] sin, x'[2j+1] = x[2j] sin - x[2j+1] cos (a reflection, as written)."""
    sw = x.reshape(*x.shape[:-1], -1, 2).flip(-1).reshape(x.shape)
    sign = torch.ones(x.shape[-1], dtype=x.dtype)
    sign[1::2] = -1
    return x * cos * sign + sw * sin


def block(x, W, i, fp16=False, attn_probe=None):
    """TransformerBlock.call on token-major x [N][361][C]."""
    p = f"blocks.{i}"
    t = lambda n: torch.from_numpy(np.asarray(W[f"{p}.{n}"], np.float64))
    N, L, C = x.shape
    D = C // HEADS
    cos, sin = (torch.from_numpy(a)[None, :, None, :] for a in rope_tables(head_dim=D))
    res = x
    h = _rms(x, t("rms_in.scale"), fp16)
    q, k, v = (h @ t(n + ".w") for n in ("q", "k", "v"))
    q, k, v = (a.reshape(N, L, HEADS, D) for a in (q, k, v))
    q = _r16(_rope(q, cos, sin), fp16)
    k = _r16(_rope(k, cos, sin), fp16)
    v = _r16(v, fp16)
    s = torch.einsum("nqhd,nkhd->nhqk", q, k) / np.sqrt(D)    # dot_product_attention: no mask, scale 1/sqrt(D)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    pr = e / e.sum(-1, keepdim=True)
    if attn_probe is not None:
        attn_probe.append(pr)
    o = torch.einsum("nhqk,nkhd->nqhd", _r16(e, fp16), v) / e.sum(-1).permute(0, 2, 1)[..., None]
    o = _r16(o.reshape(N, L, C), fp16)
    x = res + o @ t("o.w")
    res = x
    h = _rms(x, t("rms_out.scale"), fp16)
    g = h @ t("ffn_gate.w")
    u = _r16(F.silu(g) * (h @ t("ffn_up.w")), fp16)
    return _r16(res + u @ t("ffn_down.w"), fp16)


def forward(cfg, W: Dict[str, np.ndarray], planes_nhwc, feats, fp16=False, attn_probe=None) -> Dict[str, np.ndarray]:
    """P3achyGoModel.call with a transformer trunk; outputs as oracle/torch_restatement.forward."""
    dtype = torch.float64
    if fp16:
        W = {k: (v.astype(np.float16).astype(np.float32) if k in FP16_WEIGHTS or k.startswith("blocks.") and k.endswith(".w")
                 else v) for k, v in W.items()}
    T = lambda n: tr._t(W[n], dtype)
    x = tr._t(planes_nhwc, dtype).permute(0, 3, 1, 2)
    gs = tr._dense(tr._t(feats, dtype), W, "init_game", dtype)
    x = tr._conv(x, T("init_conv.w")) + gs[:, :, None, None]
    N, C = x.shape[0], x.shape[1]
    x = _r16(x.permute(0, 2, 3, 1).reshape(N, 361, C), fp16)      # NHWC reshape: token s = 19 row + col
    for i in range(cfg.blocks):
        x = block(x, W, i, fp16, attn_probe if i == 0 else None)
    trunk = x
    x = x.reshape(N, 19, 19, C).permute(0, 3, 1, 2)
    return _heads(x, W, trunk, dtype)


def _heads(x, W, trunk, dtype):
    """PolicyHead.call and ValueHead.call (model.py:783-979), as oracle/torch_restatement.forward states them."""
    N = x.shape[0]
    T = lambda n: tr._t(W[n], dtype)
    p = tr._conv(x, T("policy.conv_p.w"))
    g = tr._mish(tr._bn(tr._conv(x, T("policy.conv_g.w")), W, "policy.gpool_bn", dtype))
    gp = tr._gpool(g)
    p = tr._mish(p + tr._dense(gp, W, "policy.gpool_dense", dtype)[:, :, None, None])
    pi2 = tr._conv(p, T("policy.out_moves.w")).reshape(N, 2, 361)
    pass2 = tr._dense(gp, W, "policy.out_pass", dtype) - 3
    pi_logits = torch.cat([pi2[:, 0], pass2[:, 0:1]], dim=1)
    opt = tr._conv(p, T("policy.opt_moves.w")).reshape(N, 361)
    opt_logits = torch.cat([opt, tr._dense(gp, W, "policy.opt_pass", dtype) - 3], dim=1)
    v = tr._conv(x, T("value.conv.w"))
    vp = tr._gpool(v)
    emb = tr._mish(tr._dense(vp, W, "value.oq_embed", dtype))
    go = tr._dense(emb, W, "value.oq_out", dtype)
    own = torch.tanh(tr._conv(v, T("value.own.w"))).reshape(N, 361)
    gamma = tr._dense(tr._mish(tr._dense(vp, W, "value.gamma_pre", dtype)), W, "value.gamma_out", dtype)
    scores = 0.05 * torch.arange(-400, 400, dtype=dtype) + 0.025
    vs = torch.cat([vp[:, None, :].expand(N, 800, vp.shape[1]), scores[None, :, None].expand(N, 800, 1)], dim=2)
    sl = tr._dense(tr._mish(tr._dense(vs, W, "value.score_pre", dtype)), W, "value.score_out", dtype)
    score_logits = torch.clamp(F.softplus(gamma), max=10.0) * sl.reshape(N, 800)
    raw = torch.cat([pi_logits, opt_logits, go[:, 0:2], score_logits, own, 4 * torch.sigmoid(go[:, 5:6]), gamma], dim=1)
    return {
        "raw": raw.double().numpy(),
        "move_probs": torch.softmax(pi_logits, 1).double().numpy(),
        "value_probs": torch.softmax(go[:, 0:2], 1).double().numpy(),
        "score_probs": torch.softmax(score_logits, 1).double().numpy(),
        "opt_move_probs": torch.softmax(opt_logits, 1).double().numpy(),
        "trunk": trunk.double().numpy(),
    }
