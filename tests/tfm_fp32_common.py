"""What tests/test_transformer_fp32_cpu.py and tests/test_transformer_fp32_gpu.py share: the nets the fp32 plan of the
transformer trunks (P3HIP_FLAG_FP32_TFM, csrc/transformer_f32.hip) is tested on, their weights and positions, the float64
reference, the fp32 twin, the bounds and the kernel-by-kernel measure.

Reference: the float64 restatement tests/tfm_restatement_dh.py (forward, qkv_stage, attn_stage, ffn_stage) on
fixture_weights(name), recomputed here.  The stored tests/golden/nn_*_tfm.npz give the positions, planes and scalars
only: their outputs are float32 and carry their own rounding.  b14d96h3_transformer runs the first 8 positions of the
test_b2d96h3_tfm fixture.

Twin: the same three stages in float32 torch (float32 matmuls, softmax as exp(s - max) / sum, RMSNorm with torch.rsqrt,
torch's silu), the stem and the heads in float32 too, the RoPE tables the float32 of the float64 tables (what the engine
uploads).  No fp16 rounding anywhere.

Bounds on the outputs, one rule: twice the twin's worst over the nets of the group, rounded up to one significant
digit (test_transformer_fp32_cpu.py re-measures the twin and holds it to half of each).  The factor 2 is for the MFMA's
summation order; the conv fp32 plan measured 0.6 - 1.4 times its twin on an MI355X.
    group                       twin's worst raw / prob    RAW_TOL / PROB_TOL
    the seven two-block nets    1.15e-5 / 6.9e-7           3e-5 / 2e-6
    b14d96h3_transformer        1.22e-5 / 7.0e-7           3e-5 / 2e-6
(per net: the docstring of tests/test_transformer_fp32_cpu.py)

TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import tfm_restatement as tfm  # noqa: E402
import tfm_restatement_dh as dh  # noqa: E402
import trunk_emulation as te  # noqa: E402
from fp32_common import check_outputs  # noqa: E402,F401  (one slot of the engine against row i of a reference)

NETS = ["test_b2d64h2_tfm", "test_b2d96h3_tfm", "test_b2d128h2_tfm", "test_b2d192h6_tfm", "test_b2d256h4_tfm",
        "test_b2d384h12_tfm", "test_b2d384h6_tfm"]
DEEP_NET, DEEP_POSITIONS_OF, DEEP_NPOS = "b14d96h3_transformer", "test_b2d96h3_tfm", 8
KERNEL_NETS = ["test_b2d96h3_tfm", "test_b2d256h4_tfm", "test_b2d384h12_tfm"]   # D = 32 / 64 (blocked keys) / widest
HOT_NETS = ["test_b2d96h3_tfm", "test_b2d256h4_tfm"]
PROB_KEYS = ("move_probs", "value_probs", "score_probs", "opt_move_probs")
L, LPAD = 361, 384

RAW_TOL, PROB_TOL = 3e-5, 2e-6              # the seven two-block nets
DEEP_RAW_TOL, DEEP_PROB_TOL = 3e-5, 2e-6    # b14d96h3_transformer
BLOCK_FACTOR = 4.0   # a kernel's error against float64 may be this many times the twin's on the same input (fp32_common)


def rule(worst):
    """twice `worst`, rounded up to one significant digit"""
    v = 2.0 * worst
    e = 10.0 ** np.floor(np.log10(v))
    return float(np.ceil(v / e - 1e-9) * e)


def tolerances(name):
    return (DEEP_RAW_TOL, DEEP_PROB_TOL) if name == DEEP_NET else (RAW_TOL, PROB_TOL)


def stream_width(d):
    return 128 if d <= 128 else (256 if d <= 256 else 384)


def inputs(name):
    """(feature records, planes NHWC, scalars) of the net's positions, from the committed fixture"""
    from conftest import load_golden
    g, pos = load_golden(DEEP_POSITIONS_OF if name == DEEP_NET else name)
    n = DEEP_NPOS if name == DEEP_NET else len(pos)
    return pos[:n], np.asarray(g["planes"])[:n], np.asarray(g["scalars"])[:n]


def weights(name, hot=False):
    """(cfg, W): the fixture weights; hot: Wq, Wk x 4 (tfm_emulation.hot_weights)"""
    if hot:
        import tfm_emulation
        return tfm_emulation.hot_weights(name)
    return dh.fixture_weights(name)


def reference(name):
    """(positions, float64 outputs of them)"""
    cfg, W = weights(name)
    pos, planes, scalars = inputs(name)
    out = dh.forward(cfg, W, planes, scalars)
    return pos, {k: np.asarray(out[k], np.float64) for k in ("raw",) + PROB_KEYS}


def errors(ref, got):
    """(largest raw-output error, largest probability error)"""
    return (float(np.abs(got["raw"] - ref["raw"]).max()),
            max(float(np.abs(got[k] - ref[k]).max()) for k in PROB_KEYS))


class Twin:
    """The trunk in float32 torch, stage by stage.  x and o are [N][361][d]; q, k, v are [N][361][heads][D]."""

    def __init__(self, cfg, W):
        self.cfg, self.W = cfg, W
        self.d, self.nh = cfg.channels, cfg.bottleneck_channels
        self.D = self.d // self.nh
        cos, sin = tfm.rope_tables(head_dim=self.D)
        self.cos, self.sin = (torch.from_numpy(a.astype(np.float32))[None, :, None, :] for a in (cos, sin))
        self._stem = te.Trunk(cfg, W, twin=True)
        self._stem.fp16 = False

    def w(self, i, n):
        return torch.from_numpy(np.asarray(self.W[f"blocks.{i}.{n}"], np.float32))

    @staticmethod
    def rms(x, scale):
        inv = torch.rsqrt((x * x).sum(-1, keepdim=True) * np.float32(1.0 / x.shape[-1]) + np.float32(1e-6))
        return x * inv * scale

    def qkv(self, i, x):
        x = torch.as_tensor(x).float()
        N = x.shape[0]
        h = self.rms(x, self.w(i, "rms_in.scale"))
        q, k, v = ((h @ self.w(i, n + ".w")).reshape(N, L, self.nh, self.D) for n in ("q", "k", "v"))
        return tfm._rope(q, self.cos, self.sin), tfm._rope(k, self.cos, self.sin), v

    def attn(self, q, k, v):
        q, k, v = (torch.as_tensor(a).float() for a in (q, k, v))
        N = q.shape[0]
        s = torch.einsum("nqhd,nkhd->nhqk", q, k) / np.float32(np.sqrt(self.D))
        e = torch.exp(s - s.amax(-1, keepdim=True))
        o = torch.einsum("nhqk,nkhd->nqhd", e, v) / e.sum(-1).permute(0, 2, 1)[..., None]
        return o.reshape(N, L, self.d)

    def ffn(self, i, o, x):
        o, x = torch.as_tensor(o).float(), torch.as_tensor(x).float()
        x1 = x + o @ self.w(i, "o.w")
        h = self.rms(x1, self.w(i, "rms_out.scale"))
        u = F.silu(h @ self.w(i, "ffn_gate.w")) * (h @ self.w(i, "ffn_up.w"))
        return x1 + u @ self.w(i, "ffn_down.w")

    def forward(self, planes, scalars):
        x = self._stem.stem(planes=planes, scalars=scalars).float()     # [N][d][19][19]
        N = x.shape[0]
        x = x.reshape(N, self.d, L).permute(0, 2, 1).contiguous()
        for i in range(self.cfg.blocks):
            x = self.ffn(i, self.attn(*self.qkv(i, x)), x)
        out = tfm._heads(x.reshape(N, 19, 19, self.d).permute(0, 3, 1, 2), self.W, x, torch.float32)
        return {k: np.asarray(out[k], np.float64) for k in ("raw",) + PROB_KEYS}


def twin_errors(name):
    """the twin's (raw, prob) errors against the float64 restatement on the net's positions"""
    cfg, W = weights(name)
    _, planes, scalars = inputs(name)
    _, ref = reference(name)
    return errors(ref, Twin(cfg, W).forward(planes, scalars))


# ---- kernel by kernel ----------------------------------------------------------------------------------------------

def rel(a, ref):
    """max |a - ref| / rms(ref)"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / np.sqrt((ref * ref).mean()))


def tokens(x_debug, d):
    """HipEngine.debug_x's [n][Cs][361] -> the model's channels token-major [n][361][d], float64"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x_debug, np.float64)[:, :d].transpose(0, 2, 1)))


def heads_first(a):
    """HipEngine.debug_tfm's [n][head][384][D] -> [n][361][head][D], float64"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)[:, :, :L].transpose(0, 2, 1, 3)))


def kernel_rows(cfg, W, rec, stages=("qkv", "attn", "ffn")):
    """rec = {"x": [x0 .. x_B] [n][361][d], "q" / "k" / "v": [n][361][head][D] per block, "o": [n][361][d] per block}
    of some fp32 evaluation, float64 tensors.  Every kernel's output against the float64 stage on rec's own inputs, and
    the twin's on the same inputs: rows (kernel, tensor, block, error of rec, error of the twin) in the order the
    kernels run."""
    tw = Twin(cfg, W)
    nh = cfg.bottleneck_channels
    rows = []
    for i in range(len(rec["o"])):
        if "qkv" in stages:
            want = dh.qkv_stage(rec["x"][i], W, i, nh)
            for t, m, g in zip("qkv", want, tw.qkv(i, rec["x"][i])):
                rows.append(("k_tfm_qkv_f32", t, i, rel(rec[t][i], m), rel(g.double(), m)))
        if "attn" in stages:
            m = dh.attn_stage(rec["q"][i], rec["k"][i], rec["v"][i])
            rows.append(("k_tfm_attn_f32", "o", i, rel(rec["o"][i], m),
                         rel(tw.attn(rec["q"][i], rec["k"][i], rec["v"][i]).double(), m)))
        if "ffn" in stages:
            m = dh.ffn_stage(rec["o"][i], rec["x"][i], W, i)
            rows.append(("k_tfm_ffn_f32", "x", i, rel(rec["x"][i + 1], m),
                         rel(tw.ffn(i, rec["o"][i], rec["x"][i]).double(), m)))
    return rows


def check_rows(name, rows):
    """every row within BLOCK_FACTOR times the twin, in order: the first that is not raises, naming kernel, tensor, block"""
    for kernel, t, i, eng_err, twin_err in rows:
        assert np.isfinite(eng_err) and eng_err <= BLOCK_FACTOR * twin_err, \
            f"{name} block {i} {kernel} {t}: engine {eng_err:.3e} twin {twin_err:.3e}"
