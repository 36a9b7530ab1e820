"""What tests/test_conv_widths_cpu.py and tests/test_conv_widths_gpu.py share: the nets of netspec.WIDE_CONV_CONFIGS
under test, their weights and positions, the float64 reference and the fp16 emulation of their outputs
(tests/trunk_emulation.py Trunk with .layerwise set: every width of conv_any.hip runs layer by layer), the tolerances
derived from the emulation, and the block-by-block checker with the layer-wise bounds.

TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import tfm_restatement  # noqa: E402
import trunk_emulation as te  # noqa: E402

NETS = ["test_b3c64btl2", "test_b3c96nbt", "test_b3c192btl3", "test_b3c256btl2_cb64", "test_b3c128classic",
        "test_b3c320nbt", "test_b3c512nbt", "test_b4c512btl3_i2", "b12c192btl3", "b10c512nbt"]
PADDED_NETS = ["test_b3c96nbt", "test_b3c192btl3", "test_b3c320nbt"]        # C or C_b not a multiple of 64
BLOCK_NETS = ["test_b3c320nbt", "test_b4c512btl3_i2", "test_b3c128classic"]
PATH_NETS = ["test_b3c192btl3", "test_b3c512nbt"]
PROB_KEYS = ("move_probs", "value_probs", "score_probs", "opt_move_probs")
NPOS, SEED = 16, 11

# tests/test_engine_gpu.py
LOGIT_TOL, LOGIT_REL, PROB_TOL, VALUE_PROB_TOL, KL_TOL = 6e-3, 1e-3, 5e-5, 5e-4, 2e-6
BASE = {"logit": LOGIT_TOL, "move_probs": PROB_TOL, "value_probs": VALUE_PROB_TOL, "score_probs": PROB_TOL,
        "opt_move_probs": PROB_TOL, "kl": KL_TOL}
COLUMNS = ("logit", "move_probs", "value_probs", "score_probs", "opt_move_probs", "kl")


def padded(c):
    return (c + 63) // 64 * 64


def config(name):
    from p3achygo_amd import netspec
    return netspec.WIDE_CONV_CONFIGS[name]


def weights(name):
    from p3achygo_amd import netspec
    return netspec.generate_weights(config(name), randomize=True)


def positions(n=NPOS, seed=SEED):
    from p3achygo_amd import features
    return features.random_positions(n, seed=seed)


def trunk(cfg, W, fp16=True, twin=False):
    t = te.Trunk(cfg, W, fp16=fp16, twin=twin)
    t.layerwise = True   # is_layerwise knows the templated widths only
    return t


def outputs(cfg, W, pos, fp16):
    """raw [n, 1889] and the four distributions (float64) of the float64 restatement or of the fp16 emulation"""
    t = trunk(cfg, W, fp16=fp16)
    x = t.trunk(features=pos)[-1]
    Wh = W
    if fp16:
        Wh = {k: (v.astype(np.float16).astype(np.float32) if k in te.HEAD_CONVS else v) for k, v in W.items()}
    out = tfm_restatement._heads(x.to(te.F64), Wh, x, te.F64)
    return {k: out[k] for k in ("raw",) + PROB_KEYS}


def pad_weights(cfg, W):
    """(cfg, W) with C and C_b zero-padded to multiples of 64 by the engine's rule (weights.h WeightFile::pad_conv):
    zero conv rows and columns, zero stem weights and bias, BN gamma = beta = mean = var = 0"""
    import dataclasses
    from p3achygo_amd import netspec
    C, Cb = cfg.channels, cfg.bottleneck_channels
    big = dataclasses.replace(cfg, channels=padded(C), bottleneck_channels=Cb if cfg.block_type == "classic" else padded(Cb))
    out = {}
    for name, shape, _ in netspec.tensor_specs(big):
        w = np.zeros(shape, np.float32)
        w[tuple(slice(0, d) for d in W[name].shape)] = W[name]
        out[name] = w
    return big, out


def kl(p, q):
    p, q = np.asarray(p, np.float64), np.maximum(np.asarray(q, np.float64), 1e-30)
    m = p > 0
    return float(np.sum(p[m] * (np.log(p[m]) - np.log(q[m]))))


def emulated_errors(ref, emu):
    """the six columns of the table in tests/test_conv_widths_gpu.py: the emulation's largest error in each"""
    raw, out = ref["raw"], emu["raw"]
    d = np.abs(out - raw)
    # logit: the largest raw-output error; logit_share: the largest error as a share of max(LOGIT_TOL, LOGIT_REL |ref|)
    e = {"logit": float(d.max()), "logit_share": float((d / np.maximum(LOGIT_TOL, LOGIT_REL * np.abs(raw))).max())}
    for k in PROB_KEYS:
        e[k] = float(np.abs(emu[k] - ref[k]).max())
    e["kl"] = max(kl(ref[k][i], emu[k][i]) for k in PROB_KEYS for i in range(len(raw)))
    return e


def tolerance(err):
    """the rule of tests/test_transformer_widths_gpu.py: the bound of tests/test_engine_gpu.py where the emulation
    stays at or below half of it, else twice the emulated error"""
    t = {c: (BASE[c] if err[c] <= BASE[c] / 2 else 2 * err[c]) for c in COLUMNS}
    t["logit"] = LOGIT_TOL if err["logit_share"] <= 0.5 else 2 * err["logit"]
    return t


def check_outputs(name, tol, raw, res, ref, i):
    """one slot of the engine (raw row and result record) against row i of the reference"""
    want = ref["raw"][i]
    assert not np.isnan(raw).any(), name
    lim = np.maximum(tol["logit"], LOGIT_REL * np.abs(want))
    assert (np.abs(raw - want) <= lim).all(), (name, float(np.abs(raw - want).max()))
    for key in PROB_KEYS:
        got = np.ctypeslib.as_array(getattr(res, key))
        assert np.abs(got - ref[key][i]).max() <= tol[key], (name, key, float(np.abs(got - ref[key][i]).max()))
        assert kl(ref[key][i], got) <= tol["kl"], (name, key)
    assert np.array_equal(np.ctypeslib.as_array(res.move_logits), raw[:362])


def kind_of(cfg, k):
    """the trunk_emulation.BOUNDS key of block k of a net that runs layer by layer"""
    kind = cfg.block_kind(k)
    return "lw_" + kind if kind in ("btl", "nbt") else kind


def teacher_forced(t, xs_engine, pos, slots=None, label="", bounds=None):
    """trunk_emulation.teacher_forced with the layer-wise bounds for every width: the stem and every block of trunk `t`
    checked from the engine's own x before it.  bounds: {BOUNDS key: (max err, min identical)} overrides."""
    cfg = t.cfg
    C = cfg.channels
    B = dict(te.BOUNDS)
    B.update(bounds or {})
    xs = [torch.from_numpy(np.asarray(x, np.float64).reshape(len(x), C, 19, 19)) for x in xs_engine]
    x0 = t.stem(pos)
    out = {"stem": te.check_block(xs[0], x0, te.rms(x0), f"{label}stem", slots, *B["stem"])}
    for k in range(len(xs) - 1):
        m = t.block(k, xs[k])
        out[k] = te.check_block(xs[k + 1], m, te.block_scale(xs[k], m), f"{label}{k} ({cfg.block_kind(k)})", slots,
                                *B[kind_of(cfg, k)])
    return out
