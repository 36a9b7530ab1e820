"""What tests/test_fp32_cpu.py and tests/test_fp32_gpu.py share: the nets the fp32 plan (P3HIP_FLAG_FP32,
csrc/conv_f32.hip) is tested on, their weights and positions, the float64 restatement of their outputs
(tests/trunk_emulation.py Trunk with fp16=False and .layerwise set, heads through tfm_restatement._heads), the fp32 twin
(the same trunk in float32 torch arithmetic with the engine's fp32 BN fold and mish_f, no fp16 rounding anywhere), the
bounds and the block-by-block measure.

Bounds on the outputs: what tests/test_oracle_cpu.py demands of the fp32 C oracle against the float64 fixtures.

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

SMALL_NETS = ["test_b3c128btl2", "test_b3c256nbt", "test_b3c384btl3", "test_b3c192classic", "test_b5c256btl2_i2",
              "test_b3c96nbt", "test_b3c320nbt", "test_b4c512btl3_i2"]
DEEP_NET = "b12c256btl3"          # on its 32 golden positions
PADDED_NETS = ["test_b3c96nbt", "test_b3c320nbt"]
BLOCK_NETS = ["test_b3c320nbt", "test_b4c512btl3_i2", "test_b3c192classic", "test_b3c128btl2"]
OFFSET_NET = "test_b3c512nbt"
PROB_KEYS = ("move_probs", "value_probs", "score_probs", "opt_move_probs")
NPOS, SEED = 16, 11

RAW_TOL, PROB_TOL = 2e-5, 1e-6              # the 3-5 block nets
DEEP_RAW_TOL, DEEP_PROB_TOL = 1e-4, 2e-6    # b12c256btl3
BLOCK_FACTOR = 4.0   # the engine's block error against float64 may be this many times the twin's on the same input


def config(name):
    from p3achygo_amd import netspec
    return netspec.get_config(name)


def weights(name):
    from p3achygo_amd import netspec
    return netspec.generate_weights(config(name), randomize=True)


def padded(c):
    return (c + 63) // 64 * 64


def positions(n=NPOS, seed=SEED):
    from p3achygo_amd import features
    return features.random_positions(n, seed=seed)


def restatement(cfg, W):
    t = te.Trunk(cfg, W, fp16=False)
    t.layerwise = True
    return t


def twin(cfg, W):
    """float32 torch convolutions, the engine's fp32 BN fold and mish_f, no fp16 rounding"""
    t = te.Trunk(cfg, W, twin=True)
    t.fp16 = False
    t.layerwise = True
    return t


def outputs(t, pos):
    """raw [n, 1889] and the four distributions of trunk `t` (the restatement in float64, the twin in float32)"""
    x = t.trunk(features=pos)[-1]
    out = tfm_restatement._heads(x.to(t.dt), t.W, x, t.dt)
    return {k: out[k] for k in ("raw",) + PROB_KEYS}


def errors(ref, got):
    """(largest raw-output error, largest probability error)"""
    return (float(np.abs(got["raw"] - ref["raw"]).max()),
            max(float(np.abs(got[k] - ref[k]).max()) for k in PROB_KEYS))


def golden_reference(name):
    """(positions, outputs) of a committed fixture tests/golden/nn_<name>.npz"""
    from conftest import load_golden
    g, pos = load_golden(name)
    return pos, {k: np.asarray(g[k], np.float64) for k in ("raw",) + PROB_KEYS}


def check_outputs(name, raw, res, own, ref, i, raw_tol, prob_tol):
    """one slot of the engine (raw row, result record, ownership) against row i of the reference; returns its largest
    raw-output and probability errors"""
    assert np.isfinite(raw).all(), name
    d_raw = float(np.abs(raw - ref["raw"][i]).max())
    assert d_raw <= raw_tol, (name, "raw", d_raw)
    d_prob = 0.0
    for key in PROB_KEYS:
        d = float(np.abs(np.ctypeslib.as_array(getattr(res, key)) - ref[key][i]).max())
        assert d <= prob_tol, (name, key, d)
        d_prob = max(d_prob, d)
    assert np.array_equal(np.ctypeslib.as_array(res.move_logits), raw[:362])
    assert np.array_equal(own, raw[1526:1887])
    return d_raw, d_prob


def block_errors(cfg, W, xs, pos):
    """xs = [x after the stem, x after block 0, ...] of some fp32 evaluation ([n, C, 361] each, the file's channels),
    each block started from xs' own x before it.  Returns rows (label, error of xs, error of the twin), both
    max |x - x_f64| / scale with scale = trunk_emulation.block_scale (the stem: rms)."""
    C = cfg.channels
    f64, tw = restatement(cfg, W), twin(cfg, W)
    xt = [torch.from_numpy(np.asarray(x, np.float64).reshape(len(x), C, 19, 19)) for x in xs]
    m, t = f64.stem(pos), tw.stem(pos)
    rows = [("stem", float((xt[0] - m).abs().max()) / te.rms(m), float((t - m).abs().max()) / te.rms(m))]
    for k in range(len(xt) - 1):
        m, t = f64.block(k, xt[k]), tw.block(k, xt[k])
        s = te.block_scale(xt[k], m)
        rows.append((f"{k} ({cfg.block_kind(k)})", float((xt[k + 1] - m).abs().max()) / s, float((t - m).abs().max()) / s))
    return rows
