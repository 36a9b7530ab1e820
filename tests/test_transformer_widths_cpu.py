"""Transformer trunks of other widths and head counts without a GPU: the engine's RoPE tables of head width 32 and 64
against the reference's, the restatement of any (d, h) against tfm_restatement and its own fixtures, the attention
criterion of the fixture weights, the fp16 emulation against the GPU bounds, and p3hip_create's architecture check,
which runs before the device check."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import tfm_restatement as tfm  # noqa: E402
import tfm_restatement_dh as dh  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
PROB_KEYS = ("move_probs", "value_probs", "score_probs", "opt_move_probs")
MIN_PEAK = 0.05   # tests/golden/make_transformer_golden.py


def test_rope_table_dim_32_is_the_reference_table(built):
    from p3achygo_amd import engine
    d = np.load(os.path.join(GOLD, "rope_spiral_d32_r4_b19.npz"))
    cos, sin = engine.rope_table_dim(32)
    assert np.abs(cos - d["cos"]).max() <= 1e-12 and np.abs(sin - d["sin"]).max() <= 1e-12
    c0, s0 = engine.rope_table()
    assert np.array_equal(cos, c0) and np.array_equal(sin, s0)


def test_rope_table_dim_64_is_the_reference_table(built):
    from p3achygo_amd import engine
    d = np.load(os.path.join(GOLD, "rope_spiral_d64_r4_b19.npz"))
    assert int(d["head_dim"]) == 64 and d["cos"].shape == (361, 64)
    cos, sin = engine.rope_table_dim(64)
    assert np.abs(cos - d["cos"]).max() <= 1e-12 and np.abs(sin - d["sin"]).max() <= 1e-12
    rc, rs = tfm.rope_tables(head_dim=64)
    assert np.abs(rc - d["cos"]).max() <= 1e-12 and np.abs(rs - d["sin"]).max() <= 1e-12


@pytest.mark.parametrize("width", [16, 48, 128, 0])
def test_rope_table_dim_refuses_other_widths(built, width):
    from p3achygo_amd import engine
    with pytest.raises(ValueError, match="head width"):
        engine.rope_table_dim(width)


@pytest.mark.parametrize("fp16", [False, True])
def test_restatement_at_d96h3_is_tfm_restatement_bit_for_bit(fp16):
    from p3achygo_amd import netspec
    g, _ = load_golden("test_b2d96h3_tfm")
    cfg = netspec.TRANSFORMER_CONFIGS["test_b2d96h3_tfm"]
    W = tfm.fixture_weights("test_b2d96h3_tfm")[1]
    W2 = dh.fixture_weights("test_b2d96h3_tfm")[1]
    assert all(np.array_equal(W[k], W2[k]) for k in W)
    n = 8
    a = tfm.forward(cfg, W, g["planes"][:n].astype(np.float32), g["scalars"][:n], fp16=fp16)
    b = dh.forward(cfg, W, g["planes"][:n].astype(np.float32), g["scalars"][:n], fp16=fp16)
    for k in ("raw", "trunk") + PROB_KEYS:
        assert np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def restated():
    """name -> (golden, float64 outputs with the attention probe, fp16 emulation) of every wide net"""
    from p3achygo_amd import netspec
    out = {}
    for name in netspec.WIDE_TRANSFORMER_CONFIGS:
        g, _ = load_golden(name)
        cfg, W = dh.fixture_weights(name)
        probe = []
        ref = dh.forward(cfg, W, g["planes"].astype(np.float32), g["scalars"], attn_probe=probe)
        emu = dh.forward(cfg, W, g["planes"].astype(np.float32), g["scalars"], fp16=True)
        out[name] = (g, ref, dh.attention_peak(probe), emu)
    return out


def test_wide_nets_cover_every_stream_width_and_both_head_widths():
    from p3achygo_amd import netspec
    cfgs = list(netspec.WIDE_TRANSFORMER_CONFIGS.values())
    assert {c.channels // c.bottleneck_channels for c in cfgs} == {32, 64}
    assert {(128 if c.channels <= 128 else 256 if c.channels <= 256 else 384) for c in cfgs} == {128, 256, 384}
    assert all(netspec.transformer_supported(c.channels, c.bottleneck_channels) for c in cfgs)
    assert not set(netspec.WIDE_TRANSFORMER_CONFIGS) & (set(netspec.CONFIGS) | set(netspec.TRANSFORMER_CONFIGS))


def test_restatement_reproduces_the_fixtures_and_attention_is_peaked(restated):
    for name, (g, ref, peak, _) in restated.items():
        assert np.abs(ref["raw"] - g["raw"]).max() <= 1e-6 * max(1.0, float(np.abs(g["raw"]).max())), name
        for k in PROB_KEYS:
            assert np.abs(ref[k] - g[k]).max() <= 1e-7, (name, k)
        # the criterion of make_transformer_golden.py: every head of block 0
        assert (peak >= MIN_PEAK).all(), (name, peak)
        assert np.allclose(peak, g["attn_peak"], rtol=1e-9, atol=0)
        assert float(g["qk_scale"]) == dh.QK_SCALES[name]
        W = dh.fixture_weights(name)[1]
        wsum = sum(float(w.astype(np.float64).sum()) for w in W.values())
        wsq = sum(float((w.astype(np.float64) ** 2).sum()) for w in W.values())
        assert np.allclose(g["weight_checksum"], [wsum, wsq], rtol=1e-12, atol=1e-9), name


def test_fp16_emulation_stays_inside_half_the_gpu_bounds(restated):
    from test_transformer_gpu import _kl
    from test_transformer_widths_gpu import TOL
    assert set(TOL) == set(restated)
    for name, (g, _, _, out) in restated.items():
        t = TOL[name]
        raw = g["raw"]
        assert (np.abs(out["raw"] - raw) <= np.maximum(t["logit"], 1e-3 * np.abs(raw)) / 2).all(), name
        for k in PROB_KEYS:
            assert np.abs(out[k] - g[k]).max() <= t["prob"][k] / 2, (name, k)
            assert max(_kl(g[k][i], out[k][i]) for i in range(len(raw))) <= t["kl"] / 2, (name, k)


def test_p3w_round_trip_and_flops_of_wide_configs(tmp_path):
    from p3achygo_amd import netspec
    L = 361
    for name, cfg in netspec.WIDE_TRANSFORMER_CONFIGS.items():
        W = netspec.generate_weights(cfg, randomize=True)
        p = str(tmp_path / (name + ".p3w"))
        netspec.save_p3w(p, cfg, W)
        c2, W2, _ = netspec.load_p3w(p)
        assert (c2.blocks, c2.channels, c2.bottleneck_channels, c2.c_val, c2.block_type) == \
            (cfg.blocks, cfg.channels, cfg.bottleneck_channels, cfg.c_val, "transformer")
        assert set(W2) == set(W) and all(np.array_equal(W2[k], W[k]) for k in W)
        C = cfg.channels
        per_block = 2 * (4 * L * C * C + 2 * L * L * C + 6 * L * C * C)
        stem = netspec.flops_per_position(netspec.transformer_config("x", 1, C, cfg.bottleneck_channels,
                                                                      c_val=cfg.c_val))[0] - per_block
        assert abs(netspec.flops_per_position(cfg)[0] - (cfg.blocks * per_block + stem)) < 1.0


def _create(path):
    """p3hip_create on device 0: (engine handle or None, error message)"""
    from p3achygo_amd import engine
    L = engine.lib()
    h = L.p3hip_create(path.encode(), 4, 1, 0, 0)
    return h, (L.p3hip_create_error() or b"").decode()


@pytest.mark.parametrize("name", ["test_b2d64h2_tfm", "test_b2d128h2_tfm", "test_b2d192h6_tfm", "test_b2d256h4_tfm",
                                  "test_b2d384h12_tfm", "test_b2d384h6_tfm", "test_b2d96h3_tfm"])
def test_create_accepts_every_supported_width(built, tmp_path, name):
    """the architecture check runs before the device check: without a GPU the only refusal is the missing device"""
    from p3achygo_amd import engine, netspec
    cfg = netspec.get_config(name)
    path = str(tmp_path / "t.p3w")
    netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
    h, err = _create(path)
    if h:
        engine.lib().p3hip_destroy(h)
    else:
        assert err.startswith("no HIP device"), err


@pytest.mark.parametrize("d,heads", [(64, 4), (128, 8), (80, 1), (80, 2), (416, 13), (256, 2), (32, 1)])
def test_create_refuses_unsupported_transformers_by_name(built, tmp_path, d, heads):
    """head width 16 or 128, d not a multiple of 32, d above 384 or below 64: the architecture message, naming the set"""
    from p3achygo_amd import netspec
    assert not netspec.transformer_supported(d, heads)
    cfg = netspec.transformer_config("unsupported", 2, d, heads)
    path = str(tmp_path / "u.p3w")
    netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
    h, err = _create(path)
    assert not h
    assert err.startswith("unsupported architecture") and netspec.TRANSFORMER_SET in err, err


def test_create_refuses_int8_transformers(built, tmp_path):
    from p3achygo_amd import engine, netspec
    cfg = netspec.WIDE_TRANSFORMER_CONFIGS["test_b2d256h4_tfm"]
    path = str(tmp_path / "t.p3w")
    netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
    L = engine.lib()
    h = L.p3hip_create(path.encode(), 4, 1, 0, engine.FLAG_INT8)
    assert not h and "INT8" in (L.p3hip_create_error() or b"").decode()


def test_transformer_set_is_stated_once_in_the_header():
    from p3achygo_amd import netspec
    hdr = open(os.path.join(ROOT, "include", "p3hip.h")).read()
    assert '"%s"' % netspec.TRANSFORMER_SET in hdr
