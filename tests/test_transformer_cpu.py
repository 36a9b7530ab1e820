"""The transformer trunk without a GPU: the engine's RoPE table against the one the reference computes, the float64
restatement against its own fixtures, the .p3w header and tensors of transformer configs, FLOP counts, and the error
the kernels' fp16 storage points alone must produce (against the bounds tests/test_transformer_gpu.py sets)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import tfm_restatement as tfm  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
PROB_KEYS = ("move_probs", "value_probs", "score_probs", "opt_move_probs")


def _weights(name):
    return tfm.fixture_weights(name)[1]


def test_engine_rope_table_matches_the_reference_fixture(built):
    from p3achygo_amd import engine
    d = np.load(os.path.join(GOLD, "rope_spiral_d32_r4_b19.npz"))
    cos, sin = engine.rope_table()
    assert np.abs(cos - d["cos"]).max() <= 1e-12 and np.abs(sin - d["sin"]).max() <= 1e-12
    rc, rs = tfm.rope_tables()
    assert np.abs(rc - d["cos"]).max() <= 1e-12 and np.abs(rs - d["sin"]).max() <= 1e-12


def test_restatement_reproduces_the_short_golden():
    from p3achygo_amd import netspec
    g, _ = load_golden("test_b2d96h3_tfm")
    cfg = netspec.TRANSFORMER_CONFIGS["test_b2d96h3_tfm"]
    n = 8
    out = tfm.forward(cfg, _weights("test_b2d96h3_tfm"), g["planes"][:n].astype(np.float32), g["scalars"][:n])
    # the fixture holds the float64 outputs rounded once to float32
    assert np.abs(out["raw"] - g["raw"][:n]).max() <= 1e-6 * max(1.0, float(np.abs(g["raw"][:n]).max()))
    for k in PROB_KEYS:
        assert np.abs(out[k] - g[k][:n]).max() <= 1e-7


def test_golden_weights_are_the_seeded_ones_with_scaled_q_and_k():
    from p3achygo_amd import netspec
    for name in ("test_b2d96h3_tfm", "b14d96h3_transformer"):
        g, _ = load_golden(name)
        W = _weights(name)
        plain = netspec.generate_weights(netspec.TRANSFORMER_CONFIGS[name], randomize=True)
        assert np.array_equal(W["blocks.1.q.w"], (plain["blocks.1.q.w"] * np.float32(1.5)).astype(np.float32))
        assert float(g["qk_scale"]) == tfm.QK_SCALE
        wsum = sum(float(w.astype(np.float64).sum()) for w in W.values())
        wsq = sum(float((w.astype(np.float64) ** 2).sum()) for w in W.values())
        assert np.allclose(g["weight_checksum"], [wsum, wsq], rtol=1e-12, atol=1e-9)
        assert (g["attn_peak"] >= 0.05).all()


def test_p3w_round_trip_of_transformer_configs(tmp_path):
    from p3achygo_amd import netspec
    for name, cfg in netspec.TRANSFORMER_CONFIGS.items():
        W = netspec.generate_weights(cfg, randomize=True)
        p = str(tmp_path / (name + ".p3w"))
        netspec.save_p3w(p, cfg, W)
        with open(p, "rb") as f:
            hdr = np.frombuffer(f.read(44), "<i4", offset=4)
        # version, blocks, C, Cb = heads, H, V, bcast_interval, inner_layers, block_type, ntensors
        assert list(hdr[:9]) == [1, cfg.blocks, 96, 3, 32, 64, 0, 0, 3]
        c2, W2, v = netspec.load_p3w(p)
        assert (c2.blocks, c2.channels, c2.bottleneck_channels, c2.block_type) == (cfg.blocks, 96, 3, "transformer")
        assert set(W2) == set(W) and all(np.array_equal(W2[k], W[k]) for k in W)
        assert W["blocks.0.ffn_gate.w"].shape == (96, 192) and W["blocks.0.ffn_down.w"].shape == (192, 96)
        assert W["blocks.0.q.w"].shape == (96, 96) and W["blocks.0.rms_in.scale"].shape == (96,)
        assert 0.5 <= W["blocks.0.rms_in.scale"].min() and W["blocks.0.rms_out.scale"].max() <= 1.5
        assert not any(k.startswith("blocks.0.bn") for k in W)
    assert not set(netspec.TRANSFORMER_CONFIGS) & set(netspec.CONFIGS)


# sha256 of the .p3w of every convolutional config (randomize=True), as written before transformer configs existed
def test_existing_configs_write_the_same_files(tmp_path):
    import hashlib
    from p3achygo_amd import netspec
    digests = {}
    for name, cfg in netspec.CONFIGS.items():
        p = str(tmp_path / (name + ".p3w"))
        netspec.save_p3w(p, cfg, netspec.generate_weights(cfg, randomize=True))
        digests[name] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    want = dict(line.split() for line in open(os.path.join(GOLD, "p3w_sha256_conv_configs.txt")).read().splitlines())
    assert digests == want


def test_flops_per_position():
    from p3achygo_amd import netspec
    cfg = netspec.TRANSFORMER_CONFIGS["b14d96h3_transformer"]
    total, c3 = netspec.flops_per_position(cfg)
    L, C = 361, 96
    per_block = 2 * (3 * L * C * C + L * L * C + L * L * C + L * C * C + 2 * L * C * 2 * C + L * 2 * C * C)
    assert abs(per_block / 1e6 - 116.6) < 0.1            # QKV 20.0, QK^T 25.0, PV 25.0, O 6.7, gate+up 26.6, down 13.3
    assert c3 == 0 and abs(total / 1e9 - 1.665) < 1e-3
    stem_heads = netspec.flops_per_position(netspec.TRANSFORMER_CONFIGS["test_b2d96h3_tfm"])[0] - 2 * per_block
    assert abs(total - (14 * per_block + stem_heads)) < 1.0
    ref = netspec.flops_per_position(netspec.CONFIGS["b12c256btl3"])[0]
    assert abs(total / ref - 0.41) < 0.01


@pytest.mark.parametrize("name", ["test_b2d96h3_tfm", "b14d96h3_transformer"])
def test_fp16_storage_emulation_stays_inside_half_the_gpu_bounds(name):
    """The error the fp16 storage points alone produce (rounded where transformer.hip stores fp16) is inside every
    bound tests/test_transformer_gpu.py holds the engine to, and at most half of each bound raised there (all but
    the score probabilities')."""
    from p3achygo_amd import netspec
    from test_transformer_gpu import TOL, _kl
    g, _ = load_golden(name)
    cfg = netspec.TRANSFORMER_CONFIGS[name]
    out = tfm.forward(cfg, _weights(name), g["planes"].astype(np.float32), g["scalars"], fp16=True)
    t = TOL[name]
    raw = g["raw"]
    assert (np.abs(out["raw"] - raw) <= np.maximum(t["logit"], 1e-3 * np.abs(raw)) / 2).all()
    for k in PROB_KEYS:
        assert np.abs(out[k] - g[k]).max() <= t["prob"][k] / (1 if k == "score_probs" else 2), k
        assert max(_kl(g[k][i], out[k][i]) for i in range(len(raw))) <= t["kl"] / 2, k
