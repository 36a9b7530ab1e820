"""Transformer trunks of other widths and head counts (netspec.WIDE_TRANSFORMER_CONFIGS, csrc/transformer.hip) on the
HIP engine, through the C ABI: parity with the float64 restatement tests/tfm_restatement_dh.py at several batch sizes,
the zero padding of the residual stream, compaction, RUN_ALL_SLOTS, launch-graph replay, the NN cache and symmetry
averaging on one net of each head width, rows past 2^31 q / k / v elements, and the attention kernel's timing hook.

Tolerances, by the rule of tests/test_transformer_gpu.py: the bounds of tests/test_engine_gpu.py where the fp16
emulation (tfm_restatement_dh fp16=True) stays inside them, else twice the emulated error.  Emulated errors (16
positions each; raw outputs, move / value / score / opt-move probabilities, largest KL):
    test_b2d64h2_tfm     6.9e-3  4.0e-5  4.2e-4  1.7e-5  1.7e-5  4.0e-6
    test_b2d128h2_tfm    6.1e-3  1.8e-5  5.3e-4  8.4e-6  4.3e-5  7.6e-7
    test_b2d192h6_tfm    8.2e-3  4.0e-5  5.0e-4  1.7e-5  4.3e-5  7.7e-7
    test_b2d256h4_tfm    7.6e-3  6.5e-5  3.3e-4  8.6e-7  3.0e-5  6.2e-7
    test_b2d384h12_tfm   6.0e-3  3.8e-5  4.5e-4  1.8e-6  6.4e-5  9.8e-7
    test_b2d384h6_tfm    7.2e-3  2.8e-5  6.3e-4  6.2e-6  9.4e-5  1.2e-6
tests/test_transformer_widths_cpu.py re-measures them and checks they stay at or below half of every bound here.
"""
import os

import numpy as np
import pytest

from conftest import load_golden
from test_transformer_gpu import LOGIT_REL, PROB_KEYS, _kl

pytestmark = pytest.mark.gpu


def _tol(logit, move, value, score, opt, kl):
    return dict(logit=logit, prob={"move_probs": move, "value_probs": value, "score_probs": score,
                                   "opt_move_probs": opt}, kl=kl)


TOL = {
    "test_b2d64h2_tfm": _tol(1.4e-2, 8.0e-5, 8.4e-4, 5e-5, 5e-5, 8.0e-6),
    "test_b2d128h2_tfm": _tol(1.23e-2, 5e-5, 1.06e-3, 5e-5, 8.6e-5, 2e-6),
    "test_b2d192h6_tfm": _tol(1.65e-2, 8.1e-5, 1.01e-3, 5e-5, 8.7e-5, 2e-6),
    "test_b2d256h4_tfm": _tol(1.52e-2, 1.3e-4, 6.7e-4, 5e-5, 6.0e-5, 2e-6),
    "test_b2d384h12_tfm": _tol(1.21e-2, 7.6e-5, 9.1e-4, 5e-5, 1.29e-4, 2e-6),
    "test_b2d384h6_tfm": _tol(1.44e-2, 5.7e-5, 1.27e-3, 5e-5, 1.9e-4, 2.4e-6),
}
NETS = list(TOL)
PATH_NETS = ["test_b2d192h6_tfm", "test_b2d256h4_tfm"]   # head width 32 and 64


def _check(name, raw, res, g, i):
    t = TOL[name]
    want = g["raw"][i]
    assert not np.isnan(raw).any()
    assert (np.abs(raw - want) <= np.maximum(t["logit"], LOGIT_REL * np.abs(want))).all(), \
        (name, float(np.abs(raw - want).max()))
    for key in PROB_KEYS:
        got = np.ctypeslib.as_array(getattr(res, key))
        assert np.abs(got - g[key][i]).max() <= t["prob"][key], (name, key, float(np.abs(got - g[key][i]).max()))
        assert _kl(g[key][i], got) <= t["kl"], (name, key)
    assert np.array_equal(np.ctypeslib.as_array(res.move_logits), raw[:362])


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> .p3w of the fixture's weights (tests/tfm_restatement_dh.py fixture_weights)"""
    from p3achygo_amd import netspec
    from tfm_restatement_dh import fixture_weights
    d = tmp_path_factory.mktemp("tfm_dh")
    out = {}
    for name in NETS:
        cfg, W = fixture_weights(name)
        out[name] = os.path.join(d, name + ".p3w")
        netspec.save_p3w(out[name], cfg, W)
    return out


def _raws(eng, slots):
    return [eng.get_raw(s).copy() for s in slots]


@pytest.mark.parametrize("name", NETS)
def test_engine_matches_the_restatement_at_batch_sizes(built, files, name):
    """batch 1, 7, 61 and 1024 (slot s holds golden position (7 s + batch) mod 16): every 64-token tile of qkv / ffn past
    the first spans two positions, and at 1024 every copy of a position is bit-identical"""
    from p3achygo_amd import engine, netspec
    g, pos = load_golden(name)
    n = len(pos)
    for batch in (1, 7, 61, 1024):
        idx = (7 * np.arange(batch) + batch) % n
        eng = engine.HipEngine(files[name], batch)
        eng.load_all(pos[idx])
        eng.RunInference()
        raws = np.stack(_raws(eng, range(batch)))
        first = {}
        for s in range(batch):
            _check(name, raws[s], eng.GetBatch(s), g, idx[s])
            first.setdefault(int(idx[s]), s)
            assert np.array_equal(raws[s], raws[first[int(idx[s])]]), (name, batch, s)
        if batch == 1024:
            t, c3 = eng.flops_per_position()
            assert c3 == 0 and abs(t - netspec.flops_per_position(netspec.get_config(name))[0]) < 1.0
        eng.close()


@pytest.mark.parametrize("name", ["test_b2d64h2_tfm", "test_b2d192h6_tfm"])
def test_residual_padding_channels_stay_zero(built, files, name):
    from p3achygo_amd import engine, netspec
    d = netspec.get_config(name).channels
    cs = 128 if d <= 128 else (256 if d <= 256 else 384)
    assert cs > d
    _, pos = load_golden(name)
    eng = engine.HipEngine(files[name], len(pos))
    eng.load_all(pos)
    eng.RunInference()
    x = eng.debug_x(len(pos), cs)
    assert np.all(x[:, d:] == 0)
    assert np.abs(x[:, :d]).max() > 0
    eng.close()


@pytest.mark.parametrize("name", PATH_NETS)
def test_compaction_and_run_all_slots(built, files, name):
    from p3achygo_amd import engine
    g, pos = load_golden(name)
    eng = engine.HipEngine(files[name], 40)
    for s in range(32):
        eng.LoadBatch(s, pos[s % 16:s % 16 + 1])
    eng.RunInference()
    full = _raws(eng, range(32))
    part = [2, 9, 10, 31]
    for s in part:
        eng.LoadBatch(s, pos[s % 16:s % 16 + 1])
    eng.RunInference()
    assert all(np.array_equal(a, full[s]) for a, s in zip(_raws(eng, part), part))
    eng.close()
    eng = engine.HipEngine(files[name], 8, flags=engine.FLAG_RUN_ALL_SLOTS)
    eng.LoadBatch(5, pos[5:6])
    eng.RunInference()
    assert np.array_equal(eng.get_raw(5), full[5])
    _check(name, eng.get_raw(5), eng.GetBatch(5), g, 5)
    eng.GetBatch(0)                                      # every slot of the static batch was run
    eng.close()


@pytest.mark.parametrize("name", PATH_NETS)
def test_launch_graph_replays_bit_for_bit(built, files, name):
    from p3achygo_amd import engine
    _, pos = load_golden(name)
    B = 48
    tiled = pos[np.arange(B) % 16]
    ref = engine.HipEngine(files[name], B)
    gr = engine.HipEngine(files[name], B, flags=engine.FLAG_LAUNCH_GRAPH)
    ref.load_all(tiled)
    ref.RunInference()
    want = _raws(ref, range(B))
    for rnd in range(4):                       # eager, capture, replay, replay
        gr.load_all(tiled)
        gr.RunInference()
        assert all(np.array_equal(a, b) for a, b in zip(want, _raws(gr, range(B)))), rnd
        assert gr.graph_state() == (1 if rnd >= 1 else 0)
    ref.close()
    gr.close()


@pytest.mark.parametrize("name", PATH_NETS)
def test_nn_cache_hits_are_bit_identical(built, files, name):
    from p3achygo_amd import engine
    _, pos = load_golden(name)
    key = lambda i: (0x9E3779B97F4A7C15 * (i + 1) & (2**64 - 1), 0xC2B2AE3D27D4EB4F * (i + 7) & (2**64 - 1))
    eng = engine.HipEngine(files[name], 16)
    eng.EnableCache(8)
    for s in range(16):
        eng.LoadBatchKeyed(s, pos[s:s + 1], *key(s), symmetry=s % 8)
    eng.RunInference()
    want = _raws(eng, range(16))
    for s in range(16):
        k = 15 - s
        eng.LoadBatchKeyed(s, pos[(k + 5) % 16:(k + 5) % 16 + 1], *key(k), symmetry=1)
    eng.RunInference()
    for s in range(16):
        _, sym, hit = eng.GetBatchKeyed(s)
        assert hit and sym == (15 - s) % 8 and np.array_equal(eng.get_raw(s), want[15 - s])
    eng.close()


@pytest.mark.parametrize("name", PATH_NETS)
def test_symmetry_averaging_is_the_restated_reduce(built, files, name):
    """the k-copy reduce of tests/symavg_restatement.py over a plain engine's copies, bit for bit"""
    from p3achygo_amd import engine, features
    from test_symmetry_avg_gpu import _check_rule
    _check_rule(files[name], features.random_positions(21, seed=47), engine.symmetry_maps()[0], masks=(0x01, 0x81, 0xFF))


NPOS = 61


def _row_limit_positions(built):
    from p3achygo_amd import features
    return features.random_positions(NPOS, seed=61, n_games=41, max_moves=330, komis=(7.5, -7.5, 0.5))


def _out(eng, s):
    r = eng.GetBatch(s)
    return np.concatenate([eng.get_raw(s), np.ctypeslib.as_array(r.move_probs),
                           np.ctypeslib.as_array(r.value_probs)]).astype(np.float32).view(np.uint32)


def _load(eng, pos, n):
    """slot s holds position (7 s + n) mod 61"""
    idx = (7 * np.arange(n) + n) % NPOS
    eng.load_all(pos[idx])
    return idx


def test_rows_past_2_31_qkv_elements_d384h12(built, files):
    """16,384 rows of 384 x 384 q (and k, v) elements: 2.4e9 elements, the offset passes 2^31 from row 14,564 on; every
    slot bit-identical to a 61-position run of the same position"""
    from p3achygo_amd import engine
    name = "test_b2d384h12_tfm"
    pos = _row_limit_positions(built)
    eng = engine.HipEngine(files[name], NPOS)
    eng.load_all(pos)
    eng.RunInference()
    ref = [_out(eng, s) for s in range(NPOS)]
    eng.close()
    rows = 16384
    assert rows * 384 * 384 > 2 ** 31
    eng = engine.HipEngine(files[name], rows)
    idx = _load(eng, pos, rows)
    eng.RunInference()
    bad = [s for s in range(rows) if not np.array_equal(_out(eng, s), ref[idx[s]])]
    eng.close()
    assert not bad, (len(bad), bad[:8], [b for b in bad if b >= 14564][:8])


def test_symmetry_averaged_rows_past_2_31_qkv_elements_d384h6(built, files):
    """batch 2,048 under all eight symmetries: 16,384 rows of q / k / v; every slot bit-identical to a 61-slot
    symmetry-averaged run of the same position"""
    from p3achygo_amd import engine
    name = "test_b2d384h6_tfm"
    pos = _row_limit_positions(built)
    eng = engine.HipEngine(files[name], NPOS, flags=engine.FLAG_SYMMETRY_AVG)
    eng.load_all(pos)
    eng.RunInference()
    ref = [_out(eng, s) for s in range(NPOS)]
    eng.close()
    batch = 2048
    eng = engine.HipEngine(files[name], batch, flags=engine.FLAG_SYMMETRY_AVG)
    idx = _load(eng, pos, batch)
    eng.RunInference()
    bad = [s for s in range(batch) if not np.array_equal(_out(eng, s), ref[idx[s]])]
    eng.close()
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("name", PATH_NETS)
def test_trunk_kernel_timing_names_the_attention_kernel(built, files, name):
    from p3achygo_amd import engine, netspec
    _, pos = load_golden(name)
    d = netspec.get_config(name).channels
    eng = engine.HipEngine(files[name], 64)
    eng.load_all(pos[np.arange(64) % 16])
    eng.upload()
    ms, fl, kname = eng.time_trunk_kernel(64, 2)
    assert ms > 0 and kname == "k_tfm_attn" and fl == 2.0 * 64 * 2 * 361 * 361 * d
    eng.close()
