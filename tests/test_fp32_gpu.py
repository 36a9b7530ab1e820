"""The fp32 plan of the conv trunks (P3HIP_FLAG_FP32, csrc/conv_f32.hip) on the HIP engine, through the C ABI: parity
with the float64 restatement at several batch sizes, every block on its own against float64 and the fp32 twin, the zero
padding of C and C_b, compaction, RUN_ALL_SLOTS, launch-graph replay, symmetry averaging, the NN cache, activation
offsets past 2^32 bytes and 2^31 elements, the timing hook and an evaluation match with one fp32 player.

Bounds on the outputs (tests/fp32_common.py): those tests/test_oracle_cpu.py sets for the fp32 C oracle against the
float64 fixtures: all 1889 raw outputs 2e-5 and the four probability vectors 1e-6 on the 3-5 block nets, 1e-4 and 2e-6
on b12c256btl3.  Largest errors against the float64 restatement (16 positions, seed 11; b12c256btl3: its 32 golden
positions), the twin on the CPU (tests/test_fp32_cpu.py re-measures it) and the engine on an MI355X, over the batches
1, 7, 61 and 300:
                          twin raw  twin prob   MI355X raw  MI355X prob
    test_b3c128btl2       9.4e-7    1.6e-7      1.36e-6     8.4e-8
    test_b3c256nbt        1.5e-6    1.1e-7      9.1e-7      1.7e-7
    test_b3c384btl3       1.2e-6    1.1e-7      1.68e-6     7.9e-8
    test_b3c192classic    1.4e-6    1.3e-7      1.45e-6     1.3e-7
    test_b5c256btl2_i2    1.6e-6    8.8e-8      1.99e-6     9.1e-8
    test_b3c96nbt         1.6e-6    1.9e-7      1.75e-6     1.6e-7
    test_b3c320nbt        1.8e-6    1.6e-7      1.34e-6     1.6e-7
    test_b4c512btl3_i2    1.3e-6    1.3e-7      2.05e-6     1.1e-7
    b12c256btl3           4.8e-6    3.0e-7      4.77e-6     1.2e-7
(the fixture of b12c256btl3 stores its float64 outputs as float32, which is most of both its columns).  The engine
stays 9 times inside the raw bound and 6 times inside the probability bound on the small nets, 20 and 16 times on
b12c256btl3.
Block by block (test_blocks_against_float64_and_the_twin): max |x - x_f64| / block_scale of every block from the engine's
own x before it, the engine's and the twin's on that same input (37 positions); the engine must stay within 4 x the
twin's.  Largest per net, stem and blocks:
                          twin stem  MI355X stem  twin block           MI355X block
    test_b3c320nbt        1.60e-6    1.60e-6      2.61e-6 (broadcast)  1.33e-6 (broadcast)
    test_b4c512btl3_i2    1.69e-6    1.69e-6      3.94e-6 (broadcast)  1.37e-6 (broadcast)
    test_b3c192classic    1.23e-6    1.23e-6      1.16e-6 (classic)    1.59e-6 (classic)
    test_b3c128btl2       1.24e-6    1.24e-6      1.80e-6 (broadcast)  1.23e-6 (broadcast)
The largest ratio engine / twin on any block is 1.38 (test_b3c192classic block 0: 1.59e-6 against 1.15e-6); the stems
agree to three digits.  A first version of the layer conv that summed all of K in one chain of MFMAs measured 5.18e-6
and 6.10e-6 on the two classic blocks, 4.5 and 4.8 times the twin and over the factor 4; every K slice is now summed
on its own (csrc/conv_f32.hip k_lconv_f32).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fp32_common as fc  # noqa: E402

pytestmark = pytest.mark.gpu

PATH_NETS = ["test_b3c128btl2", "test_b3c320nbt"]   # a fused shape replanned layer by layer, a padded runtime width


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> .p3w of netspec.generate_weights(cfg, randomize=True), written on demand"""
    from p3achygo_amd import netspec
    d = tmp_path_factory.mktemp("fp32")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = os.path.join(d, name + ".p3w")
            netspec.save_p3w(cache[name], fc.config(name), fc.weights(name))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def reference():
    """name -> (positions, float64 outputs of them), computed once per net"""
    cache = {}

    def get(name):
        if name not in cache:
            if name == fc.DEEP_NET:
                cache[name] = fc.golden_reference(name)
            else:
                pos = fc.positions()
                cache[name] = (pos, fc.outputs(fc.restatement(fc.config(name), fc.weights(name)), pos))
        return cache[name]
    return get


def _fp32(path, batch, flags=0):
    from p3achygo_amd import engine
    return engine.HipEngine(path, batch, flags=flags | engine.FLAG_FP32)


def _raws(eng, slots):
    return [eng.get_raw(s).copy() for s in slots]


@pytest.mark.parametrize("name", fc.SMALL_NETS)
def test_engine_matches_the_restatement_at_batch_sizes(built, files, reference, name):
    """batch 1, 7, 61 and 300; slot s holds reference position (7 s + batch) mod 16; slots holding the same position
    are bit-identical across slots and batch sizes"""
    pos, ref = reference(name)
    n = len(pos)
    seen = {}
    worst = [0.0, 0.0]
    for batch in (1, 7, 61, 300):
        idx = (7 * np.arange(batch) + batch) % n
        eng = _fp32(files(name), batch)
        eng.load_all(pos[idx])
        eng.RunInference()
        raws = np.stack(_raws(eng, range(batch)))
        for s in range(batch):
            i = int(idx[s])
            if i not in seen:
                seen[i] = raws[s].copy()
            assert np.array_equal(raws[s], seen[i]), (name, batch, s)
            if s < 32 or s % 37 == 0:   # the record of every distinct position at every batch, and a sample beyond
                e = fc.check_outputs(name, raws[s], eng.GetBatch(s), eng.GetOwnership(s), ref, i, fc.RAW_TOL, fc.PROB_TOL)
                worst = [max(a, b) for a, b in zip(worst, e)]
        eng.close()
    print(f"fp32 outputs {name}: raw {worst[0]:.2e} prob {worst[1]:.2e}")


def test_deep_net_matches_its_golden_vectors(built, weight_files, reference):
    pos, ref = reference(fc.DEEP_NET)
    eng = _fp32(weight_files(fc.DEEP_NET), len(pos))
    eng.load_all(pos)
    eng.RunInference()
    worst = [0.0, 0.0]
    for s in range(len(pos)):
        e = fc.check_outputs(fc.DEEP_NET, eng.get_raw(s), eng.GetBatch(s), eng.GetOwnership(s), ref, s, fc.DEEP_RAW_TOL,
                             fc.DEEP_PROB_TOL)
        worst = [max(a, b) for a, b in zip(worst, e)]
    eng.close()
    print(f"fp32 outputs {fc.DEEP_NET}: raw {worst[0]:.2e} prob {worst[1]:.2e}")


def _engine_xs(path, cfg, pos):
    """x after the stem and after every block (P3HIP_DEBUG_STOP_BLOCK, read at create), cut to the file's C"""
    C, Cp = cfg.channels, fc.padded(cfg.channels)
    old = os.environ.get("P3HIP_DEBUG_STOP_BLOCK")
    xs = []
    try:
        for stop in range(cfg.blocks + 1):
            os.environ["P3HIP_DEBUG_STOP_BLOCK"] = str(stop)
            eng = _fp32(path, len(pos))
            eng.load_all(pos)
            eng.RunInference()
            xs.append(eng.debug_x(len(pos), Cp)[:, :C].copy())
            eng.close()
    finally:
        if old is None:
            os.environ.pop("P3HIP_DEBUG_STOP_BLOCK", None)
        else:
            os.environ["P3HIP_DEBUG_STOP_BLOCK"] = old
    return xs


@pytest.mark.parametrize("name", fc.BLOCK_NETS)
def test_blocks_against_float64_and_the_twin(built, files, name):
    """the stem and every block from the engine's own x before it: the error against float64 within 4 x the twin's"""
    from p3achygo_amd import features
    cfg, W = fc.config(name), fc.weights(name)
    pos = features.random_positions(37, seed=43, n_games=16, max_moves=300, komis=(7.5, -7.5, 0.5))
    rows = fc.block_errors(cfg, W, _engine_xs(files(name), cfg, pos), pos)
    for label, eng_err, twin_err in rows:
        print(f"fp32 blocks {name} {label}: engine {eng_err:.2e} twin {twin_err:.2e}")
    for label, eng_err, twin_err in rows:
        assert np.isfinite(eng_err) and eng_err <= fc.BLOCK_FACTOR * twin_err, (name, label, eng_err, twin_err)


@pytest.mark.parametrize("name", fc.PADDED_NETS)
def test_padded_channels_of_the_stream_are_exactly_zero(built, files, reference, name):
    C = fc.config(name).channels
    Cp = fc.padded(C)
    pos, _ = reference(name)
    eng = _fp32(files(name), len(pos))
    eng.load_all(pos)
    eng.RunInference()
    x = eng.debug_x(len(pos), Cp)   # p3hip_debug_x returns the padded width
    assert np.all(x[:, C:] == 0)
    assert (np.abs(x[:, :C]).max(axis=(0, 2)) > 0).all()
    eng.close()


@pytest.mark.parametrize("name", PATH_NETS)
def test_compaction_and_run_all_slots(built, files, reference, name):
    from p3achygo_amd import engine
    pos, ref = reference(name)
    eng = _fp32(files(name), 16)
    eng.load_all(pos)
    eng.RunInference()
    full = _raws(eng, range(16))
    again = _fp32(files(name), 16)
    again.load_all(pos)
    again.RunInference()
    assert all(np.array_equal(a, b) for a, b in zip(_raws(again, range(16)), full))   # two runs on the same inputs
    again.close()
    for s in range(16):
        eng.GetBatch(s)
    part = [2, 9, 10, 13, 15]                      # 5 of 16 slots, two of them loaded again before the fetch
    for s in part + [9, 13]:
        eng.LoadBatch(s, pos[s:s + 1])
    eng.RunInference()
    assert all(np.array_equal(a, full[s]) for a, s in zip(_raws(eng, part), part))
    eng.close()
    eng = _fp32(files(name), 8, flags=engine.FLAG_RUN_ALL_SLOTS)
    eng.LoadBatch(5, pos[5:6])
    eng.RunInference()
    assert np.array_equal(eng.get_raw(5), full[5])
    fc.check_outputs(name, eng.get_raw(5), eng.GetBatch(5), eng.GetOwnership(5), ref, 5, fc.RAW_TOL, fc.PROB_TOL)
    eng.GetBatch(0)                                      # every slot of the static batch was run
    eng.close()


@pytest.mark.parametrize("name", PATH_NETS)
def test_launch_graph_replays_bit_for_bit(built, files, reference, name):
    from p3achygo_amd import engine
    pos, _ = reference(name)
    B = 48
    tiled = pos[np.arange(B) % 16]
    ref = _fp32(files(name), B)
    gr = _fp32(files(name), B, flags=engine.FLAG_LAUNCH_GRAPH)
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


def test_symmetry_averaging_is_the_restated_reduce(built, files):
    """the k-copy reduce of tests/symavg_restatement.py over the fp32 engine's own copies, bit for bit"""
    from p3achygo_amd import engine, features
    from test_symmetry_avg_gpu import _check_rule
    _check_rule(files("test_b3c128btl2"), features.random_positions(4, seed=47), engine.symmetry_maps()[0], masks=(0xFF,),
                flags=engine.FLAG_FP32)


@pytest.mark.parametrize("name", PATH_NETS)
def test_nn_cache_hits_are_bit_identical(built, files, reference, name):
    pos, _ = reference(name)
    key = lambda i: (0x9E3779B97F4A7C15 * (i + 1) & (2**64 - 1), 0xC2B2AE3D27D4EB4F * (i + 7) & (2**64 - 1))
    eng = _fp32(files(name), 16)
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


def test_activation_offsets_past_2_32_bytes_and_2_31_elements(built, files, reference):
    """11,700 rows of 512 x 361 fp32 activations: the byte offset of a row passes 2^32 from row 5,810 on, its element
    offset 2^31 from row 11,619 on; every slot bit-identical to the slot holding the same position at batch 61"""
    name, rows = fc.OFFSET_NET, 11700
    per = 512 * 361
    assert 5810 * per * 4 > 2 ** 32 > 5809 * per * 4 and rows * per > 11619 * per > 2 ** 31 > 11618 * per
    pos = fc.positions()

    def out(eng, s):
        r = eng.GetBatch(s)
        return np.concatenate([eng.get_raw(s), np.ctypeslib.as_array(r.move_probs),
                               np.ctypeslib.as_array(r.value_probs)]).astype(np.float32).view(np.uint32)
    eng = _fp32(files(name), 61)
    idx = (7 * np.arange(61) + 61) % 16
    eng.load_all(pos[idx])
    eng.RunInference()
    ref = {}
    for s in range(61):
        o = out(eng, s)
        assert np.array_equal(ref.setdefault(int(idx[s]), o), o)
    eng.close()
    assert len(ref) == 16
    eng = _fp32(files(name), rows)
    idx = (7 * np.arange(rows) + rows) % 16
    eng.load_all(pos[idx])
    eng.RunInference()
    bad = [s for s in range(rows) if not np.array_equal(out(eng, s), ref[int(idx[s])])]
    eng.close()
    assert not bad, (len(bad), bad[:8], [b for b in bad if b >= 5810][:8])


@pytest.mark.parametrize("name", ["test_b3c128btl2", "test_b3c192classic", "test_b3c96nbt"])
def test_trunk_kernel_timing_names_the_fp32_conv(built, files, reference, name):
    pos, _ = reference(name)
    cfg = fc.config(name)
    w3 = cfg.channels if cfg.block_type == "classic" else cfg.bottleneck_channels   # the file's width, unpadded
    eng = _fp32(files(name), 64)
    eng.load_all(pos[np.arange(64) % 16])
    eng.upload()
    ms, fl, kname = eng.time_trunk_kernel(64, 2)
    assert ms > 0 and kname == "k_lconv_f32<3>" and fl == 2.0 * 9 * w3 * w3 * 361 * 64
    eng.close()


def test_eval_match_with_one_fp32_player(built, files):
    from p3achygo_amd import host_api
    w = files("test_b3c128btl2")
    try:
        host_api.eval_set_player_flags(cur="n: 8\n", cand="n: 8\nnn_fp32: 1\n")
        st = host_api.eval_match(w, w, num_games=4, visits_per_move=8, leaves_per_round=4, max_moves=24, num_threads=2, seed=2)
    finally:
        host_api.eval_set_player_flags()
    assert st.games == 4 and st.cur_wins + st.cand_wins + st.draws == 4
